"""gg_khop_aggregate inside the compiled reference, with the reference's own hash-aggregate plan of the same statement
(tests/khop_aggregate_ref.sql_khop_aggregate) over the same tables as the yardstick: no planner rule is on, so the joins and
the aggregate run as the reference plans them.  Both sides are read as text, the HUGEINT totals exactly."""
import os

import numpy as np
import pytest

from oracle import ref_duckdb as R
from tests import khop_aggregate_ref as K
from tests import triangles_ref as T

EXT = R.EXTENSION

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not (R.available() and os.path.exists(EXT)), reason="reference build / extension not present"),
]

GRAPH = "'person', 'p_personid', 'knows', 'k_person1id', 'k_person2id'"


@pytest.fixture(scope="module")
def db():
    vid, src, dst = T.hard_graph()
    g = T.TriangleGraph(vid, src, dst)
    rng = np.random.RandomState(0xA66)
    w = rng.randint(-(1 << 62), 1 << 62, size=g.V, dtype=np.int64) * 2 + rng.randint(0, 2, size=g.V)
    w[:4] = [-(1 << 63), (1 << 63) - 1, -1, 0]
    d = R.RefDuckDB(threads=4)
    d.load_table("person", {"p_personid": vid, "p_score": w})
    d.load_table("knows", {"k_person1id": src, "k_person2id": dst})
    d.execute(f"LOAD '{EXT}'")
    indeg = np.bincount(g.dv, minlength=g.V)
    three = np.unique(g.vid[[int(indeg.argmax()), 3] + np.nonzero(g.A.diagonal())[0].tolist()[:1]])
    assert three.size == 3  # the hub, dense index 3, a self-loop vertex
    yield d, g, three
    d.close()


def in_list(ids):
    return "'SELECT p_personid FROM person WHERE p_personid IN (" + ", ".join(str(int(s)) for s in ids) + ")'"


def function_rows(d, sources_sql, hops, group_by, weight="'p_score'", graph=GRAPH):
    rows = d.query_text(f"SELECT vertex, walks, total FROM gg_khop_aggregate({graph}, {sources_sql}, {hops}, '{group_by}', "
                        f"{weight}) ORDER BY vertex")
    return [tuple(int(x) for x in r) for r in rows]


def reference_rows(d, hops, group_by, sources, weighted=True):
    rows = d.query_text(K.sql_khop_aggregate(hops, group_by, sources, weighted))
    return sorted(tuple(int(x) for x in r) for r in rows)


@pytest.mark.parametrize("group_by", K.GROUPS)
@pytest.mark.parametrize("hops", [1, 2])
def test_equals_the_reference_hash_aggregate_plan(db, hops, group_by):
    d, g, three = db
    want_all = reference_rows(d, hops, group_by, None)
    assert len(want_all) > 0 and any(abs(t) >= 1 << 63 for _, _, t in want_all)  # the HUGEINT column is needed
    for all_sources in ("NULL", "''"):
        assert function_rows(d, all_sources, hops, group_by) == want_all
    want = reference_rows(d, hops, group_by, three)
    assert len(want) > 0 and function_rows(d, in_list(three), hops, group_by) == want
    # without a weight column: counts only, total = walks
    counts = function_rows(d, in_list(three), hops, group_by, "NULL")
    assert counts == reference_rows(d, hops, group_by, three, weighted=False) == [(v, n, n) for v, n, _ in want]
    assert function_rows(d, "NULL", hops, group_by, "NULL") == [(v, n, n) for v, n, _ in want_all]


def test_a_null_weight_weighs_nothing(db):
    d, g, three = db
    d.execute("CREATE TABLE person_nulls AS SELECT p_personid, CASE WHEN p_personid % 3 = 0 THEN NULL ELSE p_score END "
              "AS p_score FROM person")
    try:
        got = function_rows(d, "NULL", 2, "start", graph="'person_nulls', 'p_personid', 'knows', 'k_person1id', 'k_person2id'")
        sql = K.sql_khop_aggregate(2, "start").replace("person p", "person_nulls p").replace("sum(p2.p_score)",
                                                                                              "sum(coalesce(p2.p_score, 0))")
        assert got == sorted(tuple(int(x) for x in r) for r in d.query_text(sql)) and len(got) > 0
    finally:
        d.execute("DROP TABLE person_nulls")


def test_over_a_pinned_graph_twice(db):
    d, g, three = db
    want = reference_rows(d, 2, "end", three)
    d.execute("PRAGMA gg_use_pinned_graphs")
    try:
        d.execute(f"SELECT * FROM gg_graph_pin({GRAPH})")
        for _ in range(2):
            assert function_rows(d, in_list(three), 2, "end") == want
        assert int(d.execute("SELECT * FROM gg_graph_pins()")[0, 0]) == 1
    finally:
        d.execute("SELECT * FROM gg_graph_unpin()")
        d.execute("PRAGMA gg_ignore_pinned_graphs")


def test_bad_arguments_raise_and_the_connection_stays_usable(db):
    d, g, three = db
    s = in_list(three)
    bad = [
        f"'person', 'p_personid', 'knows', 'no_such_column', 'k_person2id', {s}, 2, 'start', 'p_score'",  # a missing column
        f"{GRAPH}, {s}, 2, 'start', 'no_such_weight'",
        f"{GRAPH}, {s}, 2, 'middle', 'p_score'",  # a bad group_by
        f"{GRAPH}, {s}, 0, 'start', 'p_score'",   # hops outside 1..GG_MAX_HOPS
        f"{GRAPH}, {s}, 9, 'end', 'p_score'",
    ]
    for args in bad:
        with pytest.raises(RuntimeError):
            d.execute(f"SELECT count(*) FROM gg_khop_aggregate({args})")
    assert function_rows(d, s, 1, "start") == reference_rows(d, 1, "start", three)
