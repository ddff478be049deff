"""gg_khop_aggregate_top inside the compiled reference, with the reference's own TopN above its hash-aggregate plan of the
same statement (tests/khop_aggregate_top_ref.sql_khop_aggregate_top: ORDER BY ... LIMIT n) over the same tables as the
yardstick: no planner rule is on.  Both sides are read as text in result order, the HUGEINT totals exactly."""
import os

import numpy as np
import pytest

from oracle import ref_duckdb as R
from tests import khop_aggregate_top_ref as KT
from tests import triangles_ref as T

EXT = R.EXTENSION

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not (R.available() and os.path.exists(EXT)), reason="reference build / extension not present"),
]

GRAPH = "'person', 'p_personid', 'knows', 'k_person1id', 'k_person2id'"
GROUPS = ("start", "end")
# (order_by, descending, biased)
ORDERS = [("total", True, False), ("total", False, False), ("total", True, True), ("total", False, True),
          ("walks", True, False), ("walks", False, False)]


@pytest.fixture(scope="module")
def db():
    """weights of +-2^62 and thereabouts: two-hop sums pass int64 (the HUGEINT column is needed) and no bias + sum leaves
    128 bits, where the reference would raise and the library wrap"""
    vid, src, dst = T.hard_graph()
    g = T.TriangleGraph(vid, src, dst)
    rng = np.random.RandomState(0xA66)
    w = rng.randint(-(1 << 62), 1 << 62, size=g.V, dtype=np.int64) * 2 + rng.randint(0, 2, size=g.V)
    w[:4] = [-(1 << 63), (1 << 63) - 1, -1, 0]
    bias = rng.randint(-(1 << 62), 1 << 62, size=g.V, dtype=np.int64)
    bias[:4] = [(1 << 63) - 1, -(1 << 63), 1, -1]
    d = R.RefDuckDB(threads=4)
    d.load_table("person", {"p_personid": vid, "p_score": w, "p_bias": bias})
    d.load_table("knows", {"k_person1id": src, "k_person2id": dst})
    d.execute(f"LOAD '{EXT}'")
    indeg = np.bincount(g.dv, minlength=g.V)
    three = np.unique(g.vid[[int(indeg.argmax()), 3] + np.nonzero(g.A.diagonal())[0].tolist()[:1]])
    assert three.size == 3  # the hub, dense index 3, a self-loop vertex
    yield d, g, three
    d.close()


def in_list(ids):
    return "'SELECT p_personid FROM person WHERE p_personid IN (" + ", ".join(str(int(s)) for s in ids) + ")'"


def function_rows(d, sources_sql, hops, group_by, n, order_by="total", descending=True, biased=False, weight="'p_score'",
                  graph=GRAPH):
    rows = d.query_text(
        f"SELECT rank, vertex, walks, total FROM gg_khop_aggregate_top({graph}, {sources_sql}, {hops}, '{group_by}', "
        f"{weight}, '{order_by}', {'true' if descending else 'false'}, {'NULL' if not biased else repr('p_bias')}, {n}) "
        "ORDER BY rank")
    rows = [tuple(int(x) for x in r) for r in rows]
    assert [r[0] for r in rows] == list(range(len(rows)))  # rank is 0 .. rows - 1
    return [r[1:] for r in rows]


def reference_rows(d, hops, group_by, n, order_by="total", descending=True, biased=False, sources=None, weighted=True):
    sql = KT.sql_khop_aggregate_top(hops, group_by, n, order_by, descending, sources, weighted, biased)
    return [tuple(int(x) for x in r[:3]) for r in d.query_text(sql)]  # in result order, not re-sorted


@pytest.mark.parametrize("group_by", GROUPS)
@pytest.mark.parametrize("hops", [1, 2])
def test_equals_the_reference_order_by_limit_row_for_row(db, hops, group_by):
    d, g, three = db
    everything = reference_rows(d, hops, group_by, 1 << 20)
    groups = len(everything)
    assert groups > 20 and any(abs(t) >= 1 << 63 for _, _, t in everything)  # the HUGEINT column is needed
    for order_by, descending, biased in ORDERS:
        for n in (1, 20, groups + 9):
            want = reference_rows(d, hops, group_by, n, order_by, descending, biased)
            assert len(want) == min(n, groups)
            assert function_rows(d, "NULL", hops, group_by, n, order_by, descending, biased) == want
    # from an IN list (three groups by the start, many by the end), with and without the weight column
    for order_by, descending, biased in ORDERS:
        for n in (1, 2, 5000):
            want = reference_rows(d, hops, group_by, n, order_by, descending, biased, three)
            assert len(want) > 0
            assert function_rows(d, in_list(three), hops, group_by, n, order_by, descending, biased) == want
    counts = function_rows(d, in_list(three), hops, group_by, 20, "total", True, False, "NULL")
    assert counts == reference_rows(d, hops, group_by, 20, "total", True, False, three, weighted=False)
    assert all(walks == total for _, walks, total in counts)
    # n = 0: no row; the statement above the function sees an ordinary table
    assert function_rows(d, "NULL", hops, group_by, 0) == []
    assert int(d.execute(f"SELECT count(*) FROM gg_khop_aggregate_top({GRAPH}, NULL, {hops}, '{group_by}', 'p_score', "
                         "'walks', true, NULL, 33)")[0, 0]) == min(33, groups)


def test_over_a_pinned_graph_twice(db):
    d, g, three = db
    want = reference_rows(d, 2, "end", 20, "total", True, True, three)
    d.execute("PRAGMA gg_use_pinned_graphs")
    try:
        d.execute(f"SELECT * FROM gg_graph_pin({GRAPH})")
        for _ in range(2):
            assert function_rows(d, in_list(three), 2, "end", 20, "total", True, True) == want
        assert int(d.execute("SELECT * FROM gg_graph_pins()")[0, 0]) == 1
    finally:
        d.execute("SELECT * FROM gg_graph_unpin()")
        d.execute("PRAGMA gg_ignore_pinned_graphs")


def test_a_null_bias_adds_nothing(db):
    d, g, three = db
    d.execute("CREATE TABLE person_nulls AS SELECT p_personid, p_score, CASE WHEN p_personid % 3 = 0 THEN NULL ELSE p_bias "
              "END AS p_bias FROM person")
    try:
        got = function_rows(d, "NULL", 1, "start", 50, "total", True, True,
                            graph="'person_nulls', 'p_personid', 'knows', 'k_person1id', 'k_person2id'")
        sql = KT.sql_khop_aggregate_top(1, "start", 50, "total", True, biased=True)
        sql = sql.replace("person p", "person_nulls p").replace("p0.p_bias + sum", "coalesce(p0.p_bias, 0) + sum")
        assert "coalesce" in sql
        assert got == [tuple(int(x) for x in r[:3]) for r in d.query_text(sql)] and len(got) == 50
    finally:
        d.execute("DROP TABLE person_nulls")


def test_bad_arguments_raise_and_the_connection_stays_usable(db):
    d, g, three = db
    s = in_list(three)
    tail = "'total', true, 'p_bias', 10"
    bad = [
        f"'person', 'p_personid', 'knows', 'no_such_column', 'k_person2id', {s}, 2, 'start', 'p_score', {tail}",
        f"{GRAPH}, {s}, 2, 'start', 'no_such_weight', {tail}",
        f"{GRAPH}, {s}, 2, 'start', 'p_score', 'total', true, 'no_such_bias', 10",
        f"{GRAPH}, {s}, 2, 'middle', 'p_score', {tail}",                       # a bad group_by
        f"{GRAPH}, {s}, 0, 'start', 'p_score', {tail}",                        # hops outside 1..GG_MAX_HOPS
        f"{GRAPH}, {s}, 9, 'end', 'p_score', {tail}",
        f"{GRAPH}, {s}, NULL, 'end', 'p_score', {tail}",                       # NULL hops / group_by / order_by / n / descending
        f"{GRAPH}, {s}, 2, NULL, 'p_score', {tail}",
        f"{GRAPH}, {s}, 2, 'end', 'p_score', NULL, true, 'p_bias', 10",
        f"{GRAPH}, {s}, 2, 'end', 'p_score', 'total', true, 'p_bias', NULL",
        f"{GRAPH}, {s}, 2, 'end', 'p_score', 'total', NULL, 'p_bias', 10",     # NULL descending
        f"{GRAPH}, {s}, 2, 'end', 'p_score', 'total', true, 'p_bias', -1",     # a negative n
        f"{GRAPH}, {s}, 2, 'end', 'p_score', 'sum', true, 'p_bias', 10",       # an unknown order_by
        f"{GRAPH}, {s}, 2, 'end', 'p_score', 'walks', true, 'p_bias', 10",     # a bias with the walks
    ]
    for args in bad:
        with pytest.raises(RuntimeError):
            d.execute(f"SELECT count(*) FROM gg_khop_aggregate_top({args})")
    assert function_rows(d, s, 1, "start", 2) == reference_rows(d, 1, "start", 2, sources=three)
