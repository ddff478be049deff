"""gg_khop_pair_counts inside the compiled reference, with the reference's own hash-aggregate plan on two keys of the same
statement (tests/khop_pair_counts_ref.sql_pair_counts) over the same tables as the yardstick: no planner rule is on, so the
joins and the aggregate run as the reference plans them.  Both sides are compared as sorted rows."""
import os

import numpy as np
import pytest

from oracle import ref_duckdb as R
from tests import khop_pair_counts_ref as P
from tests import triangles_ref as T

EXT = R.EXTENSION

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not (R.available() and os.path.exists(EXT)), reason="reference build / extension not present"),
]

GRAPH = "'person', 'p_personid', 'knows', 'k_person1id', 'k_person2id'"


@pytest.fixture(scope="module")
def db():
    vid, src, dst = T.hard_graph(V=300, rows=3000, seed=0x51, hub_fan=120)
    g = T.TriangleGraph(vid, src, dst)
    d = R.RefDuckDB(threads=4)
    d.load_table("person", {"p_personid": vid})
    d.load_table("knows", {"k_person1id": src, "k_person2id": dst})
    d.execute(f"LOAD '{EXT}'")
    hub = int(np.bincount(g.dv, minlength=g.V).argmax())
    loop = int(np.nonzero(g.A.diagonal())[0][0])
    six = [int(x) for x in g.vid[[hub, 3, loop, 17, 250]].tolist()] + [-123456789]  # the last one is no vertex
    assert len(set(six)) == 6
    seventy = [int(x) for x in g.vid[100:170].tolist()]  # two batches
    targets = [int(x) for x in g.vid[[3, 40, 7, 299, hub]].tolist()] + [-999]
    yield d, g, six, seventy, targets
    d.close()


def values(ids):
    """a relation of the ids as they stand, duplicates and NULLs included"""
    return "'SELECT x FROM (VALUES " + ", ".join("(NULL)" if s is None else f"({int(s)})" for s in ids) + ") t(x)'"


def function_rows(d, sources_sql, targets_sql, hops, graph=GRAPH):
    rows = d.query_text(f"SELECT source, vertex, walks FROM gg_khop_pair_counts({graph}, {sources_sql}, {targets_sql}, {hops})")
    return sorted(tuple(int(x) for x in r) for r in rows)


def reference_rows(d, hops, sources, targets=None):
    return sorted(tuple(int(x) for x in r) for r in d.query_text(P.sql_pair_counts(hops, sources, targets)))


@pytest.mark.parametrize("hops", [1, 2, 3])
def test_equals_the_reference_hash_aggregate_plan(db, hops):
    d, g, six, seventy, targets = db
    # six sources, listed with a duplicate and a NULL: the distinct non-NULL values count once each
    want = reference_rows(d, hops, six)
    rows = P.pair_counts(g, hops, six)["rows"][hops]  # the restatement agrees with the reference's plan
    assert len(want) > 0 and want == sorted((six[i], v, w) for i, v, w in zip(rows[0].tolist(), rows[1].tolist(), rows[2]))
    assert function_rows(d, values(six[:3] + [None, six[0]] + six[3:]), "NULL", hops) == want
    want_t = reference_rows(d, hops, six, targets)
    assert 0 < len(want_t) < len(want)
    assert function_rows(d, values(six), values(targets + [targets[0], None]), hops) == want_t
    # seventy sources: two batches
    assert function_rows(d, values(seventy), "''", hops) == reference_rows(d, hops, seventy)
    assert function_rows(d, values(seventy), values(targets), hops) == reference_rows(d, hops, seventy, targets)
    # every vertex
    want_all = reference_rows(d, hops, None)
    assert len(want_all) > len(want)
    for every in ("NULL", "''"):
        assert function_rows(d, every, every, hops) == want_all
    assert function_rows(d, "NULL", values(targets), hops) == reference_rows(d, hops, None, targets)


def test_empty_relations(db):
    d, g, six, seventy, targets = db
    nobody = "'SELECT p_personid FROM person WHERE p_personid IS NULL'"
    assert function_rows(d, nobody, "NULL", 2) == []  # an empty source relation is no source, not every vertex
    assert function_rows(d, values(six), nobody, 2) == []  # an empty target relation ends no row
    assert function_rows(d, values([-5, -6]), "NULL", 2) == []  # sources that are no vertices


def test_over_a_pinned_graph_twice(db):
    d, g, six, seventy, targets = db
    want = reference_rows(d, 2, seventy, targets)
    d.execute("PRAGMA gg_use_pinned_graphs")
    try:
        d.execute(f"SELECT * FROM gg_graph_pin({GRAPH})")
        for _ in range(2):
            assert function_rows(d, values(seventy), values(targets), 2) == want
        assert int(d.execute("SELECT * FROM gg_graph_pins()")[0, 0]) == 1
    finally:
        d.execute("SELECT * FROM gg_graph_unpin()")
        d.execute("PRAGMA gg_ignore_pinned_graphs")


def test_bad_arguments_raise_and_the_connection_stays_usable(db):
    d, g, six, seventy, targets = db
    s = values(six)
    bad = [
        f"'person', 'p_personid', 'knows', 'no_such_column', 'k_person2id', {s}, NULL, 2",  # a missing column
        f"{GRAPH}, 'SELECT no_such_column FROM person', NULL, 2",
        f"{GRAPH}, {s}, NULL, 0",  # hops outside 1..GG_MAX_HOPS
        f"{GRAPH}, {s}, NULL, 9",
        f"{GRAPH}, {s}, NULL, NULL",
    ]
    for args in bad:
        with pytest.raises(RuntimeError):
            d.execute(f"SELECT count(*) FROM gg_khop_pair_counts({args})")
    assert function_rows(d, s, "NULL", 1) == reference_rows(d, 1, six)
