"""gg_cheapest_path inside the compiled reference, with the reference's own plan of the hop-bounded recursive CTE under
min(cost) (tests/cheapest_ref.sql_cheapest) over the same tables as the yardstick: no planner rule is on, so the recursion,
the joins and the aggregates run as the reference plans them.  Both sides are compared as sorted rows, and the restatement in
python integers agrees with both.  The fixpoint (max_hops NULL) is compared with the restatement alone: the unbounded CTE
need not terminate on a cyclic graph and is not run."""
import os

import numpy as np
import pytest

from oracle import ref_duckdb as R
from tests import cheapest_ref as CR
from tests import triangles_ref as T

EXT = R.EXTENSION

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not (R.available() and os.path.exists(EXT)), reason="reference build / extension not present"),
]

GRAPH = "'person', 'p_personid', 'knows', 'k_person1id', 'k_person2id', 'k_weight'"


@pytest.fixture(scope="module")
def db():
    vid, src, dst = T.hard_graph(V=300, rows=3000, seed=0x51, hub_fan=120)
    wt = CR.hashed_weights(src.size)
    g = CR.WeightedGraph(vid, src, dst, wt)
    d = R.RefDuckDB(threads=4)
    d.load_table("person", {"p_personid": vid})
    d.load_table("knows", {"k_person1id": src, "k_person2id": dst, "k_weight": wt})
    d.execute(f"LOAD '{EXT}'")
    tg = T.TriangleGraph(vid, src, dst)
    hub = int(np.bincount(tg.dv, minlength=tg.V).argmax())
    loop = int(np.nonzero(tg.A.diagonal())[0][0])
    six = [int(x) for x in g.vid[[hub, 3, loop, 17, 250]].tolist()] + [-123456789]  # the last one is no vertex
    assert len(set(six)) == 6
    seventy = [int(x) for x in g.vid[100:170].tolist()]  # two batches
    targets = [int(x) for x in g.vid[[3, 40, 7, 299, hub]].tolist()] + [-999]
    yield d, g, six, seventy, targets, (vid, src, dst)
    d.close()


def values(ids):
    """a relation of the ids as they stand, duplicates and NULLs included"""
    return "'SELECT x FROM (VALUES " + ", ".join("(NULL)" if s is None else f"({int(s)})" for s in ids) + ") t(x)'"


def function_rows(d, sources_sql, targets_sql, max_hops, graph=GRAPH):
    rows = d.query_text(
        f"SELECT source, vertex, cost, hops FROM gg_cheapest_path({graph}, {sources_sql}, {targets_sql}, {max_hops})")
    return sorted(tuple(int(x) for x in r) for r in rows)


def reference_rows(d, max_hops, sources, targets=None):
    return sorted(tuple(int(x) for x in r) for r in d.query_text(CR.sql_cheapest(max_hops, sources, targets)))


def restated(g, sources, max_hops, targets=None):
    sources = list(g.vid.tolist()) if sources is None else sources
    return CR.id_rows(CR.cheapest(g, sources, max_hops, targets)["rows"], sources)


@pytest.mark.parametrize("max_hops", [1, 2, 3])
def test_equals_the_reference_recursive_cte_plan(db, max_hops):
    d, g, six, seventy, targets, _ = db
    # six sources, listed with a duplicate and a NULL: the distinct non-NULL values count once each
    want = reference_rows(d, max_hops, six)
    assert len(want) > 5 and want == restated(g, six, max_hops)  # the restatement agrees with the reference's plan
    assert function_rows(d, values(six[:3] + [None, six[0]] + six[3:]), "NULL", max_hops) == want
    want_t = reference_rows(d, max_hops, six, targets)
    assert 0 < len(want_t) < len(want) and want_t == restated(g, six, max_hops, targets)
    assert function_rows(d, values(six), values(targets + [targets[0], None]), max_hops) == want_t
    # seventy sources: two batches
    want_70 = reference_rows(d, max_hops, seventy)
    assert want_70 == restated(g, seventy, max_hops)
    assert function_rows(d, values(seventy), "''", max_hops) == want_70
    assert function_rows(d, values(seventy), values(targets), max_hops) == reference_rows(d, max_hops, seventy, targets)


def test_every_vertex_at_two_hops(db):
    d, g, six, seventy, targets, _ = db
    want_all = reference_rows(d, 2, None)
    assert len(want_all) > 300 and want_all == restated(g, None, 2)
    for every in ("NULL", "''"):
        assert function_rows(d, every, every, 2) == want_all
    assert function_rows(d, "NULL", values(targets), 2) == reference_rows(d, 2, None, targets)


def test_the_fixpoint_equals_the_restatement(db):
    d, g, six, seventy, targets, _ = db
    want = restated(g, seventy, -1)
    assert len(want) > len(restated(g, seventy, 3))
    assert function_rows(d, values(seventy), "NULL", "NULL") == want
    assert function_rows(d, values(seventy), "NULL", -1) == want
    assert function_rows(d, values(seventy), "NULL", -7) == want
    assert function_rows(d, values(six), values(targets), "NULL") == restated(g, six, -1, targets)
    assert function_rows(d, values(six), "NULL", 0) == sorted((s, s, 0, 0) for s in six[:5])  # no edge: the sources alone


def test_empty_relations(db):
    d, g, six, seventy, targets, _ = db
    nobody = "'SELECT p_personid FROM person WHERE p_personid IS NULL'"
    assert function_rows(d, nobody, "NULL", 2) == []  # an empty source relation is no source, not every vertex
    assert function_rows(d, values(six), nobody, 2) == []  # an empty target relation reports no row
    assert function_rows(d, values([-5, -6]), "NULL", 2) == []  # sources that are no vertices


def test_over_a_pinned_graph_twice(db):
    d, g, six, seventy, targets, _ = db
    want = reference_rows(d, 2, seventy, targets)
    d.execute("PRAGMA gg_use_pinned_graphs")
    try:
        d.execute("SELECT * FROM gg_graph_pin('person', 'p_personid', 'knows', 'k_person1id', 'k_person2id')")
        for _ in range(2):
            assert function_rows(d, values(seventy), values(targets), 2) == want
        assert int(d.execute("SELECT * FROM gg_graph_pins()")[0, 0]) == 1
    finally:
        d.execute("SELECT * FROM gg_graph_unpin()")
        d.execute("PRAGMA gg_ignore_pinned_graphs")


def test_bad_weights_and_arguments_raise_and_the_connection_stays_usable(db):
    d, g, six, seventy, targets, _ = db
    s = values(six)
    d.execute("CREATE TABLE knows_null AS SELECT k_person1id, k_person2id, "
              "CASE WHEN k_weight = 17 THEN NULL ELSE k_weight END AS k_weight FROM knows")
    d.execute("CREATE TABLE knows_neg AS SELECT k_person1id, k_person2id, k_weight - 50 AS k_weight FROM knows")
    d.execute("CREATE TABLE knows_real AS SELECT k_person1id, k_person2id, CAST(k_weight AS DOUBLE) AS k_weight FROM knows")
    person = "'person', 'p_personid'"
    bad = [
        (f"{person}, 'knows_null', 'k_person1id', 'k_person2id', 'k_weight', {s}, NULL, 2", "k_weight"),
        (f"{person}, 'knows_neg', 'k_person1id', 'k_person2id', 'k_weight', {s}, NULL, 2", "k_weight"),
        (f"{person}, 'knows_real', 'k_person1id', 'k_person2id', 'k_weight', {s}, NULL, 2", "k_weight"),
        (f"{person}, 'knows', 'k_person1id', 'k_person2id', 'no_such_column', {s}, NULL, 2", None),
        (f"{person}, 'knows', 'no_such_column', 'k_person2id', 'k_weight', {s}, NULL, 2", None),
        (f"{person}, 'knows', 'k_person1id', 'k_person2id', NULL, {s}, NULL, 2", None),
        (f"{GRAPH}, 'SELECT no_such_column FROM person', NULL, 2", None),
    ]
    for args, named in bad:
        with pytest.raises(RuntimeError) as e:
            d.execute(f"SELECT count(*) FROM gg_cheapest_path({args})")
        if named:  # the message names the function and the column
            assert "gg_cheapest_path" in str(e.value) and named in str(e.value), str(e.value)
    assert function_rows(d, s, "NULL", 1) == reference_rows(d, 1, six)


def test_a_changed_weight_column_gives_the_new_answer(db):
    d, g, six, seventy, targets, (vid, src, dst) = db
    d.execute("CREATE TABLE knows_upd AS SELECT k_person1id, k_person2id, k_weight FROM knows")  # (this test's own copy)
    graph = "'person', 'p_personid', 'knows_upd', 'k_person1id', 'k_person2id', 'k_weight'"
    before = function_rows(d, values(six), "NULL", "NULL", graph)
    assert before == restated(g, six, -1)
    d.execute("UPDATE knows_upd SET k_weight = 1")
    unit = CR.WeightedGraph(vid, src, dst, np.ones(src.size, np.int64))
    after = function_rows(d, values(six), "NULL", "NULL", graph)
    assert after == restated(unit, six, -1) and after != before
    assert all(cost == hops for _, _, cost, hops in after)
    sql = CR.sql_cheapest(2, six).replace(" knows k", " knows_upd k")
    assert function_rows(d, values(six), "NULL", 2, graph) == sorted(tuple(int(x) for x in r) for r in d.query_text(sql))
