"""The triangle restatement (tests/triangles_ref.py) pinned against trace(A^3), against the 6x / 1x relation of a
mirrored simple graph and, where the compiled reference is present, against its own three-join plan."""
import numpy as np
import pytest

from duckdb_pgq_amd import datagen
from oracle import ref_duckdb as R
from tests import triangles_ref as T
from tests.oracle_lib import sort_rows


@pytest.fixture(scope="module")
def hard():
    vid, src, dst = T.hard_graph(V=300, rows=3000, seed=0x51, hub_fan=120)
    return vid, src, dst, T.TriangleGraph(vid, src, dst)


def test_enumerator_equals_trace_of_the_cube(hard):
    vid, src, dst, g = hard
    rows, wedges = g.rows(0)
    assert rows.shape[0] == g.trace_cube() > 0
    deg = np.diff(g.off)
    assert wedges == int(deg[g.dv].sum())  # every 2-hop walk is looked at
    # every row is three edge rows, and its multiplicity is the product of theirs
    uniq, cnt = np.unique(rows, axis=0, return_counts=True)
    assert np.array_equal(cnt, g.A[uniq[:, 0], uniq[:, 1]] * g.A[uniq[:, 1], uniq[:, 2]] * g.A[uniq[:, 2], uniq[:, 0]])


def test_ordered_rows_are_the_ascending_ones(hard):
    vid, src, dst, g = hard
    all_rows, _ = g.rows(0)
    ids = g.id_rows(all_rows)
    want = ids[(ids[:, 0] < ids[:, 1]) & (ids[:, 1] < ids[:, 2])]
    got, wedges = g.rows(1)
    assert np.array_equal(sort_rows(g.id_rows(got)), sort_rows(want)) and want.shape[0] > 0
    assert got.shape[0] <= wedges < g.rows(0)[1]


def test_walk_semantics_of_loops_and_parallel_rows():
    vid = np.array([10, 20, 30], np.int64)
    g = T.TriangleGraph(vid, [10], [10])  # a self-loop: the one row (a, a, a)
    assert g.rows(0)[0].tolist() == [[0, 0, 0]] and g.rows(1)[0].shape[0] == 0
    g = T.TriangleGraph(vid, [10, 10, 20], [10, 20, 10])  # a 2-cycle with a self-loop
    assert sorted(g.id_rows(g.rows(0)[0]).tolist()) == [[10, 10, 10], [10, 10, 20], [10, 20, 10], [20, 10, 10]]
    g = T.TriangleGraph(vid, [10, 20, 30, 10], [20, 30, 10, 20])  # a 3-cycle, one edge twice: rotations x 2
    assert g.rows(0)[0].shape[0] == 6 and g.rows(1)[0].shape[0] == 2
    g = T.TriangleGraph(vid, [30, 20, 10], [20, 10, 30])  # descending along the cycle: no ordered row
    assert g.rows(0)[0].shape[0] == 3 and g.rows(1)[0].shape[0] == 0


def test_mirrored_simple_graph_six_and_one():
    vid, src, dst = datagen.ldbc_knows(400, 6000, 9)
    g = T.TriangleGraph(vid, src, dst)
    assert g.A.max() == 1 and np.array_equal(g.A, g.A.T) and not g.A.diagonal().any()
    n0, n1 = g.rows(0)[0].shape[0], g.rows(1)[0].shape[0]
    assert n0 == 6 * n1 > 0


def test_source_lists(hard):
    vid, src, dst, g = hard
    rows, _ = g.rows(0)
    a = int(rows[0, 0])
    one, _ = g.rows(0, [vid[a]])
    assert np.array_equal(sort_rows(one), sort_rows(rows[rows[:, 0] == a]))
    twice, _ = g.rows(0, [vid[a], -123456, vid[a]])
    assert twice.shape[0] == 2 * one.shape[0]
    assert g.rows(0, [])[0].shape[0] == 0


@pytest.mark.skipif(not R.available(), reason="reference build not present")
@pytest.mark.parametrize("ordered", [False, True])
def test_against_the_reference_three_join_plan(hard, ordered):
    vid, src, dst, g = hard
    d = R.RefDuckDB(threads=4)
    try:
        d.load_ldbc(vid, src, dst)
        got = d.execute(T.sql_triangles(T.SQL_ROWS, ordered))
        assert int(d.execute(T.sql_triangles("count(*)", ordered))[0, 0]) == got.shape[0]
    finally:
        d.close()
    want = g.id_rows(g.rows(1 if ordered else 0)[0])
    assert np.array_equal(sort_rows(got), sort_rows(want))
