"""The edge-filter restatement (tests/edge_filter_ref.py) pinned against trace(A^k), against the triangle enumerator, against
its own modes and, where the compiled reference is present, against the reference's plans of the closed-walk, NOT EXISTS
and EXISTS statements.  One test needs the built library but no GPU: the C-ABI exports the entry point."""
import ctypes as C

import numpy as np
import pytest

from oracle import ref_duckdb as R
from tests import edge_filter_ref as F
from tests import triangles_ref as T
from tests.oracle_lib import sort_rows


@pytest.fixture(scope="module")
def hard():
    vid, src, dst = T.hard_graph(V=300, rows=3000, seed=0x51, hub_fan=120)
    return vid, src, dst, T.TriangleGraph(vid, src, dst)


def sources_of(g):
    """the hub, dense index 3, the hub again, the self-loop vertices — as ids"""
    hub = int(np.bincount(g.dv, minlength=g.V).argmax())
    loops = np.nonzero(g.A.diagonal())[0].tolist()
    return g.vid[[hub, 3, hub] + loops]


@pytest.mark.parametrize("k", [2, 3, 4])
def test_closed_walks_of_all_sources_count_trace_of_the_power(hard, k):
    vid, src, dst, g = hard
    a = g.A.astype(np.float64)
    want = float(np.trace(np.linalg.matrix_power(a, k)))
    assert want < 2.0 ** 53  # float64 products of integers are exact below that
    rows, st = F.filter_graph(g, g.vid[F.walks(g, None, k - 1)], k - 1, 0, "inner")
    assert rows.shape[0] == st["rows_out"] == st["matches"] == int(round(want)) > 0
    if k == 3:
        assert np.array_equal(sort_rows(rows), sort_rows(g.id_rows(g.rows(0)[0])))


def test_walks_are_the_chained_expansion(hard):
    vid, src, dst, g = hard
    w = F.walks(g, None, 2)
    deg = np.diff(g.off)
    assert w.shape == (int(deg[g.dv].sum()), 3)
    assert (g.A[w[:, 0], w[:, 1]] > 0).all() and (g.A[w[:, 1], w[:, 2]] > 0).all()
    s = sources_of(g)
    twice = F.walks(g, np.concatenate([s, [-123456789]]), 2)
    assert twice.shape[0] == sum(F.walks(g, [x], 2).shape[0] for x in s.tolist()) > 0
    assert F.walks(g, [], 3).shape == (0, 4)


@pytest.mark.parametrize("case", [(2, 2, 0), (2, 0, 2), (2, 1, 2), (2, 1, 1), (3, 3, 0), (3, 1, 3)])
def test_semi_and_anti_partition_the_input_and_semi_collapses_inner(hard, case):
    vid, src, dst, g = hard
    hops, fc, tc = case
    rows = g.vid[F.walks(g, sources_of(g), hops)]
    inner, si = F.filter_graph(g, rows, fc, tc, "inner")
    semi, ss = F.filter_graph(g, rows, fc, tc, "semi")
    anti, sa = F.filter_graph(g, rows, fc, tc, "anti")
    assert ss["rows_out"] + sa["rows_out"] == rows.shape[0] == si["rows_in"]
    assert si["matches"] == ss["matches"] == sa["matches"] == inner.shape[0]
    m = F.multiplicity(rows, g.A, g.index, fc, tc)
    # semi and anti partition the input, in order
    assert np.array_equal(semi, rows[m > 0]) and np.array_equal(anti, rows[m == 0])
    # semi = inner with the consecutive copies of an input row collapsed
    first = np.concatenate([[0], np.cumsum(m[m > 0])[:-1]]).astype(np.int64) if inner.shape[0] else np.empty(0, np.int64)
    assert np.array_equal(inner[first], semi)
    if case == (2, 1, 2):
        assert anti.shape[0] == 0  # the second edge of a walk exists


def test_ids_unknown_to_the_condition_graph_survive_anti_only(hard):
    vid, src, dst, g = hard
    f = T.TriangleGraph(g.vid[::2], dst, src)  # half the vertices, the edge rows reversed
    rows = g.vid[F.walks(g, sources_of(g), 2)]
    known = np.isin(rows[:, 2], f.vid) & np.isin(rows[:, 0], f.vid)
    assert known.any() and not known.all()
    for mode in ("inner", "semi"):
        out, _ = F.filter_rows(rows, f.A, f.index, 2, 0, mode)
        assert out.shape[0] > 0 and np.isin(out[:, [0, 2]], f.vid).all()
    anti, _ = F.filter_rows(rows, f.A, f.index, 2, 0, "anti")
    unknown = rows[~known]
    assert np.array_equal(anti[~(np.isin(anti[:, 2], f.vid) & np.isin(anti[:, 0], f.vid))], unknown)
    empty, st = F.filter_rows(rows, np.zeros((0, 0), np.int64), {}, 2, 0, "anti")  # a condition graph of nothing
    assert np.array_equal(empty, rows) and st["matches"] == 0


def test_vectorised_digest_equals_the_oracle(hard, orc):
    vid, src, dst, g = hard
    for hops in (1, 2, 3):
        w = F.walks(g, sources_of(g), hops)[:3000]
        assert F.digest_dense_rows(w) == orc.digest_rows(w.astype(np.uint32))
    assert F.digest_dense_rows(np.empty((0, 3), np.int64)) == 0


def test_the_library_exports_the_entry_point_and_the_binding_has_the_methods():
    import duckdb_pgq_amd as pkg
    from duckdb_pgq_amd import gg as binding

    lib = C.CDLL(binding.LIB_PATH)
    assert hasattr(lib, "gg_result_filter_edge")
    assert "gg_result_filter_edge" in binding.SYMBOLS
    assert callable(getattr(pkg.GG, "filter_edge", None)) and callable(getattr(pkg.GG, "closed_walks", None))


@pytest.fixture(scope="module")
def ref(hard):
    vid, src, dst, g = hard
    d = R.RefDuckDB(threads=4)
    d.load_ldbc(vid, src, dst)
    yield d
    d.close()


needs_reference = pytest.mark.skipif(not R.available(), reason="reference build not present")


def distinct_sources(g):
    return np.unique(sources_of(g))  # an IN list does not multiply


@needs_reference
def test_against_the_reference_closed_walk_plan(hard, ref):
    vid, src, dst, g = hard
    s = distinct_sources(g)
    got = ref.execute(F.sql_closed_walks(4, s))
    want, _ = F.filter_graph(g, g.vid[F.walks(g, s, 3)], 3, 0, "inner")
    assert want.shape[0] > 0 and np.array_equal(sort_rows(got), sort_rows(want))


@needs_reference
@pytest.mark.parametrize("negate", [True, False])
def test_against_the_reference_exists_plans(hard, ref, negate):
    vid, src, dst, g = hard
    s = distinct_sources(g)
    got = ref.execute(F.sql_exists(2, 0, 2, negate, s))
    want, _ = F.filter_graph(g, g.vid[F.walks(g, s, 2)], 0, 2, "anti" if negate else "semi")
    assert want.shape[0] > 0 and np.array_equal(sort_rows(got), sort_rows(want))
