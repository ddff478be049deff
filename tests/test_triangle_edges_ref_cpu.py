"""The restatement of triangle rows with edge rowids (tests/triangle_edges_ref.py) pinned against the edge table itself,
against tests/triangles_ref.py and trace(A^3) and, where the compiled reference is present, against its own three-join
plan selecting the three rowids; and the two C-ABI calls of the feature, as far as they go without a device."""
import ctypes
import os
import re

import numpy as np
import pytest

import duckdb_pgq_amd.gg as ggmod
from oracle import ref_duckdb as R
from tests import triangle_edges_ref as E
from tests import triangles_ref as T
from tests.oracle_lib import sort_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GG_ERR_INVALID_ARG = -1
NEW_SYMBOLS = ["gg_triangles_edges", "gg_triangles_fetch_edges"]


@pytest.fixture(scope="module", params=["hard", "tiny"])
def table(request):
    vid, src, dst = E.graph() if request.param == "hard" else E.tiny_graph()
    return vid, src, dst, T.TriangleGraph(vid, src, dst)


@pytest.mark.parametrize("explicit", [False, True])
@pytest.mark.parametrize("order", [0, 1])
def test_rows_are_distinct_closing_triples_of_edge_rows(table, order, explicit):
    vid, src, dst, g = table
    rowid = E.explicit_rowids(src.size) if explicit else None
    rows = E.rows(vid, src, dst, rowid, order)
    assert rows.shape[0] > 0
    assert np.unique(rows[:, 3:], axis=0).shape[0] == rows.shape[0]  # pairwise distinct as (e1, e2, e3)
    p = E.positions_of(rows[:, 3:], rowid)
    a, b, c = rows[:, 0], rows[:, 1], rows[:, 2]
    for col, (u, v) in enumerate(((a, b), (b, c), (c, a))):
        assert np.array_equal(src[p[:, col]], u) and np.array_equal(dst[p[:, col]], v)
    want, _ = g.rows(order)
    assert np.array_equal(sort_rows(rows[:, :3]), sort_rows(g.id_rows(want)))
    if order == 0:
        assert rows.shape[0] == g.trace_cube()
    else:
        assert np.all((a < b) & (b < c))


def test_the_hand_written_graph_row_by_row():
    vid, src, dst = E.tiny_graph()
    rows = E.rows(vid, src, dst)
    loops = rows[(rows[:, :3] == 4).all(axis=1)][:, 3:]
    assert sorted(map(tuple, loops.tolist())) == [(x, y, z) for x in (5, 6) for y in (5, 6) for z in (5, 6)]
    cyc = rows[(rows[:, 0] == 1) & (rows[:, 1] == 2)]
    assert sorted(map(tuple, cyc.tolist())) == [(1, 2, 3, 1, 2, 3), (1, 2, 3, 1, 4, 3)]  # the doubled edge 2 -> 3
    assert sorted(map(tuple, rows[rows[:, 0] >= 5].tolist())) == [(5, 5, 5, 9, 9, 9), (5, 5, 6, 9, 7, 8), (5, 6, 5, 7, 8, 9),
                                                                  (6, 5, 5, 8, 9, 7)]
    assert not np.any(rows[:, 3:] == 0)  # the dangling row, first, is in no triangle and still counts as a position
    assert rows.shape[0] == 6 + 8 + 4


def test_sources_with_multiplicity_and_non_vertices():
    vid, src, dst = E.tiny_graph()
    once = E.rows(vid, src, dst, sources=[4])
    assert once.shape[0] == 8
    got = E.rows(vid, src, dst, sources=[4, -123, 1, 4])
    want = np.concatenate([once, once, E.rows(vid, src, dst, sources=[1])])
    assert np.array_equal(sort_rows(got), sort_rows(want))
    assert E.rows(vid, src, dst, sources=[]).shape == (0, 6)


def test_the_builder_separates_position_kept_index_and_csr_position():
    vid, src, dst = E.graph()
    kept = np.flatnonzero(np.isin(src, vid) & np.isin(dst, vid))
    g = T.TriangleGraph(vid, src, dst)
    assert src.size - kept.size >= 50 and np.any(kept[:1000] != np.arange(1000))  # dangling rows among the first thousand
    csr_order = np.argsort(g.su, kind="stable")
    assert np.any(csr_order != np.arange(kept.size))
    r = E.explicit_rowids(src.size)
    assert np.unique(r).size == r.size and np.all(np.diff(r) < 0)


@pytest.mark.skipif(not R.available(), reason="reference build not present")
@pytest.mark.parametrize("ordered", [False, True])
def test_against_the_reference_three_join_plan(table, ordered):
    vid, src, dst, g = table
    d = R.RefDuckDB(threads=4)
    try:
        d.load_ldbc(vid, src, dst)
        got = d.execute(T.sql_triangles(T.SQL_ROWS + ", k1.rowid, k2.rowid, k3.rowid", ordered))
    finally:
        d.close()
    assert np.array_equal(sort_rows(np.asarray(got, np.int64)), sort_rows(E.rows(vid, src, dst, None, int(ordered))))


# ---- the C-ABI of the feature, without a device ---------------------------------------------------------------------
def test_library_exports_and_header_declares_the_two_calls():
    lib = ctypes.CDLL(ggmod.LIB_PATH)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gg.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in ggmod.SYMBOLS


def test_fetch_edges_refuses_null_arguments_without_a_device():
    lib = ggmod.load_library()
    n = ctypes.c_uint32(7)
    bufs = [np.empty(4, np.int64) for _ in range(3)]
    i64p = ctypes.POINTER(ctypes.c_int64)
    ptrs = (i64p * 3)(*[b.ctypes.data_as(i64p) for b in bufs])
    assert lib.gg_triangles_fetch_edges(None, 0, 4, ptrs, ctypes.byref(n)) == GG_ERR_INVALID_ARG
