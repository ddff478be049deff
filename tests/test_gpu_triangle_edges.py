"""GG.triangles_edges (gg_triangles_edges) against the numpy restatement (tests/triangle_edges_ref.py): the six columns
(a, b, c, e1, e2, e3) for both orders, with staged rowids and with append positions, on every route the kernel has
(LDS-staged and global in-rows, split launches), on the multi-pass build and on a fully mirrored table; the id columns
position for position against GG.triangles; source lists, degenerate graphs, errors and the lazy position array.

The mirrored table cannot bring the derived reverse CSR into play here: the build derives it only in its rowid-free form
(gg_csr_fast.hip), and gg_triangles_edges refuses a CSR without rowids.  The route still runs the paired build of such a
table.  The 2^32-row refusal cannot be reached at test size; it is the same line as gg_triangles'."""
import ctypes as C

import numpy as np
import pytest

from duckdb_pgq_amd import GGError
from duckdb_pgq_amd.gg import TriStats
from tests import triangle_edges_ref as E
from tests.oracle_lib import sort_rows

pytestmark = pytest.mark.gpu

GG_ERR_INVALID_ARG, GG_ERR_STATE = -1, -6


@pytest.fixture(scope="module")
def hard():
    """the builder's graph, its mirrored copy, and a cache of what the restatement says per (table, rowids, order)"""
    vid, src, dst = E.graph()
    tables = {"plain": (src, dst), "mirrored": (np.concatenate([src, dst]), np.concatenate([dst, src]))}
    cache = {}

    def want(table, explicit, order):
        key = (table, explicit, order)
        if key not in cache:
            s, d = tables[table]
            cache[key] = sort_rows(E.rows(vid, s, d, E.explicit_rowids(s.size) if explicit else None, order))
        return cache[key]

    return vid, tables, want


def build(gg, vid, src, dst, rowid=None):
    gg.staging_clear()
    gg.append_vertices(np.asarray(vid, np.int64))
    gg.append_edges(np.asarray(src, np.int64), np.asarray(dst, np.int64), rowid)
    return gg.build_csr()


def fetch_ids(res):
    parts = [res.fetch(2, o) for o in range(0, res.rows(2), 1024)]
    return np.concatenate(parts, axis=0) if parts else np.empty((0, 3), np.int64)


def fetch_edges(res):
    parts = [res.fetch_triangle_edges(o) for o in range(0, res.rows(2), 1024)]
    return np.concatenate(parts, axis=0) if parts else np.empty((0, 3), np.int64)


def six_columns(gg, csr, sources, order):
    st, res = gg.triangles_edges(csr, sources, ordered=bool(order))
    try:
        assert res.rows(2) == st["rows"]
        return st, np.concatenate([fetch_ids(res), fetch_edges(res)], axis=1)
    finally:
        res.close()


def check(gg, csr, want_sorted, order, sources=None, rowid=None):
    """every check the routes share; returns the six columns as the device ordered them"""
    st_ids = gg.triangles(csr, sources, ordered=bool(order))
    st_mat, res_ids = gg.triangles(csr, sources, ordered=bool(order), materialise=True)
    try:
        ids_only = fetch_ids(res_ids)
    finally:
        res_ids.close()
    st, res = gg.triangles_edges(csr, sources, ordered=bool(order))
    try:
        n = res.rows(2)
        print("order", order, "edges", st, "ids only", st_ids, "restatement rows", want_sorted.shape[0])
        assert st == st_ids == st_mat and n == st["rows"] == want_sorted.shape[0]
        ids, edges = fetch_ids(res), fetch_edges(res)
        assert np.array_equal(sort_rows(np.concatenate([ids, edges], axis=1)), want_sorted)
        assert np.array_equal(ids, ids_only)  # the same rows at the same positions, unsorted
        assert res.digest(csr, 2) == (st["rows"], st["digest"])
        walk = [res.fetch_edges(2, o) for o in range(0, n, 1024)]  # gg_result_fetch_edges: the 2-hop walk's e1, e2
        assert np.array_equal(np.concatenate(walk, axis=0) if walk else np.empty((0, 2), np.int64), edges[:, :2])
        # uneven slices: offsets that are no multiple of 1024, one crossing the end, one past it
        for off, take in ((1000, 777), (n - 5, 100), (n + 3, 10), (max(n // 2, 1) + 1, 1024)):
            if off < 0:
                continue
            got = res.fetch_triangle_edges(off, take)
            assert np.array_equal(got, edges[off:off + take]) and got.shape[0] == max(0, min(take, n - off))
    finally:
        res.close()
    st2, again = six_columns(gg, csr, sources, order)
    assert st2 == st and again.tobytes() == np.concatenate([ids, edges], axis=1).tobytes()  # identical on every run
    # the rows of one wedge (e1, e2) are consecutive and their e3 ascends in append order
    if n:
        p3 = E.positions_of(edges[:, 2], rowid)
        same = (edges[1:, 0] == edges[:-1, 0]) & (edges[1:, 1] == edges[:-1, 1])
        if sources is None:  # (a source listed twice repeats its wedges)
            assert 1 + int((~same).sum()) == np.unique(edges[:, :2], axis=0).shape[0]
        assert np.all(p3[1:][same] > p3[:-1][same])
    return np.concatenate([ids, edges], axis=1)


ROUTES = ["default", "tile4", "tile64", "grid1", "grid3", "legacy_build", "mirrored"]


@pytest.mark.parametrize("explicit", [False, True], ids=["positions", "rowids"])
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("route", ROUTES)
def test_every_route_equals_the_restatement(gg, hard, route, order, explicit):
    vid, tables, want = hard
    table = "mirrored" if route == "mirrored" else "plain"
    src, dst = tables[table]
    rowid = E.explicit_rowids(src.size) if explicit else None
    if route == "legacy_build":
        gg.force_legacy_build(True)
    csr = build(gg, vid, src, dst, rowid)
    if route in ("tile4", "tile64"):  # in-rows above 4 (64) entries, the hub's included, are searched in global memory
        gg.debug_triangle_tile(4 if route == "tile4" else 64)
    if route in ("grid1", "grid3"):
        gg.max_grid_tiles(1 if route == "grid1" else 3)
    try:
        rows = check(gg, csr, want(table, explicit, order), order, rowid=rowid)
        if route == "default" and order == 0:
            assert np.any(np.unique(rows[:, 3:5], axis=0, return_counts=True)[1] > 1)  # wedges with parallel closing rows
    finally:
        csr.close()


@pytest.mark.parametrize("order", [0, 1])
def test_source_lists(gg, hard, order):
    vid, tables, want = hard
    src, dst = tables["plain"]
    rowid = E.explicit_rowids(src.size)
    kept = np.isin(src, vid) & np.isin(dst, vid)
    ids, outdeg = np.unique(src[kept], return_counts=True)
    hub = int(ids[outdeg.argmax()])
    assert outdeg.max() > 512  # far more wedges than a tile holds: tiles begin in the middle of an entry
    csr = build(gg, vid, src, dst, rowid)
    try:
        for sources in ([hub], [hub, -123456789, int(vid[0]), hub, int(vid[1]), int(vid[0])], []):
            s = np.asarray(sources, np.int64)
            check(gg, csr, sort_rows(E.rows(vid, src, dst, rowid, order, s)), order, s, rowid)
    finally:
        csr.close()


def test_degenerate_graphs(gg):
    vid = np.array([10, -20, 30], np.int64)  # dense order is not id order, one id negative
    cases = [
        ([], [], 0, 0),                              # no edges
        ([10], [10], 1, 0),                          # one self-loop
        ([10, 10], [10, 10], 8, 0),                  # two parallel self-loops: every triple of the two rows
        ([10, 77, 78], [99, 10, 79], 0, 0),          # only dangling rows
        ([10, 5, 30, -20], [30, 5, -20, 10], 3, 1),  # 10 -> 30 -> -20 -> 10: the ordered row is (-20, 10, 30)
    ]
    for src, dst, n0, n1 in cases:
        src, dst = np.array(src, np.int64), np.array(dst, np.int64)
        for rowid in (None, E.explicit_rowids(src.size)):
            csr = build(gg, vid, src, dst, rowid)
            try:
                for order, n in ((0, n0), (1, n1)):
                    rows = check(gg, csr, sort_rows(E.rows(vid, src, dst, rowid, order)), order, rowid=rowid)
                    assert rows.shape[0] == n
                    none = check(gg, csr, np.empty((0, 6), np.int64), order, np.empty(0, np.int64), rowid)  # n_src = 0
                    assert none.shape == (0, 6)
            finally:
                csr.close()


def test_errors_leave_the_context_usable(gg, hard):
    vid, tables, want = hard
    src, dst = tables["plain"]
    i64p = C.POINTER(C.c_int64)
    bufs = [np.empty(1024, np.int64) for _ in range(3)]
    ptrs = (i64p * 3)(*[b.ctypes.data_as(i64p) for b in bufs])

    def good(csr):
        st, rows = six_columns(gg, csr, None, 1)
        assert np.array_equal(sort_rows(rows), want("plain", False, 1))

    gg.set_edge_rowid(False)
    bare = build(gg, vid, src, dst)
    gg.set_edge_rowid(True)
    gg.staging_clear()
    gg.append_vertices(vid)
    gg.append_edges(src, dst)
    shard = gg.build_csr_shard(0, 2)
    csr = gg.build_csr()
    try:
        for bad in (bare, shard):
            with pytest.raises(GGError) as e:
                gg.triangles_edges(bad)
            assert e.value.code == GG_ERR_STATE
            good(csr)
        st, res = TriStats(), C.c_void_p()
        assert gg.lib.gg_triangles_edges(gg.ctx, csr.handle, None, 0, 2, C.byref(st), C.byref(res)) == GG_ERR_INVALID_ARG
        assert not res.value
        good(csr)
        _, ids_only = gg.triangles(csr, ordered=True, materialise=True)
        try:
            n = C.c_uint32()
            assert gg.lib.gg_triangles_fetch_edges(ids_only.handle, 0, 1024, ptrs, C.byref(n)) == GG_ERR_STATE
            with pytest.raises(GGError) as e:
                ids_only.fetch_triangle_edges(0)
            assert e.value.code == GG_ERR_STATE
        finally:
            ids_only.close()
        good(csr)
        _, res = gg.triangles_edges(csr, ordered=True)
        try:
            n = C.c_uint32()
            assert gg.lib.gg_triangles_fetch_edges(res.handle, 0, 1024, None, C.byref(n)) == GG_ERR_INVALID_ARG
            assert gg.lib.gg_triangles_fetch_edges(res.handle, 0, 1024, ptrs, None) == GG_ERR_INVALID_ARG
        finally:
            res.close()
        good(csr)
    finally:
        bare.close()
        shard.close()
        csr.close()


def test_the_position_array_is_built_late_and_once(gg, hard):
    """gg_triangles and gg_bfs64_paths build rnbr_by_src and never the position array; the first gg_triangles_edges
    call on the CSR builds it, with rnbr_by_src already there, and later calls do not build it again."""
    vid, tables, want = hard
    src, dst = tables["plain"]
    csr = build(gg, vid, src, dst)
    try:
        gg.profile(True)
        gg.profile_reset()
        gg.triangles(csr)
        _, res = gg.triangles(csr, ordered=True, materialise=True)
        res.close()
        gg.bfs64_paths(csr, vid[:4], np.arange(4, dtype=np.uint32), vid[10:14], 4)
        assert "tri_entry_positions" not in gg.profile_get() and "k_tri_write_edges" not in gg.profile_get()
        for order in (0, 1):
            st, rows = six_columns(gg, csr, None, order)
            assert np.array_equal(sort_rows(rows), want("plain", False, order))
        prof = gg.profile_get()
        assert prof["tri_entry_positions"][0] == 1 and prof["k_tri_write_edges"][0] == 2
    finally:
        csr.close()
