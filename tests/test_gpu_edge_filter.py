"""GG.filter_edge / GG.closed_walks (gg_result_filter_edge) against the numpy restatement (tests/edge_filter_ref.py): stats,
row count, digest and — for outputs under 200 000 rows — the rows themselves in the input's order, for every mode, on split
launches and every build form, with a second condition graph, chained, on degenerate shapes and through every error.  The
cross-check of two independent kernels: the 2-hop table of all sources closed 2 -> 0 is gg_triangles' result.  The 2^32-row
refusal of the materialising form cannot be reached at test size; it was checked by reading csrc/gg_filter.hip only."""
import ctypes as C

import numpy as np
import pytest

from duckdb_pgq_amd import GGError
from duckdb_pgq_amd.gg import EdgeFilterStats
from tests import edge_filter_ref as F
from tests import triangles_ref as T
from tests.oracle_lib import sort_rows

pytestmark = pytest.mark.gpu

GG_ERR_INVALID_ARG, GG_ERR_STATE = -1, -6
FETCH_BELOW = 200_000  # outputs of fewer rows are fetched and compared in order; larger ones by count and digest
PIECE = 65_536
CASES = [(2, 2, 0), (2, 0, 2), (2, 1, 2), (2, 1, 1), (3, 3, 0), (3, 1, 3)]


@pytest.fixture(scope="module")
def hard():
    """the graph, the source list S = [hub, dense index 3, hub again, the self-loop vertices] and the dense walk tables
    of S the restatement forms (computed once, never changed)"""
    vid, src, dst = T.hard_graph()
    g = T.TriangleGraph(vid, src, dst)
    indeg = np.bincount(g.dv, minlength=g.V)
    assert indeg.max() > 500  # the hub's in-row is the long one
    loops = np.nonzero(g.A.diagonal())[0].tolist()
    assert len(loops) == 2
    S = g.vid[[int(indeg.argmax()), 3, int(indeg.argmax())] + loops]
    walks = {h: F.walks(g, S, h) for h in (1, 2, 3)}
    for w in walks.values():
        w.setflags(write=False)
    # the cases are not trivial: closing the 2-hop walks puts rows out in every mode, and some row repeats
    m = F.multiplicity(g.vid[walks[2]], g.A, g.index, 2, 0)
    assert m.max() >= 2 and 0 < int((m > 0).sum()) < m.size
    return vid, src, dst, g, S, walks


def build(gg, vid, src, dst):
    gg.staging_clear()
    gg.append_vertices(np.asarray(vid, np.int64))
    gg.append_edges(np.asarray(src, np.int64), np.asarray(dst, np.int64))
    return gg.build_csr()


def fetch_all(res, hops):
    """every row of table `hops`, in pieces of up to PIECE rows"""
    n = res.rows(hops)
    out = np.empty((hops + 1, max(n, 1)), np.int64)
    i64p = C.POINTER(C.c_int64)
    for o in range(0, n, PIECE):
        ptrs = (i64p * (hops + 1))(*[out[c, o:].ctypes.data_as(i64p) for c in range(hops + 1)])
        got = C.c_uint32()
        res.gg._chk(res.gg.lib.gg_result_fetch(res.handle, hops, o, min(PIECE, n - o), ptrs, C.byref(got)))
        assert got.value == min(PIECE, n - o)
    return out[:, :n].T.copy()


def digest_of(orc, dense_rows):
    """orc.digest_rows where python can afford it, its vectorised twin (pinned to it on the CPU) above that"""
    if dense_rows.shape[0] < FETCH_BELOW:
        d = orc.digest_rows(dense_rows.astype(np.uint32))
        assert d == F.digest_dense_rows(dense_rows)
        return d
    return F.digest_dense_rows(dense_rows)


def check(gg, orc, csr, g, walks_res, dense_walks, hops, fc, tc, mode, cond=None, cond_csr=None):
    """one call against the restatement; cond: the condition TriangleGraph (default g).  Returns (stats, largest m)."""
    cond, cond_csr = cond or g, cond_csr or csr
    want_rows, want = F.filter_rows(g.vid[dense_walks], cond.A, cond.index, fc, tc, mode)
    count_only = gg.filter_edge(walks_res, hops, cond_csr, fc, tc, mode, materialise=False)
    st, res = gg.filter_edge(walks_res, hops, cond_csr, fc, tc, mode)
    print((hops, fc, tc), mode, "device", st, "restatement", want)
    try:
        assert st == want and count_only == st
        assert res.rows(hops) == st["rows_out"]
        want_dense = F.dense_of(g.index, want_rows.reshape(-1)).reshape(want_rows.shape)
        assert res.digest(csr, hops) == (st["rows_out"], digest_of(orc, want_dense))
        if st["rows_out"] < FETCH_BELOW:  # in order and unsorted: the restatement applied to the input as it stands
            table = fetch_all(walks_res, hops)
            assert table.shape == dense_walks.shape
            assert np.array_equal(fetch_all(res, hops), F.filter_rows(table, cond.A, cond.index, fc, tc, mode)[0])
    finally:
        res.close()
    m = F.multiplicity(g.vid[dense_walks], cond.A, cond.index, fc, tc)
    return st, int(m.max()) if m.size else 0


@pytest.mark.parametrize("case", CASES)
def test_every_mode_and_column_pair_equals_the_restatement(gg, orc, hard, case):
    vid, src, dst, g, S, walks = hard
    hops, fc, tc = case
    csr = build(gg, vid, src, dst)
    table = gg.expand_khop_result(csr, hops, S)
    try:
        for mode in F.MODES:
            check(gg, orc, csr, g, table, walks[hops], hops, fc, tc, mode)
    finally:
        table.close()
        csr.close()


def test_two_hop_table_of_all_sources_closed_is_gg_triangles(gg, hard):
    vid, src, dst, g, S, walks = hard
    csr = build(gg, vid, src, dst)
    table = gg.expand_khop_result(csr, 2)
    try:
        st, res = gg.filter_edge(table, 2, csr, 2, 0, "inner")
        tst, tri = gg.triangles(csr, materialise=True)
        try:
            assert st["rows_out"] == st["matches"] == tst["rows"] == res.rows(2) == tri.rows(2) > 0
            assert st["rows_in"] == tst["wedges"] == table.rows(2)
            assert res.digest(csr, 2) == tri.digest(csr, 2) == (tst["rows"], tst["digest"])
            assert np.array_equal(sort_rows(fetch_all(res, 2)), sort_rows(fetch_all(tri, 2)))
        finally:
            res.close()
            tri.close()
    finally:
        table.close()
        csr.close()


@pytest.mark.parametrize("route", ["default", "grid3", "legacy_build", "no_rowid"])
def test_every_route_equals_the_restatement(gg, orc, hard, route):
    vid, src, dst, g, S, walks = hard
    if route == "legacy_build":
        gg.force_legacy_build(True)
    if route == "no_rowid":
        gg.set_edge_rowid(False)
    csr = build(gg, vid, src, dst)
    tables = {h: gg.expand_khop_result(csr, h, S) for h in (2, 3)}
    if route == "grid3":
        gg.max_grid_tiles(3)  # three workgroups, 768 rows, a launch
    try:
        check(gg, orc, csr, g, tables[3], walks[3], 3, 3, 0, "inner")
        check(gg, orc, csr, g, tables[2], walks[2], 2, 0, 2, "anti")
    finally:
        for t in tables.values():
            t.close()
        csr.close()


def test_a_second_condition_graph_whose_vertex_table_lacks_ids(gg, orc, hard):
    vid, src, dst, g, S, walks = hard
    csr = build(gg, vid, src, dst)
    table = gg.expand_khop_result(csr, 2, S)
    cond = T.TriangleGraph(g.vid[::2], dst, src)  # half the vertices, the edge rows reversed
    cond_csr = build(gg, cond.vid, dst, src)
    try:
        rows = g.vid[walks[2]]
        known = np.isin(rows[:, 0], cond.vid) & np.isin(rows[:, 2], cond.vid)
        assert known.any() and not known.all()
        out = {}
        for mode in F.MODES:
            out[mode], _ = check(gg, orc, csr, g, table, walks[2], 2, 2, 0, mode, cond, cond_csr)
        # the rows with an unknown id are dropped by inner and semi and kept by anti
        m = F.multiplicity(rows, cond.A, cond.index, 2, 0)
        assert not m[~known].any() and out["anti"]["rows_out"] >= int((~known).sum()) > 0
        assert out["semi"]["rows_out"] == int((m > 0).sum()) > 0 and out["inner"]["rows_out"] == int(m.sum())
    finally:
        table.close()
        cond_csr.close()
        csr.close()


def test_chained_filters_and_the_common_neighbour_filter_behind_them(gg, orc, hard):
    vid, src, dst, g, S, walks = hard
    csr = build(gg, vid, src, dst)
    table = gg.expand_khop_result(csr, 3, S)
    try:
        st1, first = gg.filter_edge(table, 3, csr, 3, 0, "semi")
        try:
            st2, second = gg.filter_edge(first, 3, csr, 1, 3, "anti")
            try:
                ids = g.vid[walks[3]]
                w1, s1 = F.filter_graph(g, ids, 3, 0, "semi")
                w2, s2 = F.filter_graph(g, w1, 1, 3, "anti")
                assert st1 == s1 and st2 == s2 and second.rows(3) == w2.shape[0] > 0
                dense = F.dense_of(g.index, w2.reshape(-1)).reshape(w2.shape)
                assert second.digest(csr, 3) == (w2.shape[0], F.digest_dense_rows(dense))
                out = C.c_void_p()
                gg._chk(gg.lib.gg_result_filter_common_neighbour(gg.ctx, second.handle, 3, csr.handle, C.byref(out)))
                gg.lib.gg_result_destroy(out)
            finally:
                second.close()
        finally:
            first.close()
    finally:
        table.close()
        csr.close()


def test_degenerate_shapes(gg, orc):
    vid = np.array([10, 20, 30], np.int64)
    # an empty source list: 0 rows in, 0 out, a valid result handle
    csr = build(gg, vid, np.array([10, 20], np.int64), np.array([20, 10], np.int64))
    try:
        empty = gg.expand_khop_result(csr, 2, np.empty(0, np.int64))
        try:
            for mode in F.MODES:
                st, res = gg.filter_edge(empty, 2, csr, 2, 0, mode)
                assert st == {"rows_in": 0, "rows_out": 0, "matches": 0} and res.handle and res.rows(2) == 0
                assert fetch_all(res, 2).shape == (0, 3)
                res.close()
        finally:
            empty.close()
        # one input row, 10 -> 20 -> 10: no edge row 10 -> 10 closes it (2 -> 0); the edge row 20 -> 10 is its second hop (1 -> 2)
        one = gg.expand_khop_result(csr, 2, np.array([10], np.int64))
        try:
            assert one.rows(2) == 1
            assert gg.filter_edge(one, 2, csr, 2, 0, "inner", materialise=False)["rows_out"] == 0
            st, res = gg.filter_edge(one, 2, csr, 1, 2, "inner")
            assert st == {"rows_in": 1, "rows_out": 1, "matches": 1} and fetch_all(res, 2).tolist() == [[10, 20, 10]]
            res.close()
            st, res = gg.filter_edge(one, 2, csr, 2, 0, "anti")
            assert st["rows_out"] == 1 and fetch_all(res, 2).tolist() == [[10, 20, 10]]
            res.close()
        finally:
            one.close()
        # a condition graph without edges: every m is 0
        bare = build(gg, vid, np.empty(0, np.int64), np.empty(0, np.int64))
        two = gg.expand_khop_result(csr, 1, None)
        try:
            assert gg.filter_edge(two, 1, bare, 0, 1, "inner", materialise=False) == {"rows_in": 2, "rows_out": 0, "matches": 0}
            st, res = gg.filter_edge(two, 1, bare, 0, 1, "anti")
            assert st == {"rows_in": 2, "rows_out": 2, "matches": 0}
            assert np.array_equal(fetch_all(res, 1), fetch_all(two, 1))
            res.close()
            no_walks = gg.expand_khop_result(bare, 1, None)  # and a walk graph without edges: no rows at all
            assert gg.filter_edge(no_walks, 1, csr, 0, 1, "semi", materialise=False)["rows_in"] == 0
            no_walks.close()
        finally:
            two.close()
            bare.close()
    finally:
        csr.close()
    # a single self-loop, from == to
    csr = build(gg, vid, np.array([10], np.int64), np.array([10], np.int64))
    try:
        loop = gg.expand_khop_result(csr, 1, None)
        st, res = gg.filter_edge(loop, 1, csr, 1, 1, "inner")
        assert st == {"rows_in": 1, "rows_out": 1, "matches": 1} and fetch_all(res, 1).tolist() == [[10, 10]]
        res.close()
        assert gg.filter_edge(loop, 1, csr, 0, 0, "anti", materialise=False)["rows_out"] == 0
        loop.close()
    finally:
        csr.close()


@pytest.mark.parametrize("n_rows_wanted", [1, 63, 65, 257, 1000])
def test_row_counts_that_are_no_multiple_of_the_wavefront_or_the_workgroup(gg, orc, n_rows_wanted):
    """a star: centre 0 -> n leaves, every third leaf -> centre, every sixth twice; the 1-hop table of the centre has n rows"""
    n = n_rows_wanted
    vid = np.arange(100, 100 + n + 1, dtype=np.int64)
    leaves = vid[1:]
    back = np.concatenate([leaves[::3], leaves[::6]])
    src = np.concatenate([np.full(n, vid[0], np.int64), back])
    dst = np.concatenate([leaves, np.full(back.size, vid[0], np.int64)])
    g = T.TriangleGraph(vid, src, dst)
    csr = build(gg, vid, src, dst)
    table = gg.expand_khop_result(csr, 1, vid[:1])
    try:
        assert table.rows(1) == n
        for mode in F.MODES:
            st, m = check(gg, orc, csr, g, table, F.walks(g, vid[:1], 1), 1, 1, 0, mode)
            assert m == 2
    finally:
        table.close()
        csr.close()


def test_errors_leave_the_context_usable(gg, hard):
    vid, src, dst, g, S, walks = hard
    gg.staging_clear()
    gg.append_vertices(vid)
    gg.append_edges(src, dst)
    shard = gg.build_csr_shard(0, 2)
    csr = gg.build_csr()
    table = gg.expand_khop_result(csr, 2, S)
    closure = gg.walk_closure(csr, S[1:2], max_levels=2)
    want = F.filter_graph(g, g.vid[walks[2]], 2, 0, "inner")[1]

    def call(res, hops, graph, fc, tc, mode, materialise=1, out=True):
        st, o = EdgeFilterStats(), C.c_void_p()
        rc = gg.lib.gg_result_filter_edge(gg.ctx, res, hops, graph, fc, tc, mode, materialise, C.byref(st),
                                          C.byref(o) if out else None)
        assert rc != 0 and not o.value
        return rc

    try:
        bad = [
            (call(table.handle, 2, shard.handle, 2, 0, 0), GG_ERR_STATE),        # a shard CSR
            (call(closure.handle, 2, csr.handle, 2, 0, 0), GG_ERR_STATE),        # no fixed-length table
            (call(table.handle, 2, csr.handle, 3, 0, 0), GG_ERR_INVALID_ARG),    # column hops + 1
            (call(table.handle, 2, csr.handle, 2, -1, 0), GG_ERR_INVALID_ARG),   # column -1
            (call(table.handle, 2, csr.handle, 2, 0, 3), GG_ERR_INVALID_ARG),    # mode 3
            (call(table.handle, 3, csr.handle, 2, 0, 0), GG_ERR_INVALID_ARG),    # hops outside the result
            (call(table.handle, 1, csr.handle, 1, 0, 0), GG_ERR_INVALID_ARG),
            (call(None, 2, csr.handle, 2, 0, 0), GG_ERR_INVALID_ARG),
            (call(table.handle, 2, None, 2, 0, 0), GG_ERR_INVALID_ARG),
            (call(table.handle, 2, csr.handle, 2, 0, 0, out=False), GG_ERR_INVALID_ARG),  # materialise without out_result
        ]
        for i, (rc, code) in enumerate(bad):
            assert rc == code, (i, rc, code)
            assert gg.filter_edge(table, 2, csr, 2, 0, "inner", materialise=False) == want  # a correct call still works
        with pytest.raises(GGError) as e:
            gg.filter_edge(table, 2, shard, 2, 0)
        assert e.value.code == GG_ERR_STATE
        with pytest.raises(ValueError):
            gg.filter_edge(table, 2, csr, 2, 0, "outer")
    finally:
        closure.close()
        table.close()
        shard.close()
        csr.close()


@pytest.mark.parametrize("k", [2, 3, 4])
def test_closed_walks_of_a_source_list(gg, orc, hard, k):
    vid, src, dst, g, S, walks = hard
    csr = build(gg, vid, src, dst)
    try:
        want_rows, want = F.filter_graph(g, g.vid[walks[k - 1]], k - 1, 0, "inner")
        assert gg.closed_walks(csr, k, S, materialise=False) == want
        st, res = gg.closed_walks(csr, k, S)
        try:
            assert st == want and res.rows(k - 1) == want["rows_out"] > 0
            dense = F.dense_of(g.index, want_rows.reshape(-1)).reshape(want_rows.shape)
            assert res.digest(csr, k - 1) == (want["rows_out"], F.digest_dense_rows(dense))
            if want["rows_out"] < FETCH_BELOW:
                assert np.array_equal(sort_rows(fetch_all(res, k - 1)), sort_rows(want_rows))
        finally:
            res.close()
        if k == 3:  # on all sources: gg_triangles
            st, res = gg.closed_walks(csr, 3)
            tst, tri = gg.triangles(csr, materialise=True)
            try:
                assert st["rows_out"] == tst["rows"] and res.digest(csr, 2) == (tst["rows"], tst["digest"])
                assert np.array_equal(sort_rows(fetch_all(res, 2)), sort_rows(fetch_all(tri, 2)))
            finally:
                res.close()
                tri.close()
        with pytest.raises(ValueError):
            gg.closed_walks(csr, 1)
    finally:
        csr.close()
