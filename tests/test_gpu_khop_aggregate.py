"""GG.khop_aggregate (gg_khop_aggregate) against the restatement in python integers (tests/khop_aggregate_ref.py): every row
of every level, in order, plus the stats — both groupings, all sources and a list, with and without weights, on both routes
of the pull kernel and every build form, on shapes that carry, cancel and change sign, on row lengths around the lane group
and the workgroup, eight levels deep, on degenerate inputs and through every error.  Two cross-checks of independent
kernels: stats.walks[h] is gg_khop_count's rows[h], and for h <= 2 the aggregate is a group-by over the rows
gg_expand_khop_result materialises."""
import ctypes as C

import numpy as np
import pytest

from duckdb_pgq_amd import GGError
from duckdb_pgq_amd.gg import AggStats
from tests import khop_aggregate_ref as K
from tests import triangles_ref as T

pytestmark = pytest.mark.gpu

GG_ERR_INVALID_ARG, GG_ERR_STATE = -1, -6
NO_LONG_ROWS = 0xFFFFFFFF
PIECE = 65_536


def weights_of(V, seed=0xA66):
    """random int64 weights with the extremes in front"""
    rng = np.random.RandomState(seed)
    w = rng.randint(-(1 << 62), 1 << 62, size=V, dtype=np.int64) * 2 + rng.randint(0, 2, size=V)
    w[:min(V, 4)] = [-(1 << 63), (1 << 63) - 1, -1, 0][:min(V, 4)]
    return w


@pytest.fixture(scope="module")
def hard():
    """the graph, its weights, the list [hub, dense 3, hub, the self-loop vertices, an id that is no vertex] and the
    restatement's answers for k = 1..4 (computed once, never changed)"""
    vid, src, dst = T.hard_graph()
    g = T.TriangleGraph(vid, src, dst)
    indeg, outdeg = np.bincount(g.dv, minlength=g.V), np.diff(g.off)
    hub = int(indeg.argmax())
    assert indeg[hub] > 512 and outdeg[hub] > 512  # the hub's rows are long ones in both directions by default
    loops = np.nonzero(g.A.diagonal())[0].tolist()
    assert len(loops) == 2
    S = np.concatenate([g.vid[[hub, 3, hub] + loops], [-123456789]])
    w = weights_of(g.V)
    want = {(gb, which, wt): K.aggregate(g, 4, gb, None if which == "all" else S, w if wt else None)
            for gb in K.GROUPS for which in ("all", "list") for wt in (True, False)}
    # the sums are not trivial: high halves of both signs and neither 0 nor -1 from level 1 on
    his = [t >> 64 for t in want[("start", "all", True)][1][2]]
    assert min(his) < -1 and max(his) > 0
    return vid, src, dst, g, S, w, want


def build(gg, vid, src, dst):
    gg.staging_clear()
    gg.append_vertices(np.asarray(vid, np.int64))
    gg.append_edges(np.asarray(src, np.int64), np.asarray(dst, np.int64))
    return gg.build_csr()


def passes(k_max, group_by, sources, weights):
    """pull passes of a call: level 1 off an implicit level 0 reads the entries only to gather weights"""
    implicit0 = group_by == "start" or sources is None
    return k_max - (1 if implicit0 and weights is None else 0)


def check(gg, csr, g, k_min, k_max, group_by, sources, weights, want=None):
    """one call against the restatement (want: its answer where the caller has it); returns {h: (ids, walks, totals)}"""
    want = want or K.aggregate(g, k_max, group_by, sources, weights)
    agg = gg.khop_aggregate(csr, k_min, k_max, group_by, sources, weights)
    try:
        got = {h: agg.fetch(h) for h in range(k_min, k_max + 1)}
        st = agg.stats
        for h in range(k_min, k_max + 1):
            ids, walks, totals = want[h]
            print(group_by, "h", h, "groups", st["groups"][h], len(walks), "walks", st["walks"][h], sum(walks) % K.M64)
            assert K.same(got[h], want[h]), (group_by, h)
            assert agg.rows(h) == st["groups"][h] == len(walks)
            assert st["walks"][h] == sum(walks) % K.M64
        for h in range(0, T_MAX + 1):
            if not k_min <= h <= k_max:
                assert st["groups"][h] == st["walks"][h] == 0
        assert st["entries_pulled"] == passes(k_max, group_by, sources, weights) * csr.E
        only = gg.khop_aggregate(csr, k_min, k_max, group_by, sources, weights, fetch=False)
        assert only.handle is None and only.stats == st  # out_result NULL: the stats alone
    finally:
        agg.close()
    return got


T_MAX = 8  # GG_MAX_HOPS


@pytest.mark.parametrize("which", ["all", "list"])
@pytest.mark.parametrize("group_by", K.GROUPS)
def test_every_level_of_the_hard_graph_equals_the_restatement(gg, hard, group_by, which):
    vid, src, dst, g, S, w, want = hard
    sources = None if which == "all" else S
    csr = build(gg, vid, src, dst)
    try:
        got = check(gg, csr, g, 1, 4, group_by, sources, w, want[(group_by, which, True)])
        plain = check(gg, csr, g, 1, 4, group_by, sources, None, want[(group_by, which, False)])
        counted = gg.khop_count(csr, 1, 4, sources)  # an independent kernel
        for h in range(1, 5):
            assert sum(int(x) for x in got[h][1]) % K.M64 == counted[h] > 0
            assert [int(x) for x in plain[h][1]] == [int(x) for x in plain[h][2]]  # no weights: total == walks
            assert np.array_equal(plain[h][0], got[h][0]) and np.array_equal(plain[h][1], got[h][1])
        # a window of levels is the same rows
        check(gg, csr, g, 3, 4, group_by, sources, w, want[(group_by, which, True)])
    finally:
        csr.close()


def fetch_all(res, hops):
    n = res.rows(hops)
    out = np.empty((hops + 1, max(n, 1)), np.int64)
    i64p = C.POINTER(C.c_int64)
    for o in range(0, n, PIECE):
        ptrs = (i64p * (hops + 1))(*[out[c, o:].ctypes.data_as(i64p) for c in range(hops + 1)])
        got = C.c_uint32()
        res.gg._chk(res.gg.lib.gg_result_fetch(res.handle, hops, o, min(PIECE, n - o), ptrs, C.byref(got)))
        assert got.value == min(PIECE, n - o)
    return out[:, :n].T.copy()


def numpy_group_by(g, id_rows, group_by, w):
    """the brute-force group-by of the restatement over fetched id rows"""
    order = np.argsort(g.vid, kind="stable")
    return K.group_rows(g, order[np.searchsorted(g.vid[order], id_rows)], group_by, w)


@pytest.mark.parametrize("which", ["all", "list"])
def test_aggregate_is_the_group_by_over_the_materialised_rows(gg, hard, which):
    vid, src, dst, g, S, w, want = hard
    sources = None if which == "all" else S
    csr = build(gg, vid, src, dst)
    try:
        for h in (1, 2):
            table = gg.expand_khop_result(csr, h, sources)
            try:
                rows = fetch_all(table, h)
            finally:
                table.close()
            assert rows.shape[0] > 0
            for group_by in K.GROUPS:
                agg = gg.khop_aggregate(csr, h, h, group_by, sources, w)
                try:
                    assert K.same(agg.fetch(h), numpy_group_by(g, rows, group_by, w)), (h, group_by)
                    assert agg.stats["walks"][h] == rows.shape[0]
                finally:
                    agg.close()
    finally:
        csr.close()


@pytest.mark.parametrize("route", ["long_1", "long_16", "long_17", "default", "no_long_rows", "legacy_build", "no_rowid"])
def test_every_route_gives_the_restatement_s_rows(gg, hard, route):
    vid, src, dst, g, S, w, want = hard
    if route == "legacy_build":
        gg.force_legacy_build(True)
    if route == "no_rowid":
        gg.set_edge_rowid(False)
    csr = build(gg, vid, src, dst)
    if route.startswith("long_"):
        gg.debug_aggregate_long_row(int(route[5:]))
    if route == "no_long_rows":
        gg.debug_aggregate_long_row(NO_LONG_ROWS)
    if route == "default":
        gg.debug_aggregate_long_row(7)
        gg.debug_reset()  # restores the knob as well
    try:
        gg.profile(True)
        gg.profile_reset()
        for group_by in K.GROUPS:
            check(gg, csr, g, 1, 3, group_by, S, w, want[(group_by, "list", True)])
            check(gg, csr, g, 1, 3, group_by, None, w, want[(group_by, "all", True)])
            check(gg, csr, g, 2, 3, group_by, S, None, want[(group_by, "list", False)])
        seen = gg.profile_get()
        print(route, {k: v for k, v in seen.items() if k.startswith("agg_")})
        assert "agg_pull" in seen
        assert ("agg_pull_long" in seen) == (route != "no_long_rows")
    finally:
        gg.profile(False)
        csr.close()


def test_a_fully_mirrored_table_whose_reverse_rows_are_derived(gg):
    from duckdb_pgq_amd import datagen

    vid, s, d = datagen.ldbc_knows(1200, 9000, 5)
    hub = vid[7]
    fan = vid[np.random.RandomState(3).choice(1200, 700, replace=False)]
    s, d = np.concatenate([s, np.full(fan.size, hub, np.int64)]), np.concatenate([d, fan])
    src, dst = np.concatenate([s, d]), np.concatenate([d, s])
    g = T.TriangleGraph(vid, src, dst)
    w = weights_of(g.V, 9)
    gg.set_edge_rowid(False)  # the vertex-sorted form of the bucketed build is the one that derives
    gg.rank_mode(1)
    csr = build(gg, vid, src, dst)
    try:
        assert csr.reverse_derived == 1  # what END reads is the derived reverse
        S = np.concatenate([vid[[7, 2, 7]], [-5]])
        for thr in (0, 1, NO_LONG_ROWS):
            gg.debug_aggregate_long_row(thr)
            for group_by in K.GROUPS:
                check(gg, csr, g, 1, 3, group_by, None, w)
                check(gg, csr, g, 1, 3, group_by, S, w)
    finally:
        csr.close()


def star(n, base=100):
    """centre <-> n leaves (n = 0: a single vertex with a self-loop): the centre's row has n entries in both directions"""
    vid = np.arange(base, base + n + 1, dtype=np.int64)
    if n == 0:
        return vid, vid.copy(), vid.copy()
    leaves, centre = vid[1:], np.full(n, vid[0], np.int64)
    return vid, np.concatenate([centre, leaves]), np.concatenate([leaves, centre])


def test_carries_signs_and_cancellation_on_a_star(gg):
    vid, src, dst = star(3)
    g = T.TriangleGraph(vid, src, dst)
    csr = build(gg, vid, src, dst)
    try:
        for thr in (0, 1, NO_LONG_ROWS):
            gg.debug_aggregate_long_row(thr)
            for group_by in K.GROUPS:
                # three leaves of 2^62: the sum leaves the int64 range
                got = check(gg, csr, g, 1, 1, group_by, None, np.array([0, 1 << 62, 1 << 62, 1 << 62], np.int64))[1]
                assert int(got[0][0]) == 100 and int(got[1][0]) == 3 and got[2][0] == 3 << 62
                # leaves of -1: the low half wraps, the high half is -1
                agg = gg.khop_aggregate(csr, 1, 1, group_by, None, np.array([0, -1, -1, -1], np.int64))
                lo, hi = np.empty(4, np.uint64), np.empty(4, np.int64)
                ids, walks, n = np.empty(4, np.int64), np.empty(4, np.uint64), C.c_uint32()
                gg._chk(gg.lib.gg_khop_aggregate_fetch(agg.handle, 1, 0, 4, ids.ctypes.data_as(C.POINTER(C.c_int64)),
                                                       walks.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                       lo.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                       hi.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(n)))
                assert n.value == 4 and int(lo[0]) == (1 << 64) - 3 and int(hi[0]) == -1 and agg.fetch(1)[2][0] == -3
                gg._chk(gg.lib.gg_khop_aggregate_fetch(agg.handle, 1, 4, 4, ids.ctypes.data_as(C.POINTER(C.c_int64)),
                                                       walks.ctypes.data_as(C.POINTER(C.c_uint64)), None, None, C.byref(n)))
                assert n.value == 0  # past the end
                agg.close()
                # +-2^62 cancel to 0 while walks > 0: the group stays
                got = check(gg, csr, g, 1, 2, group_by, None, np.array([5, 1 << 62, -(1 << 62), 0], np.int64))
                assert int(got[1][1][0]) == 3 and got[1][2][0] == 0 and len(got[1][1]) == 4
                # the extremes next to each other
                check(gg, csr, g, 1, 3, group_by, None, np.array([-(1 << 63), (1 << 63) - 1, -(1 << 63), -1], np.int64))
    finally:
        csr.close()


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000])
def test_row_lengths_and_vertex_counts_off_the_lane_group_and_the_workgroup(gg, n):
    """V = n + 1: 1, 17 and 257 among them"""
    vid, src, dst = star(n)
    g = T.TriangleGraph(vid, src, dst)
    w = weights_of(g.V, n)
    csr = build(gg, vid, src, dst)
    try:
        assert csr.V == n + 1
        for thr in (0, 1, NO_LONG_ROWS):  # the default, every row of two entries or more long, none long
            gg.debug_aggregate_long_row(thr)
            for group_by in K.GROUPS:
                check(gg, csr, g, 1, 3, group_by, None, w)
                check(gg, csr, g, 1, 2, group_by, vid[[0, n, 0]], w)
    finally:
        csr.close()


def test_eight_levels_deep_totals_pass_64_bits(gg):
    """a complete graph of 6 vertices with self-loops and one parallel row; weights near 2^60"""
    vid = np.array([40, 10, 60, 20, 50, 30], np.int64)
    src, dst = np.repeat(vid, 6), np.tile(vid, 6)
    src, dst = np.append(src, 10), np.append(dst, 60)
    g = T.TriangleGraph(vid, src, dst)
    w = (1 << 60) + np.array([0, -3, 7, 1 << 59, -(1 << 61), 11], np.int64)
    csr = build(gg, vid, src, dst)
    try:
        for thr in (0, 1):
            gg.debug_aggregate_long_row(thr)
            for group_by in K.GROUPS:
                got = check(gg, csr, g, 1, 8, group_by, None, w)
                assert max(abs(t) for t in got[8][2]) >= 1 << 64
                check(gg, csr, g, 1, 8, group_by, vid[[1, 1, 4]], w)
    finally:
        csr.close()


def test_degenerate_inputs(gg, hard):
    vid, src, dst, g, S, w, want = hard
    csr = build(gg, vid, src, dst)
    try:
        for group_by in K.GROUPS:
            for sources in (np.empty(0, np.int64), np.array([-5, -6, -123456789], np.int64)):  # empty; no vertex in it
                agg = gg.khop_aggregate(csr, 1, 3, group_by, sources, w)
                assert agg.handle and [agg.rows(h) for h in (1, 2, 3)] == [0, 0, 0]
                assert agg.fetch(2)[0].size == 0 and sum(agg.stats["groups"]) == sum(agg.stats["walks"]) == 0
                agg.close()
    finally:
        csr.close()
    bare = build(gg, vid[:40], np.empty(0, np.int64), np.empty(0, np.int64))  # a graph without edges
    try:
        for group_by in K.GROUPS:
            agg = gg.khop_aggregate(bare, 1, 2, group_by, None, w[:40])
            assert agg.rows(1) == agg.rows(2) == 0 and agg.stats["entries_pulled"] == 0
            agg.close()
    finally:
        bare.close()


def test_errors_leave_the_context_usable(gg, hard):
    vid, src, dst, g, S, w, want = hard
    gg.staging_clear()
    gg.append_vertices(vid)
    gg.append_edges(src, dst)
    shard = gg.build_csr_shard(0, 2)
    csr = gg.build_csr()
    other = type(gg)(0)
    i64p = C.POINTER(C.c_int64)

    def call(ctx, graph, k_min, k_max, group_by, stats=True, out=True):
        st, o = AggStats(), C.c_void_p()
        rc = gg.lib.gg_khop_aggregate(ctx, graph, None, 0, k_min, k_max, group_by, None,
                                      C.byref(st) if stats else None, C.byref(o) if out else None)
        assert rc != 0 and not o.value
        return rc

    try:
        bad = [
            (call(None, csr.handle, 1, 2, 0), GG_ERR_INVALID_ARG),
            (call(gg.ctx, None, 1, 2, 0), GG_ERR_INVALID_ARG),
            (call(other.ctx, csr.handle, 1, 2, 0), GG_ERR_INVALID_ARG),   # a CSR of another context
            (call(gg.ctx, csr.handle, 0, 2, 0), GG_ERR_INVALID_ARG),
            (call(gg.ctx, csr.handle, 1, 9, 0), GG_ERR_INVALID_ARG),
            (call(gg.ctx, csr.handle, 3, 2, 0), GG_ERR_INVALID_ARG),
            (call(gg.ctx, csr.handle, 1, 2, 2), GG_ERR_INVALID_ARG),
            (call(gg.ctx, csr.handle, 1, 2, -1), GG_ERR_INVALID_ARG),
            (call(gg.ctx, csr.handle, 1, 2, 0, stats=False, out=False), GG_ERR_INVALID_ARG),
            (call(gg.ctx, shard.handle, 1, 2, 0), GG_ERR_STATE),
        ]
        for i, (rc, code) in enumerate(bad):
            assert rc == code, (i, rc, code)
            check(gg, csr, g, 2, 2, "end", S, w, want[("end", "list", True)])  # a correct call still works
        with pytest.raises(ValueError):
            gg.khop_aggregate(csr, 1, 2, "middle")
        with pytest.raises(ValueError):
            gg.khop_aggregate(csr, 1, 2, "start", None, w[:-1])
        # the result answers its own two calls only, and they answer no other result
        agg = gg.khop_aggregate(csr, 1, 2, "start", S, w)
        table = gg.expand_khop_result(csr, 1, S)
        try:
            n, got = C.c_uint64(), C.c_uint32()
            buf = np.empty((4, 8), np.int64)
            ptrs = (i64p * 3)(*[buf[c].ctypes.data_as(i64p) for c in range(3)])
            assert gg.lib.gg_result_rows(agg.handle, 1, C.byref(n)) == GG_ERR_STATE
            assert gg.lib.gg_result_fetch(agg.handle, 1, 0, 8, ptrs, C.byref(got)) == GG_ERR_STATE
            assert gg.lib.gg_result_fetch_edges(agg.handle, 1, 0, 8, ptrs, C.byref(got)) == GG_ERR_STATE
            assert gg.lib.gg_khop_aggregate_rows(table.handle, 1, C.byref(n)) == GG_ERR_STATE
            assert gg.lib.gg_khop_aggregate_fetch(table.handle, 1, 0, 8, buf[0].ctypes.data_as(i64p),
                                                  buf[1].ctypes.data_as(C.POINTER(C.c_uint64)),
                                                  buf[2].ctypes.data_as(C.POINTER(C.c_uint64)),
                                                  buf[3].ctypes.data_as(i64p), C.byref(got)) == GG_ERR_STATE
            assert gg.lib.gg_khop_aggregate_rows(agg.handle, 3, C.byref(n)) == GG_ERR_INVALID_ARG  # a level not asked for
            assert K.same(agg.fetch(2), want[("start", "list", True)][2])
        finally:
            table.close()
            agg.close()
    finally:
        other.close()
        shard.close()
        csr.close()
