"""GG.khop_pair_counts (gg_khop_pair_counts) against the restatement in python integers (tests/khop_pair_counts_ref.py):
every row of every level, in order, rows(h) and all four stats fields — on both pull routes, with and without the mask
skip, on in-row lengths around the routes' edges, on lane counts and vertex counts around the wavefront and the tile, where
counts wrap, with targets, on degenerate inputs, on every build form and through the errors.  Two cross-checks of
independent kernels: stats.walks[h] is gg_khop_count's rows[h], and for h <= 2 the rows are a group-by over the rows
gg_expand_khop_result materialises.

Not covered here: GG_ERR_TOO_LARGE needs a level of 2^32 rows, that is 2^26 vertices and 64 GiB of state, and GG_ERR_OOM
needs a state (1 KiB per vertex) larger than the device's memory; neither fits a test of seconds."""
import ctypes as C

import numpy as np
import pytest

from duckdb_pgq_amd import GGError
from duckdb_pgq_amd.gg import PairStats
from tests import khop_pair_counts_ref as P
from tests import triangles_ref as T

pytestmark = pytest.mark.gpu

GG_ERR_INVALID_ARG, GG_ERR_STATE = -1, -6
NO_LONG_ROWS = 0xFFFFFFFF
T_MAX = 8  # GG_MAX_HOPS
PIECE = 65_536


def build(gg, vid, src, dst):
    gg.staging_clear()
    gg.append_vertices(np.asarray(vid, np.int64))
    gg.append_edges(np.asarray(src, np.int64), np.asarray(dst, np.int64))
    return gg.build_csr()


def check(gg, csr, g, k_min, k_max, sources, targets=None, want=None, gather_all=False):
    """one call against the restatement (want: its answer where the caller has it); returns {h: (idx, ids, walks)}"""
    want = want or P.pair_counts(g, k_max, sources, targets)
    res = gg.khop_pair_counts(csr, k_min, k_max, sources, targets)
    try:
        got = {h: res.fetch(h) for h in range(k_min, k_max + 1)}
        st = res.stats
        for h in range(k_min, k_max + 1):
            idx, ids, walks = want["rows"][h]
            print("h", h, "pairs", st["pairs"][h], len(walks), "walks", st["walks"][h], sum(walks) % P.M64)
            assert P.same(got[h], want["rows"][h]), h
            assert res.rows(h) == st["pairs"][h] == len(walks)
            assert st["walks"][h] == sum(walks) % P.M64
        for h in range(0, T_MAX + 1):
            if not k_min <= h <= k_max:
                assert st["pairs"][h] == st["walks"][h] == 0
        print("entries_pulled", st["entries_pulled"], want["entries_pulled"], "rows_gathered", st["rows_gathered"],
              want["rows_gathered"])
        assert st["entries_pulled"] == want["entries_pulled"]
        assert st["rows_gathered"] == (want["entries_pulled"] if gather_all else want["rows_gathered"])
        only = gg.khop_pair_counts(csr, k_min, k_max, sources, targets, fetch=False)
        assert only.parts == [] and only.stats == st  # out_result NULL: the stats alone
    finally:
        res.close()
    return got


@pytest.fixture(scope="module")
def hard():
    """the graph, 64 sources = [hub, hub again, both self-loop vertices, the negative id, an id that is no vertex, 58 others]
    and the restatement's answers for k = 1..4 (computed once, never changed)"""
    vid, src, dst = T.hard_graph()
    g = T.TriangleGraph(vid, src, dst)
    indeg = np.bincount(g.dv, minlength=g.V)
    hub = int(indeg.argmax())
    assert indeg[hub] > 512  # the hub's in-row is a long one by default
    loops = np.nonzero(g.A.diagonal())[0].tolist()
    assert len(loops) == 2 and -77 in g.index
    head = [int(g.vid[hub]), int(g.vid[hub]), int(g.vid[loops[0]]), int(g.vid[loops[1]]), -77, -123456789]
    others = [int(x) for x in g.vid.tolist() if int(x) not in head][:58]
    S = np.array(head + others, np.int64)
    assert S.size == 64
    return vid, src, dst, g, S, P.pair_counts(g, 4, S)


@pytest.fixture(scope="module")
def small():
    vid, src, dst = T.hard_graph(V=300, rows=3000, seed=0x51, hub_fan=120)
    return vid, src, dst, T.TriangleGraph(vid, src, dst)


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


def test_every_level_of_the_hard_graph_equals_the_restatement(gg, hard):
    vid, src, dst, g, S, want = hard
    csr = build(gg, vid, src, dst)
    try:
        got = check(gg, csr, g, 1, 4, S, None, want)
        check(gg, csr, g, 3, 4, S, None, want)  # a window of levels is the same rows
        counted = gg.khop_count(csr, 1, 4, S)  # an independent kernel
        for h in range(1, 5):
            assert sum(int(x) for x in got[h][2]) % P.M64 == counted[h] > 0
        # lanes 0 and 1 are the same vertex: equal rows
        for h in range(1, 5):
            a, b = got[h][0] == 0, got[h][0] == 1
            assert a.sum() > 0 and np.array_equal(got[h][1][a], got[h][1][b]) and np.array_equal(got[h][2][a], got[h][2][b])
        # the group-by over the materialised walk rows: a source listed m times has m times the rows
        mult = {int(s): int((S == s).sum()) for s in S.tolist()}
        for h in (1, 2):
            table = gg.expand_khop_result(csr, h, S)
            try:
                rows = fetch_all(table, h)
            finally:
                table.close()
            keys, cnt = np.unique(rows[:, [0, h]], axis=0, return_counts=True)
            by_pair = {(int(a), int(b)): int(c) for (a, b), c in zip(keys.tolist(), cnt.tolist())}
            idx, ids, walks = got[h]
            assert len(by_pair) == len({(int(S[i]), int(v)) for i, v in zip(idx.tolist(), ids.tolist())})
            for i, v, w in zip(idx.tolist(), ids.tolist(), walks.tolist()):
                assert by_pair[(int(S[i]), int(v))] == int(w) * mult[int(S[i])]
    finally:
        csr.close()


@pytest.mark.parametrize("gather_mode", [0, 1])
@pytest.mark.parametrize("long_row", [1, NO_LONG_ROWS, 0])
def test_both_pull_routes_with_and_without_the_skip_give_the_same_rows(gg, hard, long_row, gather_mode):
    vid, src, dst, g, S, want = hard
    csr = build(gg, vid, src, dst)
    try:
        gg.debug_pair_counts(long_row, gather_mode)
        gg.profile(True)
        gg.profile_reset()
        check(gg, csr, g, 1, 4, S, None, want, gather_all=gather_mode == 1)
        seen = gg.profile_get()
        print(long_row, gather_mode, {k: v for k, v in seen.items() if k.startswith("pc_")})
        assert "pc_pull" in seen and "pc_count" in seen and "pc_write" in seen
        assert ("pc_pull_long" in seen) == (long_row != NO_LONG_ROWS)
        gg.debug_pair_counts(7, 1)
        gg.debug_reset()  # restores both knobs
        check(gg, csr, g, 2, 2, S[:5], None, None)
        with pytest.raises(GGError) as e:
            gg.debug_pair_counts(0, 2)
        assert e.value.code == GG_ERR_INVALID_ARG
        with pytest.raises(GGError):
            gg.debug_pair_counts(0, -1)
    finally:
        gg.profile(False)
        csr.close()


def star_plus_ring():
    """a ring of 1025 leaves (in-degree 1; 2 for the 16 a centre points back at), and 16 centres whose in-degrees are 0, 1, 2, 3, 4, 5, 63, 64, 65, 255,
    256, 257, 511, 512, 513 and 1025: centre k is wired from the first d_k leaves and points back at leaf k"""
    degs = [0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025]
    n = 1025
    leaves = np.arange(1000, 1000 + n, dtype=np.int64)
    centres = np.arange(10, 10 + len(degs), dtype=np.int64)
    src, dst = [leaves], [np.roll(leaves, -1)]
    for k, d in enumerate(degs):
        src += [leaves[:d], centres[k:k + 1]]
        dst += [np.full(d, centres[k], np.int64), leaves[k:k + 1]]
    return np.concatenate([centres, leaves]), np.concatenate(src), np.concatenate(dst), degs


def test_row_lengths_around_the_routes_edges(gg):
    vid, src, dst, degs = star_plus_ring()
    g = T.TriangleGraph(vid, src, dst)
    indeg = np.bincount(g.dv, minlength=g.V)
    assert indeg[:len(degs)].tolist() == degs
    # 16 centres, leaves on both sides of every in-row's end, two lanes on one leaf
    S = np.concatenate([vid[:16], vid[16 + np.array([0, 1, 2, 3, 4, 62, 63, 64, 254, 255, 256, 510, 511, 512, 1023, 1024, 0])]])
    want = P.pair_counts(g, 3, S)
    csr = build(gg, vid, src, dst)
    try:
        for long_row in (0, 1, 64, NO_LONG_ROWS):
            for gather_mode in (0, 1):
                gg.debug_pair_counts(long_row, gather_mode)
                check(gg, csr, g, 1, 3, S, None, want, gather_all=gather_mode == 1)
    finally:
        csr.close()


@pytest.mark.parametrize("n", [1, 2, 63, 64])
def test_lane_counts(gg, small, n):
    vid, src, dst, g = small
    hub = int(np.bincount(g.dv, minlength=g.V).argmax())
    S = np.concatenate([g.vid[[hub]], g.vid[:63]])[:n]
    csr = build(gg, vid, src, dst)
    try:
        check(gg, csr, g, 1, 3, S)
    finally:
        csr.close()


def test_a_list_of_130_runs_in_three_batches_and_none_is_every_vertex(gg, small):
    vid, src, dst, g = small
    S = np.concatenate([g.vid[:129], [-4]])  # the last batch: one vertex and an id that is none
    csr = build(gg, vid, src, dst)
    try:
        got = check(gg, csr, g, 1, 2, S)
        assert got[2][0].max() == 128 and (np.diff(got[2][0]) >= 0).all()  # the batch offsets are in the source index
    finally:
        csr.close()
    keep = np.isin(src, vid[:200]) & np.isin(dst, vid[:200])
    g2 = T.TriangleGraph(vid[:200], src[keep], dst[keep])
    csr = build(gg, vid[:200], src[keep], dst[keep])
    try:
        assert csr.V == 200
        want = P.pair_counts(g2, 2, g2.vid)
        check(gg, csr, g2, 1, 2, None, None, want)
        check(gg, csr, g2, 1, 2, g2.vid, None, want)
    finally:
        csr.close()


@pytest.mark.parametrize("V", [1, 63, 64, 65, 128, 129])
def test_tile_edges(gg, V):
    """a ring plus random chords; the lane-major scan crosses tile boundaries with empty and full tiles"""
    rng = np.random.RandomState(V)
    vid = (np.arange(V, dtype=np.int64) * 7 + 3)[rng.permutation(V)]
    chords = rng.randint(0, V, size=(2, 3 * V))
    src = np.concatenate([vid, vid[chords[0]]])
    dst = np.concatenate([np.roll(vid, -1), vid[chords[1]]])
    g = T.TriangleGraph(vid, src, dst)
    S = vid[:64]
    csr = build(gg, vid, src, dst)
    try:
        for long_row in (0, 1):
            gg.debug_pair_counts(long_row, 0)
            check(gg, csr, g, 1, 3, S)
        # one source whose level-1 rows sit in the last tile only: every other tile is empty
        check(gg, csr, g, 1, 1, vid[V - 1:V])
    finally:
        csr.close()


@pytest.mark.parametrize("back", [256, 255])
def test_counts_wrap_mod_2_64(gg, back):
    a, b = 5, 9
    vid = np.array([a, b], np.int64)
    src = np.concatenate([np.full(256, a), np.full(back, b)]).astype(np.int64)
    dst = np.concatenate([np.full(256, b), np.full(back, a)]).astype(np.int64)
    g = T.TriangleGraph(vid, src, dst)
    csr = build(gg, vid, src, dst)
    try:
        for long_row in (0, 1):
            gg.debug_pair_counts(long_row, 0)
            got = check(gg, csr, g, 1, 8, [a, b])
            lane0 = got[8][0] == 0
            if back == 256:  # 256^8 = 2^64 = 0 at (a, a): the pair is absent and level 8 of that lane is empty
                assert lane0.sum() == 0 and got[7][2][got[7][0] == 0].tolist() == [256 ** 7]
            else:
                assert got[8][1][lane0].tolist() == [a] and int(got[8][2][lane0][0]) == (256 * 255) ** 4 > 1 << 63
    finally:
        csr.close()


def test_targets_filter_the_rows_never_the_recurrence(gg, small):
    vid, src, dst, g = small
    hub = int(np.bincount(g.dv, minlength=g.V).argmax())
    S = np.concatenate([g.vid[[hub, 3, hub, 17, 250]], [-123456789]])
    targets = np.concatenate([g.vid[[3, 40, 40, 7, 299]], [S[0]], [-999]])  # a duplicate, a source itself, a non-vertex
    csr = build(gg, vid, src, dst)
    try:
        full = check(gg, csr, g, 1, 3, S)
        cut = check(gg, csr, g, 1, 3, S, targets)
        assert len(cut[3][2]) > 0
        for h in (1, 2, 3):
            assert P.same(cut[h], P.filtered(full[h], g, targets))
        only3 = check(gg, csr, g, 3, 3, S, targets)
        assert P.same(only3[3], P.filtered(full[3], g, targets))
        none = check(gg, csr, g, 1, 2, S, np.empty(0, np.int64))  # n_dst = 0 with a list: no rows
        assert len(none[1][2]) == len(none[2][2]) == 0
        every = check(gg, csr, g, 1, 2, S, g.vid)
        assert P.same(every[2], full[2])
    finally:
        csr.close()


def test_degenerate_inputs(gg, small):
    vid, src, dst, g = small
    csr = build(gg, vid, src, dst)
    try:
        got = check(gg, csr, g, 1, 3, np.array([-5, -6, -123456789], np.int64))  # no vertex among the sources
        assert all(len(got[h][2]) == 0 for h in (1, 2, 3))
        empty = gg.khop_pair_counts(csr, 1, 2, np.empty(0, np.int64))  # an empty list: no batch
        assert empty.rows(1) == 0 and empty.fetch(2)[0].size == 0 and sum(empty.stats["pairs"]) == 0
        empty.close()
    finally:
        csr.close()
    none = np.empty(0, np.int64)
    bare = build(gg, vid[:40], none, none)  # a graph without edges
    try:
        got = check(gg, bare, T.TriangleGraph(vid[:40], none, none), 1, 2, vid[:5])
        assert len(got[1][2]) == 0
    finally:
        bare.close()
    one = np.array([42], np.int64)
    loop = build(gg, one, one, one)  # V = 1 with a self-loop
    try:
        got = check(gg, loop, T.TriangleGraph(one, one, one), 1, 8, np.array([42, 42, 7], np.int64))
        assert got[8][0].tolist() == [0, 1] and got[8][1].tolist() == [42, 42] and got[8][2].tolist() == [1, 1]
    finally:
        loop.close()


@pytest.mark.parametrize("form", ["legacy_build", "no_rowid"])
def test_build_forms(gg, hard, form):
    vid, src, dst, g, S, want = hard
    if form == "legacy_build":
        gg.force_legacy_build(True)
    else:
        gg.set_edge_rowid(False)
    csr = build(gg, vid, src, dst)
    try:
        check(gg, csr, g, 1, 4, S, None, want)
    finally:
        csr.close()


def test_a_fully_mirrored_table_whose_reverse_rows_are_derived(gg):
    from duckdb_pgq_amd import datagen

    vid, s, d = datagen.ldbc_knows(1200, 9000, 5)
    hub = vid[7]
    fan = vid[np.random.RandomState(3).choice(1200, 700, replace=False)]
    s, d = np.concatenate([s, np.full(fan.size, hub, np.int64)]), np.concatenate([d, fan])
    src, dst = np.concatenate([s, d]), np.concatenate([d, s])
    g = T.TriangleGraph(vid, src, dst)
    gg.set_edge_rowid(False)  # the vertex-sorted form of the bucketed build is the one that derives
    gg.rank_mode(1)
    csr = build(gg, vid, src, dst)
    try:
        assert csr.reverse_derived == 1  # what the pull reads is the derived reverse
        S = np.concatenate([vid[[7, 2, 7]], [-5], vid[100:120]])
        want = P.pair_counts(g, 3, S)
        for long_row in (0, 1, NO_LONG_ROWS):
            gg.debug_pair_counts(long_row, 0)
            check(gg, csr, g, 1, 3, S, None, want)
    finally:
        csr.close()


def test_errors_leave_the_context_usable(gg, small):
    vid, src, dst, g = small
    gg.staging_clear()
    gg.append_vertices(vid)
    gg.append_edges(src, dst)
    shard = gg.build_csr_shard(0, 2)
    csr = gg.build_csr()
    other = type(gg)(0)
    i64p, u64p = C.POINTER(C.c_int64), C.POINTER(C.c_uint64)
    S = np.ascontiguousarray(g.vid[:4])
    sp = S.ctypes.data_as(i64p)
    want = P.pair_counts(g, 2, S)

    def call(ctx, graph, srcs, n_src, k_min, k_max, dst=None, n_dst=0, stats=True, out=True):
        st, o = PairStats(), C.c_void_p()
        rc = gg.lib.gg_khop_pair_counts(ctx, graph, srcs, n_src, k_min, k_max, dst, n_dst,
                                        C.byref(st) if stats else None, C.byref(o) if out else None)
        assert rc != 0 and not o.value
        return rc

    try:
        bad = [
            lambda: (call(None, csr.handle, sp, 4, 1, 2), GG_ERR_INVALID_ARG),
            lambda: (call(gg.ctx, None, sp, 4, 1, 2), GG_ERR_INVALID_ARG),
            lambda: (call(gg.ctx, csr.handle, None, 4, 1, 2), GG_ERR_INVALID_ARG),
            lambda: (call(other.ctx, csr.handle, sp, 4, 1, 2), GG_ERR_INVALID_ARG),  # a CSR of another context
            lambda: (call(gg.ctx, csr.handle, sp, 0, 1, 2), GG_ERR_INVALID_ARG),
            lambda: (call(gg.ctx, csr.handle, sp, 65, 1, 2), GG_ERR_INVALID_ARG),
            lambda: (call(gg.ctx, csr.handle, sp, -1, 1, 2), GG_ERR_INVALID_ARG),
            lambda: (call(gg.ctx, csr.handle, sp, 4, 0, 2), GG_ERR_INVALID_ARG),
            lambda: (call(gg.ctx, csr.handle, sp, 4, 1, 9), GG_ERR_INVALID_ARG),
            lambda: (call(gg.ctx, csr.handle, sp, 4, 3, 2), GG_ERR_INVALID_ARG),
            lambda: (call(gg.ctx, csr.handle, sp, 4, 1, 2, None, 3), GG_ERR_INVALID_ARG),  # targets without a list
            lambda: (call(gg.ctx, csr.handle, sp, 4, 1, 2, stats=False, out=False), GG_ERR_INVALID_ARG),
            lambda: (gg.lib.gg_debug_pair_counts(gg.ctx, 0, 2), GG_ERR_INVALID_ARG),
            lambda: (gg.lib.gg_debug_pair_counts(gg.ctx, 0, -1), GG_ERR_INVALID_ARG),
            lambda: (gg.lib.gg_debug_pair_counts(None, 0, 0), GG_ERR_INVALID_ARG),
            lambda: (call(gg.ctx, shard.handle, sp, 4, 1, 2), GG_ERR_STATE),
        ]
        for i, case in enumerate(bad):
            rc, code = case()
            assert rc == code, (i, rc, code)
            check(gg, csr, g, 2, 2, S, None, want)  # a correct call still works
        # the result answers its own two calls only, and they answer no other result
        res = gg.khop_pair_counts(csr, 1, 2, S)
        agg = gg.khop_aggregate(csr, 1, 2, "end", S)
        table = gg.expand_khop_result(csr, 1, S)
        try:
            handle = res.parts[0][0]
            n, got = C.c_uint64(), C.c_uint32()
            buf = np.empty((4, 8), np.int64)
            ptrs = (i64p * 3)(*[buf[c].ctypes.data_as(i64p) for c in range(3)])
            assert gg.lib.gg_result_rows(handle, 1, C.byref(n)) == GG_ERR_STATE
            assert gg.lib.gg_result_fetch(handle, 1, 0, 8, ptrs, C.byref(got)) == GG_ERR_STATE
            assert gg.lib.gg_result_fetch_edges(handle, 1, 0, 8, ptrs, C.byref(got)) == GG_ERR_STATE
            assert gg.lib.gg_khop_aggregate_rows(handle, 1, C.byref(n)) == GG_ERR_STATE
            assert gg.lib.gg_khop_aggregate_fetch(handle, 1, 0, 8, buf[0].ctypes.data_as(i64p), buf[1].ctypes.data_as(u64p),
                                                  None, None, C.byref(got)) == GG_ERR_STATE
            levels = C.c_int()
            assert gg.lib.gg_walk_closure_levels(handle, None, 0, C.byref(levels)) == GG_ERR_STATE
            for h in (agg.handle, table.handle):
                assert gg.lib.gg_khop_pair_counts_rows(h, 1, C.byref(n)) == GG_ERR_STATE
                assert gg.lib.gg_khop_pair_counts_fetch(h, 1, 0, 8, buf[0].ctypes.data_as(i64p), buf[1].ctypes.data_as(i64p),
                                                        buf[2].ctypes.data_as(u64p), C.byref(got)) == GG_ERR_STATE
            assert gg.lib.gg_khop_pair_counts_rows(handle, 3, C.byref(n)) == GG_ERR_INVALID_ARG  # a level not asked for
            assert gg.lib.gg_khop_pair_counts_rows(None, 1, C.byref(n)) == GG_ERR_INVALID_ARG
            # the fetch's conventions: any output may be NULL, nothing past the end
            total = res.rows(2)
            assert total > 8
            assert gg.lib.gg_khop_pair_counts_fetch(handle, 2, total - 3, 8, None, buf[1].ctypes.data_as(i64p), None,
                                                    C.byref(got)) == 0 and got.value == 3
            assert buf[1][:3].tolist() == want["rows"][2][1][-3:].tolist()
            assert gg.lib.gg_khop_pair_counts_fetch(handle, 2, 0, 8, None, None, None, C.byref(got)) == 0 and got.value == 8
            assert gg.lib.gg_khop_pair_counts_fetch(handle, 2, total, 8, buf[0].ctypes.data_as(i64p), None, None,
                                                    C.byref(got)) == 0 and got.value == 0
            assert P.same(res.fetch(2), want["rows"][2])
        finally:
            table.close()
            agg.close()
            res.close()
    finally:
        other.close()
        shard.close()
        csr.close()
