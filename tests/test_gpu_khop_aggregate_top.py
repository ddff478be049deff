"""GG.khop_aggregate_top (gg_khop_aggregate_top) against the restatement in python integers
(tests/khop_aggregate_top_ref.py): every row of every result, in order — group counts around the lane, the wavefront, the
workgroup and the LDS bound, keys that are all equal, ties across the cut, 128-bit signed totals with and without a bias,
unsigned walks, inputs from a source list and from a level in the middle, the top of a top, both sort routes and every
compaction point, every error, every build form."""
import ctypes as C

import numpy as np
import pytest

from duckdb_pgq_amd import GGError
from duckdb_pgq_amd.gg import TopStats
from tests import khop_aggregate_ref as K
from tests import khop_aggregate_top_ref as KT
from tests import triangles_ref as T

pytestmark = pytest.mark.gpu

GG_ERR_INVALID_ARG, GG_ERR_STATE = -1, -6
NEVER, AT_ONCE = 1, 0xFFFFFFFF  # candidate_floor: nothing is left to compact at 1; at once after the first halving pass
LDS_ROWS = 1024
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
EVERY_ORDER = [("total", True), ("total", False), ("walks", True), ("walks", False)]


def weights_of(V, seed=0xA66):
    """random int64 weights with the extremes in front (the weights of tests/test_gpu_khop_aggregate.py)"""
    rng = np.random.RandomState(seed)
    w = rng.randint(-(1 << 62), 1 << 62, size=V, dtype=np.int64) * 2 + rng.randint(0, 2, size=V)
    w[:min(V, 4)] = [I64_MIN, I64_MAX, -1, 0][:min(V, 4)]
    return w


def build(gg, vid, src, dst):
    gg.staging_clear()
    gg.append_vertices(np.asarray(vid, np.int64))
    gg.append_edges(np.asarray(src, np.int64), np.asarray(dst, np.int64))
    return gg.build_csr()


def star(n, base=100):
    """centre <-> n leaves (n = 0: a single vertex with a self-loop): n + 1 groups at every level, in both groupings"""
    vid = np.arange(base, base + n + 1, dtype=np.int64)
    if n == 0:
        return vid, vid.copy(), vid.copy()
    leaves, centre = vid[1:], np.full(n, vid[0], np.int64)
    return vid, np.concatenate([centre, leaves]), np.concatenate([leaves, centre])


def expected_route(rows_out, forced=0):
    if rows_out < 2:
        return 0
    return 1 if forced != 2 and rows_out <= LDS_ROWS else 2


def check_top(gg, agg, level, h, n, order_by="total", descending=True, csr=None, bias=None, g=None, forced=0):
    """one call against the restatement: every row in order, and the stats; returns (rows, stats)"""
    want = KT.top(level, n, order_by, descending, KT.bias_by_id(g, bias) if bias is not None else None)
    top = gg.khop_aggregate_top(agg, h, order_by, descending, n, csr, bias)
    try:
        got, st = top.fetch(h), top.stats
        groups = len(level[1])
        assert K.same(got, want), (order_by, descending, n)
        assert top.rows(h) == st["rows_out"] == min(n, groups) and st["rows_in"] == groups
        assert st["sort_route"] == expected_route(st["rows_out"], forced)
        # bytes of the key: 8 walks or 16 total, + 8 id; nothing to select when every group (or none) is asked for
        assert (st["select_passes"] == 0) if (n == 0 or n >= groups) else (1 <= st["select_passes"] <= (16 if order_by == "walks" else 24))
    finally:
        top.close()
    return got, st


@pytest.fixture(scope="module")
def hard():
    """the hard graph of the aggregate tests, its weights, a bias with the extremes, a list with duplicates and an id that
    is no vertex, and the restatement's levels 1..3 (computed once, never changed)"""
    vid, src, dst = T.hard_graph()
    g = T.TriangleGraph(vid, src, dst)
    indeg = np.bincount(g.dv, minlength=g.V)
    hub = int(indeg.argmax())
    S = np.concatenate([g.vid[[hub, 3, hub, 17, 17, 400]], [-123456789]])
    w = weights_of(g.V)
    bias = weights_of(g.V, 0xB1A5)[::-1].copy()
    want = {(gb, which): K.aggregate(g, 3, gb, None if which == "all" else S, w)
            for gb in K.GROUPS for which in ("all", "list")}
    return vid, src, dst, g, S, w, bias, want


@pytest.mark.parametrize("G", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3000])
def test_group_counts_at_the_lane_wavefront_workgroup_and_route_edges(gg, G):
    vid, src, dst = star(G - 1)
    g = T.TriangleGraph(vid, src, dst)
    w = weights_of(g.V, G)
    level = K.aggregate(g, 1, "start", None, w)[1]
    assert len(level[1]) == G
    csr = build(gg, vid, src, dst)
    agg = gg.khop_aggregate(csr, 1, 1, "start", None, w)
    try:
        for n in (0, 1, G - 1, G, G + 1, 1 << 33):
            for order_by, descending in EVERY_ORDER:
                check_top(gg, agg, level, 1, n, order_by, descending)
    finally:
        agg.close()
        csr.close()


TILE = 4096  # rows per workgroup of the selection's tiled kernels (TOP_TILE, csrc/gg_aggregate_top.hip)


@pytest.mark.parametrize("G", [TILE - 1, TILE, TILE + 1, 9000])
def test_group_counts_across_the_tile_edge_several_workgroups_select_compact_and_place(gg, G):
    """A ring of G vertices with weights: G groups at level 1, every total another random int64 (the key bytes select, in
    every tile), every walks 1 (the ids alone select).  The ids are (i % 2) << 40 | i // 2 in a shuffled table: byte 5 of
    the id halves the candidates and the bytes below it still differ, so with all keys equal the selection compacts half
    the rows — a list that spans two tiles at G = 9000 — and goes on over the list; the library says how long the list was
    (gg_debug_aggregate_top_listed), so the test knows the list path ran, and that it did not where it must not."""
    i = np.arange(G, dtype=np.int64)
    ids = ((i % 2) << 40) | (i // 2)
    vid = ids[np.random.RandomState(G).permutation(G)]
    src, dst = vid, np.roll(vid, 1)
    g = T.TriangleGraph(vid, src, dst)
    w, bias = weights_of(g.V, G), weights_of(g.V, G + 1)[::-1].copy()
    level = K.aggregate(g, 1, "start", None, w)[1]
    assert len(level[1]) == G and set(level[1]) == {1} and len(set(level[2])) > G - 8
    low_half = (G + 1) // 2  # ids with bit 40 clear: they come first in every walks order
    csr = build(gg, vid, src, dst)
    agg = gg.khop_aggregate(csr, 1, 1, "start", None, w)
    by_id = KT.bias_by_id(g, bias)
    try:
        for n in (1, 1000, G // 2 - 1, TILE + 5, G - 1, G, G + 1):
            cases = [(o, d, False) for o, d in EVERY_ORDER] + [("total", True, True), ("total", False, True)]
            for order_by, descending, biased in cases:
                want = KT.top(level, n, order_by, descending, by_id if biased else None)
                # the list the walks orders must write: the half of the rows the rank lies in, if it is at most half of
                # them and the byte did not decide the selection by itself
                rank = min(n, G)
                half = low_half if rank <= low_half else G - low_half
                listed_walks = half if (rank < G and 2 * half <= G and rank not in (low_half,)) else 0
                for route, floor in ((0, 0), (1, NEVER), (2, AT_ONCE), (0, AT_ONCE), (2, NEVER), (0, 3000)):
                    gg.debug_aggregate_top(route, floor)
                    top = gg.khop_aggregate_top(agg, 1, order_by, descending, n, csr if biased else None,
                                                bias if biased else None)
                    try:
                        assert K.same(top.fetch(1), want), (n, order_by, descending, biased, route, floor)
                        st = top.stats
                        assert st["rows_out"] == min(n, G) and st["sort_route"] == expected_route(st["rows_out"], route)
                        listed = gg.debug_aggregate_top_listed()
                        if floor == NEVER or n >= G:
                            assert listed == 0
                        elif order_by == "walks":  # (3000: below the half, and what is left later is decided at once)
                            assert listed == (listed_walks if floor != 3000 or listed_walks <= 3000 else 0), (n, floor)
                        else:
                            assert listed <= G // 2
                    finally:
                        top.close()
    finally:
        agg.close()
        csr.close()


def test_all_keys_equal_the_ids_alone_decide(gg):
    """a ring counted without weights: walks = total = 1 in every group"""
    ids = [I64_MIN, I64_MAX, -1, 0, 1, I64_MIN + 1, I64_MAX - 1]
    ids += [(k << 56) + 0x00ABCDEF12345678 for k in range(-128, 128, 3)]   # differ in their top byte only
    ids += [0x0102030405060700 + k for k in range(0, 256, 5)]               # in their bottom byte only
    ids += [-0x0102030405060700 - k for k in range(0, 256, 7)]
    vid = np.array(ids, np.int64)
    assert np.unique(vid).size == vid.size
    vid = vid[np.random.RandomState(11).permutation(vid.size)]
    src, dst = vid, np.roll(vid, 1)
    g = T.TriangleGraph(vid, src, dst)
    level = K.aggregate(g, 1, "start", None, None)[1]
    assert set(level[1]) == {1} and set(level[2]) == {1} and len(level[1]) == vid.size
    csr = build(gg, vid, src, dst)
    agg = gg.khop_aggregate(csr, 1, 1, "start", None, None)
    try:
        for floor in (0, NEVER, AT_ONCE):
            gg.debug_aggregate_top(0, floor)
            for n in (1, 2, 5, vid.size // 2, vid.size - 1, vid.size):
                for order_by, descending in EVERY_ORDER:
                    got, st = check_top(gg, agg, level, 1, n, order_by, descending)
                    assert got[0].tolist() == sorted(vid.tolist())[:n]  # ascending ids in both directions
                    if n < vid.size:  # the key bytes select nothing: the passes reach the id bytes
                        assert st["select_passes"] > (8 if order_by == "walks" else 16)
    finally:
        agg.close()
        csr.close()


def test_ties_across_the_cut_keep_the_smaller_id_in_both_directions(gg):
    """in-stars of equal fan, grouped by the end without weights: runs of ten groups with the same walks"""
    rng = np.random.RandomState(5)
    fans = [2] * 10 + [3] * 10 + [4] * 10
    centres = rng.permutation(np.arange(1000, 1030)).astype(np.int64)
    leaves = np.arange(5000, 5000 + sum(fans), dtype=np.int64)
    vid = rng.permutation(np.concatenate([centres, leaves]))
    src, dst = leaves, np.repeat(centres, fans)
    g = T.TriangleGraph(vid, src, dst)
    level = K.aggregate(g, 1, "end", None, None)[1]
    assert sorted(level[1]) == fans
    csr = build(gg, vid, src, dst)
    agg = gg.khop_aggregate(csr, 1, 1, "end", None, None)
    try:
        for floor in (0, NEVER, AT_ONCE):
            gg.debug_aggregate_top(0, floor)
            for order_by in KT.ORDERS:
                for descending in (True, False):
                    for n in (9, 10, 11, 15, 19, 20, 21, 29):  # the middle run: its first, inside, its last, one past
                        got, _ = check_top(gg, agg, level, 1, n, order_by, descending)
                        run = [int(i) for i, c in zip(got[0], got[1]) if c == 3]
                        assert run == sorted(run) and len(run) == min(max(n - 10, 0), 10)
    finally:
        agg.close()
        csr.close()


def test_128_bit_signed_order_and_a_bias_that_carries_and_flips_the_sign(gg, hard):
    vid, src, dst, g, S, w, bias, want = hard
    level = want[("start", "all")][2]
    totals, by_id = level[2], KT.bias_by_id(g, bias)
    # the properties the order has to get right, on the restatement: totals beyond +-2^63 of both signs, high words that
    # differ, low words with and without their top bit, a bias whose addition carries out of the low word, one that
    # flips the sign
    assert min(totals) < -(1 << 63) and max(totals) >= 1 << 63 and len({t >> 64 for t in totals}) > 2
    assert {(t >> 63) & 1 for t in totals} == {0, 1}
    pairs = [(t, by_id[int(i)]) for i, t in zip(level[0], totals)]
    assert any(b > 0 and (t % K.M64) + b >= K.M64 for t, b in pairs) and any(b < 0 and (t % K.M64) + b < 0 for t, b in pairs)
    assert any((t < 0) != (K.wrap128(t + b) < 0) for t, b in pairs)
    csr = build(gg, vid, src, dst)
    agg = gg.khop_aggregate(csr, 1, 3, "start", None, w)
    try:
        for descending in (True, False):
            for n in (1, 100, 1024, 1025, len(totals) - 1, len(totals)):
                check_top(gg, agg, level, 2, n, "total", descending)
                check_top(gg, agg, level, 2, n, "total", descending, csr, bias, g)
        # the star of the aggregate tests: three leaves of 2^62 pass int64, leaves of -1 borrow, +-2^62 cancel
        for ws in ([0, 1 << 62, 1 << 62, 1 << 62], [0, -1, -1, -1], [5, 1 << 62, -(1 << 62), 0], [I64_MIN, I64_MAX, I64_MIN, -1]):
            svid, ssrc, sdst = star(3)
            sg = T.TriangleGraph(svid, ssrc, sdst)
            sw = np.array(ws, np.int64)
            scsr = build(gg, svid, ssrc, sdst)
            sagg = gg.khop_aggregate(scsr, 1, 2, "end", None, sw)
            try:
                for h in (1, 2):
                    lv = K.aggregate(sg, 2, "end", None, sw)[h]
                    for n in (1, 2, 3, 4):
                        for descending in (True, False):
                            check_top(gg, sagg, lv, h, n, "total", descending)
                            check_top(gg, sagg, lv, h, n, "total", descending, scsr, np.array([1, -1, I64_MAX, I64_MIN], np.int64), sg)
            finally:
                sagg.close()
                scsr.close()
    finally:
        agg.close()
        csr.close()


def dense_multigraph():
    """12 vertices, every ordered pair joined by 20..60 parallel rows: ~480 rows out of every vertex, 480^8 ~ 2^71: the
    counts of level 8 have wrapped"""
    rng = np.random.RandomState(0x8E)
    vid = rng.permutation(np.arange(-6, 6)).astype(np.int64) * 1000
    mult = rng.randint(20, 61, size=(12, 12))
    a, b = np.nonzero(mult)
    return vid, np.repeat(vid[a], mult[a, b]), np.repeat(vid[b], mult[a, b])


def test_walks_are_ordered_unsigned(gg):
    vid, src, dst = dense_multigraph()
    g = T.TriangleGraph(vid, src, dst)
    # no weights: the library forms no sum, total = walks as they wrapped (include/gg.h)
    levels = {h: (ids, walks, list(walks)) for h, (ids, walks, _) in K.aggregate(g, 8, "start", None, None).items()}
    level = levels[8]
    assert any(c >= 1 << 63 for c in level[1]) and any(c < 1 << 63 for c in level[1])  # a signed compare would misplace
    csr = build(gg, vid, src, dst)
    agg = gg.khop_aggregate(csr, 1, 8, "start", None, None)
    try:
        for h in (7, 8):
            for n in (1, 3, 11, 12):
                for descending in (True, False):
                    check_top(gg, agg, levels[h], h, n, "walks", descending)
                    check_top(gg, agg, levels[h], h, n, "total", descending)  # the same values as a signed 128-bit key
    finally:
        agg.close()
        csr.close()


@pytest.mark.parametrize("group_by", K.GROUPS)
def test_inputs_from_a_source_list_and_a_level_in_the_middle(gg, hard, group_by):
    vid, src, dst, g, S, w, bias, want = hard
    csr = build(gg, vid, src, dst)
    listed = gg.khop_aggregate(csr, 1, 3, group_by, S, w)
    every = gg.khop_aggregate(csr, 1, 3, group_by, None, w)
    try:
        for agg, which in ((listed, "list"), (every, "all")):
            level = want[(group_by, which)][2]  # k_min < 2 < k_max
            groups = len(level[1])
            assert groups > 3
            for n in (1, 3, groups // 2, groups, groups + 1):
                for order_by, descending in EVERY_ORDER:
                    check_top(gg, agg, level, 2, n, order_by, descending)
                check_top(gg, agg, level, 2, n, "total", True, csr, bias, g)
        for h in (1, 3):
            check_top(gg, listed, want[(group_by, "list")][h], h, 20, "total", False, csr, bias, g)
    finally:
        listed.close()
        every.close()
        csr.close()


def test_the_top_of_a_top_and_the_input_stays_as_it_was(gg, hard):
    vid, src, dst, g, S, w, bias, want = hard
    level = want[("end", "all")][2]
    csr = build(gg, vid, src, dst)
    agg = gg.khop_aggregate(csr, 2, 2, "end", None, w)
    try:
        before = agg.fetch(2)
        for order_by, descending in EVERY_ORDER:
            b = bias if order_by == "total" else None
            for m in (1200, 300):  # above and below the LDS bound
                first = gg.khop_aggregate_top(agg, 2, order_by, descending, m, csr if b is not None else None, b)
                try:
                    mid = KT.top(level, m, order_by, descending, KT.bias_by_id(g, b) if b is not None else None)
                    assert K.same(first.fetch(2), mid)
                    for n in (0, 1, 100, m, m + 7):
                        got, _ = check_top(gg, first, mid, 2, n, order_by, descending, csr if b is not None else None, b, g)
                        assert K.same(got, KT.top(level, min(n, m), order_by, descending,
                                                  KT.bias_by_id(g, b) if b is not None else None))
                    # the other direction over the top m: its worst rows first
                    check_top(gg, first, mid, 2, 10, order_by, not descending, csr if b is not None else None, b, g)
                    assert K.same(first.fetch(2), mid)
                    with pytest.raises(GGError):  # one level: the others are outside it
                        gg.khop_aggregate_top(first, 1, order_by, descending, 5)
                finally:
                    first.close()
        assert K.same(agg.fetch(2), before) and K.same(before, level)
    finally:
        agg.close()
        csr.close()


def test_every_route_and_every_compaction_point_give_the_same_rows(gg, hard):
    vid, src, dst, g, S, w, bias, want = hard
    level = want[("start", "all")][3]
    groups = len(level[1])
    assert groups > LDS_ROWS + 1
    csr = build(gg, vid, src, dst)
    agg = gg.khop_aggregate(csr, 3, 3, "start", None, w)
    try:
        gg.profile(True)
        for n in (2, 100, LDS_ROWS, LDS_ROWS + 1, groups):
            seen = {}
            for route in (0, 1, 2):
                for floor in (0, NEVER, AT_ONCE):
                    gg.debug_aggregate_top(route, floor)
                    gg.profile_reset()
                    for order_by, descending, b in (("total", True, bias), ("walks", False, None)):
                        got, st = check_top(gg, agg, level, 3, n, order_by, descending, csr if b is not None else None, b, g,
                                            forced=route)
                        again, st2 = check_top(gg, agg, level, 3, n, order_by, descending, csr if b is not None else None,
                                               b, g, forced=route)
                        assert K.same(got, again) and st == st2  # the same call twice
                        key = (order_by, descending)
                        rows = (got[0].tolist(), [int(x) for x in got[1]], [int(x) for x in got[2]], st["rows_out"])
                        assert seen.setdefault(key, rows) == rows
                    names = gg.profile_get()
                    took = expected_route(min(n, groups), route)
                    assert ("top_sort_lds" in names) == (took == 1) and ("top_chunk" in names) == (took == 2)
                    assert "top_gather" in names and ("top_hist" in names) == ("top_pick" in names) == (n < groups)
        # the knob goes back with the others
        gg.debug_aggregate_top(2, AT_ONCE)
        gg.debug_reset()
        _, st = check_top(gg, agg, level, 3, 100, "total", True)
        assert st["sort_route"] == 1
        with pytest.raises(GGError):
            gg.debug_aggregate_top(3, 0)
    finally:
        gg.profile(False)
        agg.close()
        csr.close()


def test_errors_leave_the_context_usable(gg, hard):
    vid, src, dst, g, S, w, bias, want = hard
    level = want[("start", "all")][2]
    gg.staging_clear()
    gg.append_vertices(vid)
    gg.append_edges(src, dst)
    shard = gg.build_csr_shard(0, 2)
    csr = gg.build_csr()
    agg = gg.khop_aggregate(csr, 1, 2, "start", None, w)
    table = gg.expand_khop_result(csr, 1, S)
    other = type(gg)(0)
    other.append_vertices(vid)
    other.append_edges(src, dst)
    foreign = other.build_csr()  # the same graph, built in another context
    # another graph: some of the aggregate's ids are no vertices of it
    ovid, osrc, odst = star(40, base=int(g.vid.min()))
    ocsr = build(gg, ovid, osrc, odst)
    obias = np.arange(ocsr.V, dtype=np.int64)
    bp = bias.ctypes.data_as(C.POINTER(C.c_int64))

    def call(ctx, res, hops, order_by, graph=None, b=None, out=True, n=10):
        st, o = TopStats(), C.c_void_p()
        rc = gg.lib.gg_khop_aggregate_top(ctx, res, hops, order_by, 1, n, graph, b, C.byref(st), C.byref(o) if out else None)
        assert rc != 0 and not o.value
        return rc

    try:
        bad = [
            (call(None, agg.handle, 2, 0), GG_ERR_INVALID_ARG),
            (call(gg.ctx, None, 2, 0), GG_ERR_INVALID_ARG),
            (call(gg.ctx, agg.handle, 2, 0, out=False), GG_ERR_INVALID_ARG),
            (call(other.ctx, agg.handle, 2, 0), GG_ERR_INVALID_ARG),               # a result of another context
            (call(gg.ctx, agg.handle, 2, 0, foreign.handle, bp), GG_ERR_INVALID_ARG),  # a csr of another context
            (call(gg.ctx, agg.handle, 2, 0, foreign.handle), GG_ERR_INVALID_ARG),      # ... also without a bias
            (call(gg.ctx, agg.handle, 0, 0), GG_ERR_INVALID_ARG),                  # levels outside the input's
            (call(gg.ctx, agg.handle, 3, 0), GG_ERR_INVALID_ARG),
            (call(gg.ctx, agg.handle, 2, 2), GG_ERR_INVALID_ARG),                  # order_by outside {0, 1}
            (call(gg.ctx, agg.handle, 2, -1), GG_ERR_INVALID_ARG),
            (call(gg.ctx, agg.handle, 2, 0, None, bp), GG_ERR_INVALID_ARG),        # a bias without csr
            (call(gg.ctx, agg.handle, 2, 1, csr.handle, bp), GG_ERR_INVALID_ARG),  # a bias with the walks
            (call(gg.ctx, table.handle, 1, 0), GG_ERR_STATE),                      # not an aggregate
            (call(gg.ctx, agg.handle, 2, 0, shard.handle, bp), GG_ERR_STATE),      # a shard CSR
            (call(gg.ctx, agg.handle, 2, 0, ocsr.handle, obias.ctypes.data_as(C.POINTER(C.c_int64))), GG_ERR_STATE),
        ]
        for i, (rc, code) in enumerate(bad):
            assert rc == code, (i, rc, code)
            check_top(gg, agg, level, 2, 50, "total", True, csr, bias, g)  # a correct call still works
        with pytest.raises(ValueError):
            gg.khop_aggregate_top(agg, 2, "sum")
        with pytest.raises(ValueError):
            gg.khop_aggregate_top(agg, 2, "total", True, 5, csr, bias[:-1])
        with pytest.raises(ValueError):
            gg.khop_aggregate_top(agg, 2, "total", True, 5, None, bias)
        # the answer is an aggregate result: the walk tables' calls refuse it
        top = gg.khop_aggregate_top(agg, 2, "walks", True, 5)
        try:
            n = C.c_uint64()
            assert gg.lib.gg_result_rows(top.handle, 2, C.byref(n)) == GG_ERR_STATE
            assert gg.lib.gg_khop_aggregate_rows(top.handle, 1, C.byref(n)) == GG_ERR_INVALID_ARG
            assert top.rows(2) == 5
        finally:
            top.close()
    finally:
        table.close()
        agg.close()
        foreign.close()
        other.close()
        ocsr.close()
        shard.close()
        csr.close()


@pytest.mark.parametrize("form", ["legacy_build", "no_rowid", "derived_reverse"])
def test_every_build_form(gg, form):
    from duckdb_pgq_amd import datagen

    vid, s, d = datagen.ldbc_knows(1200, 9000, 5)
    src, dst = np.concatenate([s, d]), np.concatenate([d, s])
    g = T.TriangleGraph(vid, src, dst)
    w, bias = weights_of(g.V, 9), weights_of(g.V, 10)
    if form == "legacy_build":
        gg.force_legacy_build(True)
    else:
        gg.set_edge_rowid(False)
    if form == "derived_reverse":
        gg.rank_mode(1)
    csr = build(gg, vid, src, dst)
    try:
        if form == "derived_reverse":
            assert csr.reverse_derived == 1
        for group_by in K.GROUPS:
            level = K.aggregate(g, 2, group_by, None, w)[2]
            agg = gg.khop_aggregate(csr, 2, 2, group_by, None, w)
            try:
                for n in (100, len(level[1])):
                    check_top(gg, agg, level, 2, n, "total", True, csr, bias, g)
                    check_top(gg, agg, level, 2, n, "walks", False)
            finally:
                agg.close()
    finally:
        csr.close()
