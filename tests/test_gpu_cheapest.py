"""GG.cheapest64 / GG.cheapest_path_lengths (gg_cheapest64 over a gg_edge_weights) against the restatement in python
integers (tests/cheapest_ref.py): every row in order, rows() and all five stats fields — on hand graphs where the hop bound
changes the answer, at the saturation point, on in-row lengths, lane counts and vertex counts around the wavefront and the
tile, on both pull routes with the threshold at, below and above a row's length, with and without the mask skip, with
targets, on a chain of 300 rounds, with weights given in all four forms, on every build form and through the errors.  One
cross-check of an independent kernel: with unit weights cost = hops = gg_bfs64's distances.

Not covered here: GG_ERR_TOO_LARGE needs 2^32 rows, that is 2^26 vertices reached from 64 sources and 120 GiB of state, and
GG_ERR_OOM needs a state (1.8 KiB per vertex) larger than the device's memory; neither fits a test of seconds."""
import ctypes as C

import numpy as np
import pytest

from duckdb_pgq_amd import GGError
from duckdb_pgq_amd.gg import CheapestStats
from tests import cheapest_ref as R
from tests import edge_ids as EI
from tests import lazy_reverse_tables as LT
from tests import triangles_ref as T

pytestmark = pytest.mark.gpu

GG_ERR_INVALID_ARG, GG_ERR_STATE = -1, -6
NO_LONG_ROWS = 0xFFFFFFFF
INT64_MAX = R.INT64_MAX
STATS = ("rounds", "reached_pairs", "cells_lowered", "entries_pulled", "rows_gathered")


def build(gg, vid, src, dst, rowid=None):
    gg.staging_clear()
    gg.append_vertices(np.asarray(vid, np.int64))
    gg.append_edges(np.asarray(src, np.int64), np.asarray(dst, np.int64), rowid)
    return gg.build_csr()


def check(gg, csr, w, g, sources, max_hops=-1, targets=None, want=None, gather_all=False):
    """one call against the restatement (want: its answer where the caller has it); returns (idx, ids, cost, hops)"""
    want = want or R.cheapest(g, sources, max_hops, targets)
    res = gg.cheapest_path_lengths(csr, w, sources, max_hops, targets)
    try:
        got, st = res.fetch(), res.stats
        print("rows", res.rows(), len(want["rows"][2]), {k: (st[k], want[k]) for k in STATS})
        assert R.same(got, want["rows"])
        assert got[3].dtype == np.int32 and got[2].dtype == np.int64
        assert res.rows() == len(want["rows"][2])
        for k in STATS:
            if k == "rows_gathered" and gather_all:
                assert st[k] == want["entries_pulled"]
            else:
                assert st[k] == want[k], k
        only = gg.cheapest_path_lengths(csr, w, sources, max_hops, targets, fetch=False)
        assert only.parts == [] and only.stats == st  # out_result NULL: the stats alone
    finally:
        res.close()
    return got


def rows_of(got):
    return list(zip(got[0].tolist(), got[1].tolist(), [int(x) for x in got[2]], [int(x) for x in got[3]]))


def run_tiny(gg, edges, sources, max_hops=-1, targets=None, vid=(1, 2, 3, 4)):
    vid = np.array(vid, np.int64)
    src, dst, wt = (np.array(x, np.int64) for x in zip(*edges))
    g = R.WeightedGraph(vid, src, dst, wt)
    csr = build(gg, vid, src, dst)
    w = gg.edge_weights(csr, wt)
    try:
        return rows_of(check(gg, csr, w, g, np.array(sources, np.int64), max_hops, targets))
    finally:
        w.close()
        csr.close()


@pytest.fixture(scope="module")
def hard():
    """the graph of tests/test_gpu_khop_pair_counts.py with hashed weights; 64 sources = [hub, hub again, both self-loop
    vertices, the negative id, an id that is no vertex, 58 others] and the restatement's fixpoint (computed once)"""
    vid, src, dst = T.hard_graph()
    wt = R.hashed_weights(src.size)
    g = R.WeightedGraph(vid, src, dst, wt)
    tg = T.TriangleGraph(vid, src, dst)
    indeg = np.bincount(tg.dv, minlength=tg.V)
    hub = int(indeg.argmax())
    assert indeg[hub] > 512  # the hub's in-row is a long one by default
    loops = np.nonzero(tg.A.diagonal())[0].tolist()
    assert len(loops) == 2 and -77 in g.index
    head = [int(g.vid[hub]), int(g.vid[hub]), int(g.vid[loops[0]]), int(g.vid[loops[1]]), -77, -123456789]
    others = [int(x) for x in g.vid.tolist() if int(x) not in head][:58]
    S = np.array(head + others, np.int64)
    assert S.size == 64
    return vid, src, dst, wt, g, S, R.cheapest(g, S)


@pytest.fixture(scope="module")
def small():
    vid, src, dst = T.hard_graph(V=300, rows=3000, seed=0x51, hub_fan=120)
    wt = R.hashed_weights(src.size)
    g = R.WeightedGraph(vid, src, dst, wt)
    indeg = np.bincount(np.asarray(g.dv), minlength=g.V)
    return vid, src, dst, wt, g, int(indeg.argmax()), int(indeg.max())


def test_the_hop_bound_changes_the_answer(gg):
    detour = [(1, 3, 10), (1, 2, 1), (2, 3, 2)]  # a direct edge of weight 10 beside a 2-edge detour of weight 3
    assert run_tiny(gg, detour, [1], 1) == [(0, 1, 0, 0), (0, 2, 1, 1), (0, 3, 10, 1)]
    assert run_tiny(gg, detour, [1], 2) == [(0, 1, 0, 0), (0, 2, 1, 1), (0, 3, 3, 2)]
    assert run_tiny(gg, detour, [1], -1) == [(0, 1, 0, 0), (0, 2, 1, 1), (0, 3, 3, 2)]  # 4 is unreachable: no row
    assert run_tiny(gg, detour, [1], 0) == [(0, 1, 0, 0)]
    assert run_tiny(gg, detour, [1], 1 << 40) == [(0, 1, 0, 0), (0, 2, 1, 1), (0, 3, 3, 2)]


def test_parallel_rows_self_loops_zero_cycles_and_ties(gg):
    assert run_tiny(gg, [(1, 2, 7), (1, 2, 4), (1, 2, 9), (2, 2, 0), (1, 1, 3)], [1]) == [(0, 1, 0, 0), (0, 2, 4, 1)]
    # a zero-weight 2-cycle 2 <-> 3 behind 1, and a zero-weight tie: 1 -> 4 directly (5) and through 2 (5 + 0)
    got = run_tiny(gg, [(1, 2, 5), (2, 3, 0), (3, 2, 0), (1, 4, 5), (2, 4, 0)], [1, 3])
    assert got == [(0, 1, 0, 0), (0, 2, 5, 1), (0, 3, 5, 2), (0, 4, 5, 1), (1, 2, 0, 1), (1, 3, 0, 0), (1, 4, 0, 2)]


def test_costs_saturate_at_int64_max(gg):
    got = run_tiny(gg, [(1, 2, 1 << 62), (2, 3, 1 << 62), (3, 4, 1 << 62)], [1])
    assert got == [(0, 1, 0, 0), (0, 2, 1 << 62, 1), (0, 3, INT64_MAX, 2), (0, 4, INT64_MAX, 3)]
    got = run_tiny(gg, [(1, 2, INT64_MAX), (2, 3, 1)], [1])
    assert got == [(0, 1, 0, 0), (0, 2, INT64_MAX, 1), (0, 3, INT64_MAX, 2)]


def star_plus_ring():
    """a ring of 131 leaves and 10 centres whose in-degrees are 0, 1, 2, 3, 4, 5, 63, 64, 65 and 131: centre k is wired from
    the first d_k leaves and points back at leaf k"""
    degs = [0, 1, 2, 3, 4, 5, 63, 64, 65, 131]
    n = 131
    leaves = np.arange(1000, 1000 + n, dtype=np.int64)
    centres = np.arange(10, 10 + len(degs), dtype=np.int64)
    src, dst = [leaves], [np.roll(leaves, -1)]
    for k, d in enumerate(degs):
        src += [leaves[:d], centres[k:k + 1]]
        dst += [np.full(d, centres[k], np.int64), leaves[k:k + 1]]
    return np.concatenate([centres, leaves]), np.concatenate(src), np.concatenate(dst), degs


def test_row_lengths_around_the_wavefront_and_few_live_entries(gg):
    vid, src, dst, degs = star_plus_ring()
    wt = R.hashed_weights(src.size, 0, 9)  # zero weights among them
    g = R.WeightedGraph(vid, src, dst, wt)
    indeg = np.bincount(np.asarray(g.dv), minlength=g.V)
    assert indeg[:len(degs)].tolist() == degs
    leaves = vid[len(degs):]
    csr = build(gg, vid, src, dst)
    w = gg.edge_weights(csr, wt)
    try:
        for n_live in (1, 2, 3, 4, 5):  # round 1 finds exactly n_live live entries in the chunks of the long in-rows
            S = leaves[:n_live]
            want = R.cheapest(g, S, 2)
            for long_row in (0, 1, 64, NO_LONG_ROWS):
                gg.debug_cheapest(long_row, 0)
                check(gg, csr, w, g, S, 2, None, want)
        S = np.concatenate([vid[:10], leaves[[0, 1, 2, 3, 4, 62, 63, 64, 65, 129, 130, 0]]])
        want = R.cheapest(g, S)
        for long_row in (0, 1, 63, 64, 65, NO_LONG_ROWS):
            for gather_mode in (0, 1):
                gg.debug_cheapest(long_row, gather_mode)
                check(gg, csr, w, g, S, -1, None, want, gather_all=gather_mode == 1)
    finally:
        w.close()
        csr.close()


@pytest.mark.parametrize("n", [1, 63, 64])
def test_lane_counts(gg, small, n):
    vid, src, dst, wt, g, hub, _ = small
    S = np.concatenate([g.vid[[hub]], g.vid[:63]])[:n]
    csr = build(gg, vid, src, dst)
    w = gg.edge_weights(csr, wt)
    try:
        check(gg, csr, w, g, S)
        res = gg.cheapest64(csr, w, S, 2)  # the single call
        assert R.same(res.fetch(), R.cheapest(g, S, 2)["rows"])
        res.close()
    finally:
        w.close()
        csr.close()


@pytest.mark.parametrize("V", [63, 64, 65, 129])
def test_tile_edges(gg, V):
    """a ring plus random chords; the lane-major scan crosses tile boundaries with empty and full tiles"""
    rng = np.random.RandomState(V)
    vid = (np.arange(V, dtype=np.int64) * 7 + 3)[rng.permutation(V)]
    chords = rng.randint(0, V, size=(2, 3 * V))
    src = np.concatenate([vid, vid[chords[0]]])
    dst = np.concatenate([np.roll(vid, -1), vid[chords[1]]])
    wt = R.hashed_weights(src.size)
    g = R.WeightedGraph(vid, src, dst, wt)
    csr = build(gg, vid, src, dst)
    w = gg.edge_weights(csr, wt)
    try:
        for long_row in (0, 1):
            gg.debug_cheapest(long_row, 0)
            check(gg, csr, w, g, vid[:64])
        check(gg, csr, w, g, vid[V - 1:V], 1)  # one source in the last tile, one round
    finally:
        w.close()
        csr.close()


def test_the_threshold_at_below_and_above_the_hub_row(gg, small):
    vid, src, dst, wt, g, hub, fan = small
    S = np.concatenate([g.vid[[hub]], g.vid[:40]])
    want = R.cheapest(g, S)
    csr = build(gg, vid, src, dst)
    w = gg.edge_weights(csr, wt)
    try:
        for long_row in (fan, fan - 1, fan + 1, 8):
            for gather_mode in (0, 1):
                gg.debug_cheapest(long_row, gather_mode)
                gg.profile(True)
                gg.profile_reset()
                check(gg, csr, w, g, S, -1, None, want, gather_all=gather_mode == 1)
                seen = gg.profile_get()
                assert "cp_pull" in seen and "cp_pull_long" in seen and "cp_count" in seen and "cp_write" in seen
        gg.debug_cheapest(NO_LONG_ROWS, 0)
        gg.profile_reset()
        check(gg, csr, w, g, S, -1, None, want)
        assert "cp_pull_long" not in gg.profile_get()
        gg.debug_cheapest(7, 1)
        gg.debug_reset()  # restores both knobs
        check(gg, csr, w, g, S, -1, None, want)
        with pytest.raises(GGError) as e:
            gg.debug_cheapest(0, 2)
        assert e.value.code == GG_ERR_INVALID_ARG
    finally:
        gg.profile(False)
        w.close()
        csr.close()


def test_the_hard_graph_sources_targets_and_determinism(gg, hard):
    vid, src, dst, wt, g, S, want = hard
    csr = build(gg, vid, src, dst)
    w = gg.edge_weights(csr, wt)
    try:
        got = check(gg, csr, w, g, S, -1, None, want)  # the default threshold: the hub's in-row is a long one
        a, b = got[0] == 0, got[0] == 1  # lanes 0 and 1 are the same vertex: equal rows
        assert a.sum() > 100 and all(np.array_equal(got[c][a], got[c][b]) for c in (1, 2, 3))
        assert not (got[0] == 5).any()  # a source that is no vertex has no rows
        check(gg, csr, w, g, S, -1, None, want)  # a second run: the same bits
        gg.max_grid_tiles(3)
        check(gg, csr, w, g, S, -1, None, want)
        gg.max_grid_tiles(0)
        gg.debug_cheapest(0, 1)
        check(gg, csr, w, g, S, -1, None, want, gather_all=True)
        gg.debug_cheapest(0, 0)
        targets = np.concatenate([g.vid[[3, 40, 40, 7, 299]], [S[0]], [-999]])  # a duplicate, a source itself, a non-vertex
        cut = check(gg, csr, w, g, S, -1, targets)
        allowed = set(targets.tolist())
        keep = np.array([int(v) in allowed for v in got[1].tolist()])
        assert len(cut[0]) > 0 and all(np.array_equal(cut[c], got[c][keep]) for c in range(4))
        none = check(gg, csr, w, g, S, -1, np.empty(0, np.int64))  # n_dst = 0 with a list: no rows
        assert none[0].size == 0
        check(gg, csr, w, g, S, 2)  # and a bound
    finally:
        w.close()
        csr.close()


def test_a_chain_of_300_runs_299_lowering_rounds(gg):
    vid = np.arange(300, dtype=np.int64) * 3 + 1
    src, dst = vid[:-1], vid[1:]
    wt = R.hashed_weights(src.size)
    g = R.WeightedGraph(vid, src, dst, wt)
    csr = build(gg, vid, src, dst)
    w = gg.edge_weights(csr, wt)
    try:
        full = R.cheapest(g, vid[:1])
        assert full["rounds"] == 300 and full["cells_lowered"] == 299
        got = check(gg, csr, w, g, vid[:1], -1, None, full)
        assert got[3].tolist() == list(range(300)) and int(got[2][-1]) == int(wt.sum())
        cut = R.cheapest(g, vid[:1], 150)
        assert cut["rounds"] == 150 and len(cut["rows"][2]) == 151
        check(gg, csr, w, g, vid[:1], 150, None, cut)
    finally:
        w.close()
        csr.close()


def test_unit_weights_give_the_bfs_distances_of_an_independent_kernel(gg, hard):
    vid, src, dst, _, g, S, _ = hard
    csr = build(gg, vid, src, dst)
    w = gg.edge_weights(csr, np.ones(src.size, np.int64))
    try:
        for max_hops in (-1, 3):
            dist, _ = gg.bfs64(csr, S, max_hops if max_hops >= 0 else 1 << 20)
            res = gg.cheapest64(csr, w, S, max_hops)
            idx, ids, cost, hops = res.fetch()
            res.close()
            lane, v = np.nonzero(dist >= 0)  # unreached cells have no row; the rest in (lane, dense index) order
            assert lane.size > 1000
            assert np.array_equal(idx, lane) and np.array_equal(ids, g.vid[v])
            assert np.array_equal(cost, dist[lane, v]) and np.array_equal(hops, dist[lane, v])
    finally:
        w.close()
        csr.close()


def test_degenerate_inputs(gg, small):
    vid, src, dst, wt, g, hub, _ = small
    csr = build(gg, vid, src, dst)
    w = gg.edge_weights(csr, wt)
    try:
        got = check(gg, csr, w, g, np.array([-5, -6, -123456789], np.int64))  # no vertex among the sources: one idle round
        assert got[0].size == 0
        empty = gg.cheapest_path_lengths(csr, w, np.empty(0, np.int64))  # an empty list: no batch
        assert empty.rows() == 0 and empty.fetch()[0].size == 0 and empty.stats["rounds"] == 0
        empty.close()
    finally:
        w.close()
        csr.close()
    none = np.empty(0, np.int64)
    bare = build(gg, vid[:40], none, none)  # a graph without edges: no round runs, the sources are their own rows
    try:
        for by in ("rowid", "entry"):
            w = gg.edge_weights(bare, none, by=by)
            got = check(gg, bare, w, R.WeightedGraph(vid[:40], none, none, []), np.concatenate([vid[:5], vid[:1], [-5]]))
            assert rows_of(got) == [(i, int(v), 0, 0) for i, v in enumerate(vid[:5].tolist() + vid[:1].tolist())]
            w.close()
    finally:
        bare.close()
    one = np.array([42], np.int64)
    loop = build(gg, one, one, one)  # V = 1 with a self-loop: it never lowers anything
    try:
        w = gg.edge_weights(loop, np.array([0], np.int64))
        got = check(gg, loop, w, R.WeightedGraph(one, one, one, [0]), np.array([42, 42, 7], np.int64))
        assert rows_of(got) == [(0, 42, 0, 0), (1, 42, 0, 0)]
        w.close()
    finally:
        loop.close()


def test_the_four_weight_forms_give_identical_rows(gg, small):
    vid, src, dst, wt, g, hub, _ = small
    assert g.E < src.size  # dangling rows: their weights are never read (here: negative, which a read would refuse)
    dangling = np.ones(src.size, bool)
    dangling[g.kept] = False
    given = wt.copy()
    given[dangling] = -5
    S = np.concatenate([g.vid[[hub]], g.vid[:30]])
    want = R.cheapest(g, S)
    rng = np.random.RandomState(5)
    # implicit rowids
    csr = build(gg, vid, src, dst)
    try:
        w = gg.edge_weights(csr, given)
        check(gg, csr, w, g, S, -1, None, want)
        w.close()
        eid = csr.export()[2]
        w = gg.edge_weights(csr, given[eid], by="entry")  # in the order csr.export() shows
        assert np.array_equal(given[eid], g.entry_weights())
        check(gg, csr, w, g, S, -1, None, want)
        w.close()
    finally:
        csr.close()
    # explicit rowids in shuffled order: weights[rowid]
    rowid = rng.permutation(src.size).astype(np.int64) + 3
    by_rowid = np.full(src.size + 3, -9, np.int64)
    by_rowid[rowid] = given
    by_rowid[:3] = -9  # rowids nobody has
    csr = build(gg, vid, src, dst, rowid)
    try:
        w = gg.edge_weights(csr, by_rowid)
        check(gg, csr, w, g, S, -1, None, want)
        w.close()
    finally:
        csr.close()
    # by entry on a rowid-free build
    gg.set_edge_rowid(False)
    csr = build(gg, vid, src, dst)
    try:
        w = gg.edge_weights(csr, g.entry_weights(), by="entry")
        check(gg, csr, w, g, S, -1, None, want)
        w.close()
        with pytest.raises(GGError) as e:
            gg.edge_weights(csr, given)  # by rowid on a rowid-free CSR
        assert e.value.code == GG_ERR_STATE
    finally:
        csr.close()


def test_the_legacy_build(gg, small):
    vid, src, dst, wt, g, hub, _ = small
    S = np.concatenate([g.vid[[hub]], g.vid[:30]])
    gg.force_legacy_build(True)
    csr = build(gg, vid, src, dst)
    w = gg.edge_weights(csr, wt)
    try:
        for long_row in (0, 8):
            gg.debug_cheapest(long_row, 0)
            check(gg, csr, w, g, S)
    finally:
        w.close()
        csr.close()


def test_a_fully_mirrored_table_whose_reverse_rows_are_derived(gg):
    vid, src, dst = LT.table("a_packed")
    wt = R.hashed_weights(src.size)
    g = R.WeightedGraph(vid, src, dst, wt)
    gg.set_edge_rowid(False)  # the vertex-sorted form of the bucketed build is the one that derives
    gg.rank_mode(1)
    csr = build(gg, vid, src, dst)
    try:
        assert csr.reverse_derived == 1 and not csr.reverse_rows_ready  # the rows are rotated on first use
        w = gg.edge_weights(csr, g.entry_weights(), by="entry")
        try:
            S = np.concatenate([vid[[7, 2, 7]], [-5], vid[100:120]])
            want = R.cheapest(g, S)
            for long_row in (0, 1, NO_LONG_ROWS):
                gg.debug_cheapest(long_row, 0)
                check(gg, csr, w, g, S, -1, None, want)
        finally:
            w.close()
    finally:
        csr.close()


@pytest.mark.parametrize("kind", EI.PLACEMENTS)
def test_edge_case_vertex_ids(gg, kind):
    eg = EI.edge_graph(kind)
    wt = R.hashed_weights(eg.src.size)
    g = R.WeightedGraph(eg.vid, eg.src, eg.dst, wt)
    S = np.concatenate([np.asarray(eg.named, np.int64), np.asarray(eg.wired, np.int64)[:20], [eg.hub], EI.LISTED])[:64]
    csr = build(gg, eg.vid, eg.src, eg.dst)
    w = gg.edge_weights(csr, wt)
    try:
        got = check(gg, csr, w, g, S)
        assert set(np.asarray(eg.named).tolist()) <= set(got[1].tolist())
        check(gg, csr, w, g, S, 2, np.concatenate([np.asarray(eg.named, np.int64), EI.LISTED]))
    finally:
        w.close()
        csr.close()


def test_errors_leave_the_context_usable(gg, small):
    vid, src, dst, wt, g, hub, _ = small
    gg.staging_clear()
    gg.append_vertices(vid)
    gg.append_edges(src, dst)
    shard = gg.build_csr_shard(0, 2)
    csr = gg.build_csr()
    twin = gg.build_csr()  # the same graph, another CSR
    other = type(gg)(0)
    i64p, i32p = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    S = np.ascontiguousarray(g.vid[:4])
    sp = S.ctypes.data_as(i64p)
    wp = np.ascontiguousarray(wt).ctypes.data_as(i64p)
    want = R.cheapest(g, S, 2)
    w = gg.edge_weights(csr, wt)
    w_twin = gg.edge_weights(twin, wt)

    def make(ctx, graph, weights, n, by=0, out=True):
        h = C.c_void_p(1)
        rc = gg.lib.gg_edge_weights_create(ctx, graph, weights, n, by, C.byref(h) if out else None)
        assert rc != 0 and (not out or not h.value)
        return rc

    def call(ctx, graph, weights, srcs, n_src, dst=None, n_dst=0, stats=True, out=True):
        st, o = CheapestStats(), C.c_void_p(1)
        rc = gg.lib.gg_cheapest64(ctx, graph, weights, srcs, n_src, -1, dst, n_dst, C.byref(st) if stats else None,
                                  C.byref(o) if out else None)
        assert rc != 0 and (not out or not o.value)
        return rc

    negative = wt.copy()
    negative[g.kept[17]] = -1
    np_ = np.ascontiguousarray(negative).ctypes.data_as(i64p)
    try:
        bad = [
            lambda: (make(gg.ctx, csr.handle, np_, wt.size), GG_ERR_INVALID_ARG),  # a negative weight
            lambda: (make(gg.ctx, csr.handle, wp, wt.size, 1), GG_ERR_INVALID_ARG),  # by entry: n_weights != E
            lambda: (make(gg.ctx, csr.handle, wp, g.kept[-1]), GG_ERR_INVALID_ARG),  # by rowid: the last kept rowid outside
            lambda: (make(gg.ctx, csr.handle, wp, 0), GG_ERR_INVALID_ARG),
            lambda: (make(gg.ctx, csr.handle, None, wt.size), GG_ERR_INVALID_ARG),
            lambda: (make(gg.ctx, csr.handle, wp, wt.size, 2), GG_ERR_INVALID_ARG),
            lambda: (make(gg.ctx, csr.handle, wp, wt.size, 0, out=False), GG_ERR_INVALID_ARG),
            lambda: (make(None, csr.handle, wp, wt.size), GG_ERR_INVALID_ARG),
            lambda: (make(gg.ctx, None, wp, wt.size), GG_ERR_INVALID_ARG),
            lambda: (make(other.ctx, csr.handle, wp, wt.size), GG_ERR_INVALID_ARG),  # a CSR of another context
            lambda: (make(gg.ctx, shard.handle, wp, wt.size), GG_ERR_STATE),
            lambda: (call(None, csr.handle, w.handle, sp, 4), GG_ERR_INVALID_ARG),
            lambda: (call(gg.ctx, None, w.handle, sp, 4), GG_ERR_INVALID_ARG),
            lambda: (call(gg.ctx, csr.handle, None, sp, 4), GG_ERR_INVALID_ARG),
            lambda: (call(gg.ctx, csr.handle, w.handle, None, 4), GG_ERR_INVALID_ARG),
            lambda: (call(gg.ctx, csr.handle, w_twin.handle, sp, 4), GG_ERR_INVALID_ARG),  # weights of another CSR
            lambda: (call(other.ctx, csr.handle, w.handle, sp, 4), GG_ERR_INVALID_ARG),
            lambda: (call(gg.ctx, shard.handle, w.handle, sp, 4), GG_ERR_STATE),
            lambda: (call(gg.ctx, csr.handle, w.handle, sp, 0), GG_ERR_INVALID_ARG),
            lambda: (call(gg.ctx, csr.handle, w.handle, sp, 65), GG_ERR_INVALID_ARG),
            lambda: (call(gg.ctx, csr.handle, w.handle, sp, 4, None, 3), GG_ERR_INVALID_ARG),  # targets without a list
            lambda: (call(gg.ctx, csr.handle, w.handle, sp, 4, stats=False, out=False), GG_ERR_INVALID_ARG),
            lambda: (gg.lib.gg_debug_cheapest(gg.ctx, 0, 2), GG_ERR_INVALID_ARG),
            lambda: (gg.lib.gg_debug_cheapest(gg.ctx, 0, -1), GG_ERR_INVALID_ARG),
            lambda: (gg.lib.gg_debug_cheapest(None, 0, 0), GG_ERR_INVALID_ARG),
        ]
        for i, case in enumerate(bad):
            rc, code = case()
            assert rc == code, (i, rc, code)
            check(gg, csr, w, g, S, 2, None, want)  # a correct call still works
        check(gg, twin, w_twin, g, S, 2, None, want)
        # the result answers its own two calls only, and they answer no other result
        res = gg.cheapest64(csr, w, S, 2)
        agg = gg.khop_aggregate(csr, 1, 2, "end", S)
        table = gg.expand_khop_result(csr, 1, S)
        pairs = gg.khop_pair_counts(csr, 1, 1, S)
        try:
            handle = res.parts[0][0]
            n, got, levels = C.c_uint64(), C.c_uint32(), C.c_int()
            buf = np.empty((4, 8), np.int64)
            h32 = np.empty(8, np.int32)
            u64p = C.POINTER(C.c_uint64)
            ptrs = (i64p * 3)(*[buf[c].ctypes.data_as(i64p) for c in range(3)])
            lib = gg.lib
            assert lib.gg_result_rows(handle, 1, C.byref(n)) == GG_ERR_STATE
            assert lib.gg_result_fetch(handle, 1, 0, 8, ptrs, C.byref(got)) == GG_ERR_STATE
            assert lib.gg_result_fetch_edges(handle, 1, 0, 8, ptrs, C.byref(got)) == GG_ERR_STATE
            assert lib.gg_walk_closure_levels(handle, None, 0, C.byref(levels)) == GG_ERR_STATE
            assert lib.gg_reach_closure_levels(handle, None, 0, C.byref(levels)) == GG_ERR_STATE
            assert lib.gg_level_sets_levels(handle, None, 0, C.byref(levels)) == GG_ERR_STATE
            assert lib.gg_bfs64_paths_rows(handle, C.byref(n)) == GG_ERR_STATE
            assert lib.gg_khop_aggregate_rows(handle, 1, C.byref(n)) == GG_ERR_STATE
            assert lib.gg_khop_pair_counts_rows(handle, 1, C.byref(n)) == GG_ERR_STATE
            assert lib.gg_components_rows(handle, 0, C.byref(n)) == GG_ERR_STATE
            assert lib.gg_bfs64_all_paths_rows(handle, 0, C.byref(n)) == GG_ERR_STATE
            for h in (table.handle, agg.handle, pairs.parts[0][0]):
                assert lib.gg_cheapest64_rows(h, C.byref(n)) == GG_ERR_STATE
                assert lib.gg_cheapest64_fetch(h, 0, 8, buf[0].ctypes.data_as(i64p), None, None, None,
                                               C.byref(got)) == GG_ERR_STATE
            assert lib.gg_cheapest64_rows(None, C.byref(n)) == GG_ERR_INVALID_ARG
            # the fetch's conventions: any output may be NULL, nothing past the end
            total = res.rows()
            assert total > 8
            assert lib.gg_cheapest64_fetch(handle, total - 3, 8, None, buf[1].ctypes.data_as(i64p), None,
                                           h32.ctypes.data_as(i32p), C.byref(got)) == 0 and got.value == 3
            assert buf[1][:3].tolist() == want["rows"][1][-3:].tolist() and h32[:3].tolist() == want["rows"][3][-3:]
            assert lib.gg_cheapest64_fetch(handle, 0, 8, None, None, None, None, C.byref(got)) == 0 and got.value == 8
            assert lib.gg_cheapest64_fetch(handle, total, 8, None, None, buf[2].ctypes.data_as(i64p), None,
                                           C.byref(got)) == 0 and got.value == 0
            assert R.same(res.fetch(), want["rows"])
        finally:
            pairs.close()
            table.close()
            agg.close()
            res.close()
    finally:
        w_twin.close()
        w.close()
        other.close()
        shard.close()
        twin.close()
        csr.close()
