"""GG.cheapest64_paths / GG.cheapest_paths (gg_cheapest64_paths) against the restatement in python integers
(tests/cheapest_paths_ref.py): the path rows and the pair table row for row and in order, and every stats field — on hand
graphs that pin which of the cheapest paths is returned, at the saturation point, on in-rows around the lane group with
the only qualifying entry last, on a graph of many ties and zero weights under every knob, on a chain, on vertex and lane
counts around the wavefront, on every build form and id placement, and through the errors.  One cross-check of an
independent kernel: with unit weights the rows are gg_bfs64_paths' rows.

Not covered here: both GG_ERR_TOO_LARGE cases need 2^32 pairs or path rows."""
import ctypes as C

import numpy as np
import pytest

from duckdb_pgq_amd import GGError
from duckdb_pgq_amd.gg import CheapestPathsStats
from tests import cheapest_paths_ref as PR
from tests import cheapest_ref as R
from tests import edge_ids as EI
from tests import lazy_reverse_tables as LT
from tests import triangles_ref as T

pytestmark = pytest.mark.gpu

GG_ERR_INVALID_ARG, GG_ERR_STATE = -1, -6
INT64_MAX = R.INT64_MAX
LANES = 16  # GG_CPP_LANES, the lanes of a pair's group (gg_cheapest.hip); the counts asserted below hold for any value
COUNTS = ("pairs_reached", "pairs_saturated", "entries_scanned")


def build(gg, vid, src, dst, rowid=None):
    gg.staging_clear()
    gg.append_vertices(np.asarray(vid, np.int64))
    gg.append_edges(np.asarray(src, np.int64), np.asarray(dst, np.int64), rowid)
    return gg.build_csr()


def all_pairs(S, vid):
    return np.repeat(np.arange(len(S), dtype=np.uint32), len(vid)), np.tile(np.asarray(vid, np.int64), len(S))


def check(gg, csr, w, g, S, lanes, targets, rowid=None, edges=True, want=None, gather_all=False):
    """one call against the restatement (want: its answer where the caller has it); returns (rows, pairs, stats)"""
    want = want or PR.paths(g, S, lanes, targets, rowid, edges)
    rows, pairs, st = gg.cheapest64_paths(csr, w, S, lanes, targets, edges)
    print("rows", rows[0].size, want["n_rows"], {k: (st[k], want[k]) for k in COUNTS}, st["search"], want["search"])
    assert PR.same_rows(rows, want["rows"])
    assert PR.same_rows(pairs, want["pairs"])
    assert [a.dtype for a in rows] == [np.int64, np.int32, np.int64, np.int64, np.int64]
    assert [a.dtype for a in pairs] == [np.int64, np.int64, np.int32, np.int32]
    assert st["rows"] == want["n_rows"]
    for k in COUNTS:
        assert st[k] == want[k], k
    for k, v in want["search"].items():  # the rounds, as gg_cheapest64(max_hops = -1) reports them
        assert st["search"][k] == (want["search"]["entries_pulled"] if gather_all and k == "rows_gathered" else v), k
    return rows, pairs, st


def tuples(rows):
    return list(zip(*[[int(x) for x in col] for col in rows]))


def run_hand(gg, edges, S, lanes, targets, vid=(1, 2, 3, 4, 5, 6), rowid=None):
    vid = np.array(vid, np.int64)
    src, dst, wt = (np.array(x, np.int64) for x in zip(*edges))
    rowid = None if rowid is None else np.array(rowid, np.int64)
    g = R.WeightedGraph(vid, src, dst, wt)
    csr = build(gg, vid, src, dst, rowid)
    w = gg.edge_weights(csr, wt if rowid is None else _by_rowid(wt, rowid))
    try:
        rows, pairs, st = check(gg, csr, w, g, np.array(S, np.int64), np.array(lanes, np.uint32),
                                np.array(targets, np.int64), rowid)
        return tuples(rows), tuples(pairs), st
    finally:
        w.close()
        csr.close()


def _by_rowid(wt, rowid):
    out = np.zeros(int(rowid.max()) + 1, np.int64)
    out[rowid] = wt
    return out


# ---- hand graphs: which path is pinned


def test_a_zero_weight_cycle_on_the_way_ends(gg):
    edges = [(1, 2, 5), (2, 3, 0), (3, 2, 0), (3, 4, 1), (4, 3, 0)]
    rows, pairs, _ = run_hand(gg, edges, [1], [0], [4])
    assert rows == [(0, 0, 1, -1, 0), (0, 1, 2, 0, 5), (0, 2, 3, 1, 5), (0, 3, 4, 3, 6)]
    assert pairs == [(0, 6, 3, 1)]


def test_of_two_equal_predecessors_the_smaller_vertex_table_position_wins(gg):
    edges = [(1, 2, 1), (1, 3, 1), (3, 4, 1), (2, 4, 1)]
    rows, _, _ = run_hand(gg, edges, [1], [0], [4], vid=(1, 2, 3, 4))
    assert [r[2] for r in rows] == [1, 2, 4] and rows[2][3] == 3  # 2 stands before 3 in the vertex table
    rows, _, _ = run_hand(gg, edges, [1], [0], [4], vid=(1, 3, 2, 4))
    assert [r[2] for r in rows] == [1, 3, 4] and rows[2][3] == 2  # now 3 does, whatever the ids say


def test_a_predecessor_of_equal_cost_but_more_hops_is_not_taken(gg):
    # 5 costs 3 in 2 hops through 2; 4 also offers 2 + 1 = 3 but lies 2 hops out, and stands first in the vertex table
    edges = [(1, 2, 2), (1, 3, 1), (3, 4, 1), (4, 5, 1), (2, 5, 1)]
    rows, pairs, st = run_hand(gg, edges, [1], [0, 0], [5, 4], vid=(1, 4, 2, 3, 5))
    assert rows[:3] == [(0, 0, 1, -1, 0), (0, 1, 2, 0, 2), (0, 2, 5, 4, 3)]
    assert pairs == [(0, 3, 2, 1), (1, 2, 2, 1)]
    assert st["entries_scanned"] == (2 + 1) + (1 + 1)  # 5's in-row: 4 is looked at and passed over


def test_parallel_rows_the_qualifying_one_and_among_equals_the_first_appended(gg):
    rows, _, _ = run_hand(gg, [(1, 2, 7), (1, 2, 4), (1, 2, 9)], [1], [0], [2])
    assert rows == [(0, 0, 1, -1, 0), (0, 1, 2, 1, 4)]
    # equal weights: the row appended first, reported by the rowid it was given (50, not the smaller 40)
    rows, _, st = run_hand(gg, [(1, 2, 9), (1, 2, 4), (1, 2, 4)], [1], [0], [2], rowid=[7, 50, 40])
    assert rows == [(0, 0, 1, -1, 0), (0, 1, 2, 50, 4)] and st["entries_scanned"] == 2


def test_self_loops_the_source_itself_unreached_targets_and_ids_that_are_no_vertices(gg):
    edges = [(1, 1, 3), (1, 2, 4), (2, 2, 0), (2, 3, 0), (3, 3, 0), (5, 4, 1)]
    S = [1, 77, 1, 3]  # lane 1 is no vertex; lanes 0 and 2 carry one source
    lanes = [0, 0, 0, 0, 1, 0, 2, 0, 3, 3]
    targets = [1, 3, 4, 99, 2, 3, 3, 1, 3, 1]  # s == t; 2 hops; unreached; no vertex; from no vertex; a duplicate; lane 2 ...
    rows, pairs, st = run_hand(gg, edges, S, lanes, targets)
    path = [(0, 1, -1, 0), (1, 2, 1, 4), (2, 3, 3, 4)]
    want = [(0, 0, 1, -1, 0)] + [(p,) + r for p in (1, 5, 6) for r in path] + [(7, 0, 1, -1, 0), (8, 0, 3, -1, 0)]
    assert rows == want
    assert pairs == [(0, 0, 0, 1), (1, 4, 2, 1), (5, 4, 2, 1), (6, 4, 2, 1), (7, 0, 0, 1), (8, 0, 0, 1)]
    assert st["pairs_reached"] == 6 and st["rows"] == 12


def test_the_counter_example_graph_at_its_fixpoint(gg):
    edges = [(0, 3, 10), (0, 1, 1), (1, 2, 1), (2, 3, 1), (3, 4, 1)]
    rows, pairs, st = run_hand(gg, edges, [0], [0, 0], [4, 3], vid=(0, 1, 2, 3, 4))
    assert rows[:5] == [(0, 0, 0, -1, 0), (0, 1, 1, 1, 1), (0, 2, 2, 2, 2), (0, 3, 3, 3, 3), (0, 4, 4, 4, 4)]
    assert pairs == [(0, 4, 4, 1), (1, 3, 3, 1)] and st["entries_scanned"] == 5 + 4


def test_a_saturated_pair_is_listed_and_never_traced(gg):
    edges = [(1, 2, INT64_MAX - 1), (2, 3, 5)]
    rows, pairs, st = run_hand(gg, edges, [1], [0, 0], [3, 2], vid=(1, 2, 3))
    assert pairs == [(0, INT64_MAX, 2, 0), (1, INT64_MAX - 1, 1, 1)]
    assert rows == [(1, 0, 1, -1, 0), (1, 1, 2, 0, INT64_MAX - 1)]
    assert st["pairs_saturated"] == 1 and st["pairs_reached"] == 2 and st["rows"] == 2


# ---- in-rows around the lane group


def test_in_rows_around_the_lane_group_with_the_only_qualifying_entry_last(gg):
    """centre k has in-degree d_k: d_k - 1 leaves, half of them reached at the wrong cost and half not at all, and q,
    which stands behind every leaf in the vertex table and is the one predecessor"""
    degs = [LANES - 1, LANES, LANES + 1, 2 * LANES + 1, 63, 64, 65, 129, 130]
    n = max(degs) - 1
    s, q = 5, 6
    leaves = np.arange(1000, 1000 + n, dtype=np.int64)
    centres = np.arange(10, 10 + len(degs), dtype=np.int64)
    vid = np.concatenate([[s], leaves, [q], centres])
    half = leaves[::2]  # s -> every second leaf at 5: such a leaf offers 5 + 1, not 2; the others offer nothing
    src, dst, wt = [np.array([s]), np.full(half.size, s)], [np.array([q]), half], [np.array([1]), np.full(half.size, 5)]
    for k, d in enumerate(degs):
        src += [leaves[:d - 1], np.array([q])]
        dst += [np.full(d - 1, centres[k]), centres[k:k + 1]]
        wt += [np.ones(d - 1, np.int64), np.array([1])]
    src, dst, wt = np.concatenate(src), np.concatenate(dst), np.concatenate(wt).astype(np.int64)
    g = R.WeightedGraph(vid, src, dst, wt)
    assert np.bincount(np.asarray(g.dv), minlength=g.V)[-len(degs):].tolist() == degs
    csr = build(gg, vid, src, dst)
    w = gg.edge_weights(csr, wt)
    try:
        for k, d in enumerate(degs):
            rows, pairs, st = check(gg, csr, w, g, [s], [0], centres[k:k + 1])
            assert rows[2].tolist() == [s, q, centres[k]] and tuples(pairs) == [(0, 2, 2, 1)]
            assert st["entries_scanned"] == d + 1  # the whole in-row of the centre, then q's one entry
        _, _, st = check(gg, csr, w, g, [s, s], *all_pairs([s, s], vid))
        assert st["entries_scanned"] == 2 * (sum(degs) + len(degs) + 1 + half.size)
    finally:
        w.close()
        csr.close()


# ---- many ties and zeros, every knob


@pytest.fixture(scope="module")
def small():
    """tests/test_gpu_cheapest.py's small graph with weights hashed into 0..3; 64 sources = [the hub twice, an id that is
    no vertex, the negative id, 60 others] x every vertex, and the restatement's answer (computed once, never changed)"""
    vid, src, dst = T.hard_graph(V=300, rows=3000, seed=0x51, hub_fan=120)
    wt = R.hashed_weights(src.size, 0, 3)
    g = R.WeightedGraph(vid, src, dst, wt)
    indeg = np.bincount(np.asarray(g.dv), minlength=g.V)
    hub = int(indeg.argmax())
    assert indeg[hub] >= 100 and -77 in g.index
    head = [int(g.vid[hub]), int(g.vid[hub]), -123456789, -77]
    S = np.array(head + [int(x) for x in g.vid.tolist() if int(x) not in head][:60], np.int64)
    lanes, targets = all_pairs(S, vid)
    assert lanes.size == 19_200
    return vid, src, dst, wt, g, S, lanes, targets, PR.paths(g, S, lanes, targets)


def test_every_vertex_from_64_sources_under_every_knob(gg, small):
    vid, src, dst, wt, g, S, lanes, targets, want = small
    csr = build(gg, vid, src, dst)
    w = gg.edge_weights(csr, wt)
    try:
        rows, pairs, st = check(gg, csr, w, g, S, lanes, targets, want=want)
        assert st["rows"] > 50_000 and st["pairs_saturated"] == 0
        assert not (pairs[0] // 300 == 2).any()  # a source that is no vertex reaches nothing
        again = check(gg, csr, w, g, S, lanes, targets, want=want)  # the same call: the same bits
        assert all(np.array_equal(a, b) for a, b in zip(rows + pairs, again[0] + again[1])) and again[2] == st
        gg.debug_cheapest(1, 0)  # every in-row is a long one for the rounds
        check(gg, csr, w, g, S, lanes, targets, want=want)
        gg.debug_cheapest(0, 1)
        check(gg, csr, w, g, S, lanes, targets, want=want, gather_all=True)
        gg.debug_cheapest(0, 0)
        gg.max_grid_tiles(3)
        check(gg, csr, w, g, S, lanes, targets, want=want)
        gg.max_grid_tiles(0)
        plain, plain_pairs, plain_st = gg.cheapest64_paths(csr, w, S, lanes, targets, edges=False)
        assert np.all(plain[3] == -1) and (rows[3] != -1).any()
        assert all(np.array_equal(plain[c], rows[c]) for c in (0, 1, 2, 4))
        assert all(np.array_equal(a, b) for a, b in zip(plain_pairs, pairs)) and plain_st == st
    finally:
        w.close()
        csr.close()


def test_any_number_of_pairs_in_batches_of_64_sources(gg, small):
    vid, src, dst, wt, g, _, _, _, _ = small
    rng = np.random.RandomState(9)
    s = np.concatenate([g.vid[rng.randint(0, 90, 400)], [-5, int(g.vid[3])]])  # up to 91 distinct sources: two batches
    d = np.concatenate([g.vid[rng.randint(0, g.V, 400)], [int(g.vid[0]), -6]])
    assert np.unique(s).size > 64
    want = PR.pair_paths(g, s, d)
    csr = build(gg, vid, src, dst)
    w = gg.edge_weights(csr, wt)
    try:
        assert PR.same_rows(gg.cheapest_paths(csr, w, s, d), want["rows"])
        none = np.empty(0, np.int64)
        assert [c.size for c in gg.cheapest_paths(csr, w, none, none)] == [0] * 5
    finally:
        w.close()
        csr.close()


# ---- other shapes


def test_a_chain_of_300_is_one_path_of_300_rows(gg):
    vid = np.arange(300, dtype=np.int64) * 3 + 1
    src, dst = vid[:-1], vid[1:]
    wt = R.hashed_weights(src.size, 0, 9)
    g = R.WeightedGraph(vid, src, dst, wt)
    csr = build(gg, vid, src, dst)
    w = gg.edge_weights(csr, wt)
    try:
        rows, pairs, st = check(gg, csr, w, g, vid[:1], [0, 0], [vid[-1], vid[150]])
        assert rows[1][:300].tolist() == list(range(300)) and rows[2][:300].tolist() == vid.tolist()
        assert rows[3][1:300].tolist() == list(range(299)) and rows[4][:300].tolist() == [0] + np.cumsum(wt).tolist()
        assert st["rows"] == 300 + 151 and st["entries_scanned"] == 299 + 150
    finally:
        w.close()
        csr.close()


@pytest.mark.parametrize("V", [63, 64, 65, 129])
def test_vertex_counts_around_the_tile(gg, V):
    rng = np.random.RandomState(V)
    vid = (np.arange(V, dtype=np.int64) * 7 + 3)[rng.permutation(V)]
    chords = rng.randint(0, V, size=(2, 3 * V))
    src = np.concatenate([vid, vid[chords[0]]])
    dst = np.concatenate([np.roll(vid, -1), vid[chords[1]]])
    wt = R.hashed_weights(src.size, 0, 5)
    g = R.WeightedGraph(vid, src, dst, wt)
    csr = build(gg, vid, src, dst)
    w = gg.edge_weights(csr, wt)
    try:
        S = vid[:64]
        check(gg, csr, w, g, S, *all_pairs(S, vid))
    finally:
        w.close()
        csr.close()


@pytest.mark.parametrize("n", [1, 63, 64])
def test_lane_counts(gg, small, n):
    vid, src, dst, wt, g, S, _, _, _ = small
    csr = build(gg, vid, src, dst)
    w = gg.edge_weights(csr, wt)
    try:
        lanes, targets = all_pairs(S[:n], vid[:40])
        check(gg, csr, w, g, S[:n], lanes, targets)
    finally:
        w.close()
        csr.close()


def test_unit_weights_give_the_rows_of_the_bfs_trace_an_independent_kernel(gg, small):
    vid, src, dst, _, g, S, lanes, targets, _ = small
    csr = build(gg, vid, src, dst)
    w = gg.edge_weights(csr, np.ones(src.size, np.int64))
    try:
        (pair, step, vtx, edge), _ = gg.bfs64_paths(csr, S, lanes, targets)
        rows, pairs, st = gg.cheapest64_paths(csr, w, S, lanes, targets)
        assert pair.size > 50_000
        assert all(np.array_equal(a, b) for a, b in zip((pair, step, vtx, edge), rows[:4]))  # the pin rules coincide
        assert np.array_equal(rows[4], step)  # and the cost of a step is its number
        assert np.array_equal(pairs[1], pairs[2]) and np.all(pairs[3] == 1)
    finally:
        w.close()
        csr.close()


# ---- build forms and ids


def test_the_legacy_build(gg, small):
    vid, src, dst, wt, g, S, lanes, targets, want = small
    gg.force_legacy_build(True)
    csr = build(gg, vid, src, dst)
    w = gg.edge_weights(csr, wt)
    try:
        check(gg, csr, w, g, S, lanes, targets, want=want)
    finally:
        w.close()
        csr.close()


def test_a_fully_mirrored_table_whose_reverse_rows_are_derived(gg):
    vid, src, dst = LT.table("a_packed")
    wt = R.hashed_weights(src.size, 0, 3)
    g = R.WeightedGraph(vid, src, dst, wt)
    gg.set_edge_rowid(False)  # the vertex-sorted form of the bucketed build is the one that derives
    gg.rank_mode(1)
    csr = build(gg, vid, src, dst)
    try:
        assert csr.reverse_derived == 1 and not csr.reverse_rows_ready  # the rows are rotated on first use
        w = gg.edge_weights(csr, g.entry_weights(), by="entry")
        try:
            S = np.concatenate([vid[[7, 2, 7]], [-5], vid[100:120]])
            check(gg, csr, w, g, S, *all_pairs(S, vid), edges=False)
        finally:
            w.close()
    finally:
        csr.close()


@pytest.mark.parametrize("kind", EI.PLACEMENTS)
def test_edge_case_vertex_ids(gg, kind):
    eg = EI.edge_graph(kind)
    wt = R.hashed_weights(eg.src.size, 0, 3)
    g = R.WeightedGraph(eg.vid, eg.src, eg.dst, wt)
    s, d = EI.path_pairs(eg)
    want = PR.pair_paths(g, s, d)
    csr = build(gg, eg.vid, eg.src, eg.dst)
    w = gg.edge_weights(csr, wt)
    try:
        got = gg.cheapest_paths(csr, w, s, d)
        assert PR.same_rows(got, want["rows"])
        assert set(np.asarray(eg.named)[:4].tolist()) <= set(got[2].tolist())
    finally:
        w.close()
        csr.close()


def test_weights_by_entry_on_a_csr_without_rowids(gg, small):
    vid, src, dst, wt, g, S, lanes, targets, want = small
    gg.set_edge_rowid(False)
    csr = build(gg, vid, src, dst)
    w = gg.edge_weights(csr, g.entry_weights(), by="entry")
    try:
        with pytest.raises(GGError) as e:
            gg.cheapest64_paths(csr, w, S, lanes, targets, edges=True)
        assert e.value.code == GG_ERR_STATE
        rows, pairs, _ = gg.cheapest64_paths(csr, w, S, lanes, targets, edges=False)
        assert np.all(rows[3] == -1) and all(PR.same_rows([rows[c]], [want["rows"][c]]) for c in (0, 1, 2, 4))
        assert PR.same_rows(pairs, want["pairs"])
    finally:
        w.close()
        csr.close()


# ---- result kinds and errors


def test_result_kinds_and_errors_leave_the_context_usable(gg, small):
    vid, src, dst, wt, g, S, _, _, _ = small
    gg.staging_clear()
    gg.append_vertices(vid)
    gg.append_edges(src, dst)
    shard = gg.build_csr_shard(0, 2)
    csr = gg.build_csr()
    twin = gg.build_csr()  # the same graph, another CSR
    i64p, i32p, u32p, u64p = (C.POINTER(t) for t in (C.c_int64, C.c_int32, C.c_uint32, C.c_uint64))
    S4 = np.ascontiguousarray(S[:4])
    lanes, targets = all_pairs(S4, vid[:50])
    targets = np.ascontiguousarray(targets)
    want = PR.paths(g, S4, lanes, targets)
    sp, lp, tp = S4.ctypes.data_as(i64p), lanes.ctypes.data_as(u32p), targets.ctypes.data_as(i64p)
    bad_lanes = lanes.copy()
    bad_lanes[-1] = 4  # names source 4 of 4
    w = gg.edge_weights(csr, wt)
    w_twin = gg.edge_weights(twin, wt)

    def call(ctx, graph, weights, srcs, n_src, lane=lp, dst=tp, n=lanes.size, out=True):
        st, o = CheapestPathsStats(), C.c_void_p(1)
        st.rows = 9
        rc = gg.lib.gg_cheapest64_paths(ctx, graph, weights, srcs, n_src, lane, dst, n, 1, C.byref(st),
                                        C.byref(o) if out else None)
        assert rc != 0 and (not out or not o.value) and st.rows == 0  # the outputs are cleared
        return rc

    try:
        bad = [
            lambda: (call(gg.ctx, csr.handle, w.handle, sp, 4, bad_lanes.ctypes.data_as(u32p)), GG_ERR_INVALID_ARG),
            lambda: (call(gg.ctx, csr.handle, w_twin.handle, sp, 4), GG_ERR_INVALID_ARG),  # weights of another CSR
            lambda: (call(gg.ctx, shard.handle, w.handle, sp, 4), GG_ERR_STATE),
            lambda: (call(gg.ctx, csr.handle, w.handle, sp, 0), GG_ERR_INVALID_ARG),
            lambda: (call(gg.ctx, csr.handle, w.handle, sp, 65), GG_ERR_INVALID_ARG),
            lambda: (call(gg.ctx, csr.handle, None, sp, 4), GG_ERR_INVALID_ARG),
            lambda: (call(gg.ctx, csr.handle, w.handle, None, 4), GG_ERR_INVALID_ARG),
            lambda: (call(gg.ctx, csr.handle, w.handle, sp, 4, None), GG_ERR_INVALID_ARG),  # pairs without their lanes
            lambda: (call(gg.ctx, csr.handle, w.handle, sp, 4, lp, None), GG_ERR_INVALID_ARG),
            lambda: (call(gg.ctx, csr.handle, w.handle, sp, 4, out=False), GG_ERR_INVALID_ARG),
        ]
        for i, case in enumerate(bad):
            rc, code = case()
            assert rc == code, (i, rc, code)
            check(gg, csr, w, g, S4, lanes, targets, want=want)  # a correct call still works
        check(gg, twin, w_twin, g, S4, lanes, targets, want=want)

        # the result answers its own three calls only, and they answer no other result
        st, res = CheapestPathsStats(), C.c_void_p()
        assert gg.lib.gg_cheapest64_paths(gg.ctx, csr.handle, w.handle, sp, 4, lp, tp, lanes.size, 1, C.byref(st),
                                          C.byref(res)) == 0
        costs = gg.cheapest64(csr, w, S4)
        try:
            lib, n, got = gg.lib, C.c_uint64(), C.c_uint32()
            buf = np.empty((5, 8), np.int64)
            b = [buf[c].ctypes.data_as(i64p) for c in range(5)]
            h32 = np.empty((2, 8), np.int32)
            h = [h32[c].ctypes.data_as(i32p) for c in range(2)]
            ptrs = (i64p * 3)(*b[:3])
            assert lib.gg_cheapest64_fetch(res, 0, 8, b[0], b[1], b[2], h[0], C.byref(got)) == GG_ERR_STATE
            assert lib.gg_cheapest64_rows(res, C.byref(n)) == GG_ERR_STATE
            assert lib.gg_bfs64_paths_fetch(res, 0, 8, b[0], h[0], b[1], b[2], C.byref(got)) == GG_ERR_STATE
            assert lib.gg_result_fetch(res, 1, 0, 8, ptrs, C.byref(got)) == GG_ERR_STATE
            assert lib.gg_components_fetch(res, 0, 8, b[0], b[1], buf[2].ctypes.data_as(u64p), C.byref(got)) == GG_ERR_STATE
            assert lib.gg_bfs64_all_paths_rows(res, 0, C.byref(n)) == GG_ERR_STATE
            other = costs.parts[0][0]  # a gg_cheapest64 result
            assert lib.gg_cheapest64_paths_rows(other, 0, C.byref(n)) == GG_ERR_STATE
            assert lib.gg_cheapest64_paths_fetch_pairs(other, 0, 8, b[0], b[1], h[0], h[1], C.byref(got)) == GG_ERR_STATE
            assert lib.gg_cheapest64_paths_fetch(other, 0, 8, b[0], h[0], b[1], b[2], b[3], C.byref(got)) == GG_ERR_STATE
            assert lib.gg_cheapest64_paths_rows(res, 2, C.byref(n)) == GG_ERR_INVALID_ARG  # no such table
            # the fetches' conventions: the nullable outputs, nothing past the end
            assert lib.gg_cheapest64_paths_rows(res, 1, C.byref(n)) == 0 and n.value == want["n_rows"] > 8
            total = n.value
            assert lib.gg_cheapest64_paths_fetch(res, total - 3, 8, b[0], h[0], b[1], None, None, C.byref(got)) == 0
            assert got.value == 3 and buf[1][:3].tolist() == want["rows"][2][-3:].tolist()
            assert lib.gg_cheapest64_paths_fetch(res, total - 3, 8, b[0], h[0], b[1], None, b[4], C.byref(got)) == 0
            assert buf[4][:3].tolist() == want["rows"][4][-3:]
            assert lib.gg_cheapest64_paths_fetch(res, total, 8, b[0], h[0], b[1], b[2], b[3], C.byref(got)) == 0
            assert got.value == 0
            assert lib.gg_cheapest64_paths_fetch(res, 0, 8, None, h[0], b[1], b[2], b[3], C.byref(got)) == GG_ERR_INVALID_ARG
            assert lib.gg_cheapest64_paths_rows(res, 0, C.byref(n)) == 0 and n.value == want["pairs_reached"] > 8
            assert lib.gg_cheapest64_paths_fetch_pairs(res, 2, 4, None, b[1], None, h[1], C.byref(got)) == 0
            assert got.value == 4 and buf[1][:4].tolist() == want["pairs"][1][2:6]
            assert h32[1][:4].tolist() == want["pairs"][3][2:6].tolist()
            assert lib.gg_cheapest64_paths_fetch_pairs(res, 0, 8, None, None, None, None, C.byref(got)) == 0
            assert got.value == 8
        finally:
            costs.close()
            gg.lib.gg_result_destroy(res)
    finally:
        w_twin.close()
        w.close()
        shard.close()
        twin.close()
        csr.close()
