"""gg_bfs64_all_paths / GG.all_shortest_paths / GG.shortest_path_counts against the Python restatement of the relation
(tests/all_shortest_paths_ref.py): both tables with their dtypes and every statistic, exactly — the number of shortest
paths saturates and their rank order is pinned, so nothing is compared up to a choice."""
import ctypes as C

import numpy as np
import pytest

from duckdb_pgq_amd import GGError, datagen
from tests import all_shortest_paths_ref as ref
from tests import deep_graphs
from tests.test_golden import NAMES, bfs_cases, load

pytestmark = pytest.mark.gpu

GG_ERR_INVALID_ARG, GG_ERR_TOO_LARGE, GG_ERR_STATE = -1, -5, -6
SAT = (1 << 64) - 1
T0_DTYPES = (np.int64, np.int32, np.uint64, np.uint64)
T1_DTYPES = (np.int64, np.int64, np.int32, np.int64, np.int64)


def build(gg, vid, src, dst, rowid=None):
    gg.staging_clear()
    gg.append_vertices(np.asarray(vid, np.int64))
    gg.append_edges(np.asarray(src, np.int64), np.asarray(dst, np.int64), rowid)
    return gg.build_csr()


def same_tables(got, want, dtypes, what):
    assert len(got) == len(want) == len(dtypes)
    for c, (g, w, t) in enumerate(zip(got, want, dtypes)):
        assert g.dtype == w.dtype == t, (what, c)
        assert np.array_equal(g, w), (what, c)


def check_batch(gg, csr, sources, lane, dst, max_hops=-1, path_limit=0, edges=True, materialise=True, arrays=None,
                batch=None):
    """one device batch against the restatement: table 0, table 1, the six counters and the BFS's statistics"""
    off, nbr, eid, vid = arrays or csr.export()
    want0, want1, want_st = ref.batch_tables(off, nbr, eid, vid, sources, lane, dst, max_hops, path_limit, edges, materialise,
                                             batch=batch)
    got0, got1, st = gg.bfs64_all_paths(csr, sources, lane, dst, max_hops, path_limit, edges, materialise)
    same_tables(got0, want0, T0_DTYPES, "pairs")
    if materialise:
        assert want1 is not None
        same_tables(got1, want1, T1_DTYPES, "rows")
    else:
        assert got1 is None
    bfs = st.pop("bfs")
    assert st == want_st
    assert bfs == gg.bfs64(csr, sources, max_hops, fetch=False)[1]
    return got0, got1, st


def check_pairs(gg, csr, s, t, max_hops=-1, path_limit=0, edges=True):
    """any number of pairs (GG.all_shortest_paths / GG.shortest_path_counts) against the restatement"""
    off, nbr, eid, vid = csr.export()
    want = ref.all_shortest_paths(off, nbr, eid, vid, s, t, max_hops, path_limit, edges)
    got = gg.all_shortest_paths(csr, s, t, max_hops, path_limit, edges)
    same_tables(got, want, T1_DTYPES, "rows")
    same_tables(gg.shortest_path_counts(csr, s, t, max_hops), ref.shortest_path_counts(off, nbr, vid, s, t, max_hops),
                (np.int64, np.int32, np.uint64), "counts")
    return got


def path_zero_is_the_pinned_path(gg, csr, s, t, max_hops, rows):
    """path 0 of every pair, and path_limit = 1, are exactly the rows of gg.shortest_paths"""
    one = gg.shortest_paths(csr, s, t, max_hops)
    first = rows[1] == 0
    for g, w in zip((rows[0][first], rows[2][first], rows[3][first], rows[4][first]), one):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    lim = gg.all_shortest_paths(csr, s, t, max_hops, path_limit=1)
    assert not lim[1].any()
    for g, w in zip((lim[0], lim[2], lim[3], lim[4]), one):
        assert g.dtype == w.dtype and np.array_equal(g, w)


def all_pairs(sources, vid):
    lane = np.repeat(np.arange(len(sources)), vid.size)
    return lane, np.tile(vid, len(sources))


@pytest.mark.parametrize("name", NAMES)
def test_goldens(gg, name):
    g = load(name)
    csr = build(gg, g["vid"], g["src"], g["dst"])
    arrays = csr.export()
    for sources, max_hops, rel in bfs_cases(g):
        lane_of = {int(s): i for i, s in enumerate(sources)}
        lane = np.array([lane_of[int(s)] for s in rel[:, 0]])
        batch = ref.make_batch(arrays[0], arrays[1], arrays[3], sources, max_hops)  # sigma once for both modes
        got0, got1, st = check_batch(gg, csr, sources, lane, rel[:, 1], max_hops, arrays=arrays, batch=batch)
        assert np.array_equal(got0[0], np.arange(rel.shape[0])) and np.array_equal(got0[1], rel[:, 2])  # friends_shortest
        check_batch(gg, csr, sources, lane, rel[:, 1], max_hops, materialise=False, arrays=arrays, batch=batch)
    csr.close()


@pytest.mark.parametrize("name", deep_graphs.SMALL)
@pytest.mark.parametrize("max_hops", [-1, 3])
def test_deep_graph_shapes(gg, name, max_hops):
    vid, src, dst = deep_graphs.shape(name)
    csr = build(gg, vid, src, dst)
    sources = datagen.pick_sources(vid, 20, 31)
    lane, t = all_pairs(sources, vid)
    check_batch(gg, csr, sources, lane, t, max_hops)
    csr.close()


@pytest.fixture(scope="module")
def small():
    return datagen.small_graph(400, 700, 77, dangling=6, dup_edges=20)


def test_random_graph_all_64_lanes(gg, small):
    vid, src, dst = small
    csr = build(gg, vid, src, dst)
    sources = vid[:64]
    lane, t = all_pairs(sources, vid)
    got0, got1, st = check_batch(gg, csr, sources, lane, t)
    assert st["paths"] == st["paths_kept"] == 27_146 and st["rows"] == 289_680 and int(got0[2].max()) == 32
    check_batch(gg, csr, sources, lane, t, materialise=False)
    check_batch(gg, csr, sources, lane, t, 2, path_limit=3, edges=False)
    again = gg.bfs64_all_paths(csr, sources, lane, t)  # determinism: identical bytes
    for a, b in zip(again[0] + again[1], got0 + got1):
        assert a.tobytes() == b.tobytes()
    assert again[2]["sigma_entries"] == st["sigma_entries"] and again[2]["sigma_gathered"] == st["sigma_gathered"]
    csr.close()


def test_more_than_64_sources_duplicates_missing_ids_and_source_equals_target(gg, small):
    vid, src, dst = small
    csr = build(gg, vid, src, dst)
    rng = np.random.default_rng(5)
    s = vid[rng.integers(0, 150, 600)]  # 150 distinct sources: three batches, the pairs of a batch scattered
    t = vid[rng.integers(0, vid.size, 600)]
    assert np.unique(s).size > 128
    s[::17] = -5  # ids that are no vertex, on either side
    t[::19] = vid.max() + 3
    t[::23] = s[::23]  # s == t
    s, t = np.concatenate([s, s[:40], s[:40]]), np.concatenate([t, t[:40], t[:40]])  # duplicates, apart
    for max_hops in (-1, 0, 2):
        rows = check_pairs(gg, csr, s, t, max_hops)
        path_zero_is_the_pinned_path(gg, csr, s, t, max_hops, rows)
    check_pairs(gg, csr, s, t, -1, path_limit=2)
    check_pairs(gg, csr, s, t, -1, edges=False)
    assert gg.all_shortest_paths(csr, [], [])[0].size == 0 and gg.shortest_path_counts(csr, [], [])[0].size == 0
    csr.close()


def test_two_lanes_may_carry_the_same_source_and_a_source_may_be_no_vertex(gg, small):
    vid, src, dst = small
    csr = build(gg, vid, src, dst)
    sources = np.array([vid[3], -9, vid[3], vid[8]])
    lane, t = all_pairs(sources, vid)
    got0, got1, st = check_batch(gg, csr, sources, lane, t)
    n = vid.size
    assert np.array_equal(got0[2][got0[0] < n], got0[2][(got0[0] >= 2 * n) & (got0[0] < 3 * n)])
    csr.close()


@pytest.mark.parametrize("path_limit", [0, 1, 17, 5999])
def test_hub_the_rank_crosses_many_chunks(gg, path_limit):
    # s -> 3000 spokes -> t, spoke i reached by i % 3 + 1 parallel rows from s: sigma varies inside t's in-row
    n = 3000
    vid = datagen.person_ids(n + 2, 9)
    s_id, t_id, spokes = vid[0], vid[1], vid[2:]
    reps = np.arange(n) % 3 + 1
    src = np.concatenate([np.repeat(s_id, int(reps.sum())), spokes])
    dst = np.concatenate([np.repeat(spokes, reps), np.repeat(t_id, n)])
    order = np.random.default_rng(3).permutation(src.size)  # parallel rows apart in the table
    csr = build(gg, vid, src[order], dst[order])
    got0, got1, st = check_batch(gg, csr, [s_id], [0, 0, 0], [t_id, spokes[7], s_id], path_limit=path_limit)
    assert got0[2].tolist() == [6000, 2, 1] and st["paths"] == 6003
    assert got0[3].tolist() == [min(6000, path_limit or 6000), min(2, path_limit or 2), 1]
    csr.close()


def test_parallel_rows_are_in_append_order_and_a_self_loop_adds_nothing(gg):
    # 1 -> 2 three times among other rows, 2 -> 3 twice, loops on 2 and 3; with and without explicit descending rowids
    src, dst = np.array([1, 5, 1, 2, 2, 1, 2, 5, 3]), np.array([2, 2, 2, 3, 2, 2, 3, 3, 3])
    vid = np.array([3, 5, 1, 2, 8])
    csr = build(gg, vid, src, dst)
    got0, got1, st = check_batch(gg, csr, [1, 5], [0, 0, 1, 1], [3, 2, 3, 8])
    assert got0[2].tolist() == [6, 3, 1] and got0[1].tolist() == [2, 1, 1]
    first = got1[0] == 0  # rank order at 3: the rows 3, 6 of 2 -> 3, under each the rows 0, 2, 5 of 1 -> 2
    assert got1[4][first].reshape(6, 3).tolist() == [[-1, 0, 3], [-1, 2, 3], [-1, 5, 3], [-1, 0, 6], [-1, 2, 6], [-1, 5, 6]]
    csr.close()
    rowid = 90 - 10 * np.arange(src.size)  # the order is append order, whatever the rowids say
    csr = build(gg, vid, src, dst, rowid)
    got0, got1, st = check_batch(gg, csr, [1, 5], [0, 0, 1, 1], [3, 2, 3, 8])
    first = got1[0] == 0
    assert got1[4][first].reshape(6, 3).tolist() == [[-1, 90, 60], [-1, 70, 60], [-1, 40, 60], [-1, 90, 30], [-1, 70, 30],
                                                    [-1, 40, 30]]
    csr.close()


def test_ladder_saturates_and_refuses_what_does_not_fit(gg):
    vid, src, dst, layers = ref.ladder()
    csr = build(gg, vid, src, dst)
    s_id, t_id = vid[0], vid[layers[66][0]]
    targets = np.array([t_id, vid[layers[64][0]], vid[layers[64][1]], vid[layers[65][0]], vid[layers[65][1]]])
    got0, _, st = check_batch(gg, csr, [s_id], np.zeros(5, int), targets, materialise=False)
    assert got0[2].tolist() == [SAT, 1 << 63, 1 << 63, SAT, SAT] and st["paths"] == SAT and st["rows"] == SAT
    with pytest.raises(GGError) as e:  # 2^64 - 1 or more paths do not fit 2^32 rows
        gg.bfs64_all_paths(csr, [s_id], [0], [t_id])
    assert e.value.code == GG_ERR_TOO_LARGE
    got0, got1, st = check_batch(gg, csr, [s_id], [0], [t_id], path_limit=5)  # the context is usable afterwards
    assert got0[3].tolist() == [5] and got1[0].size == 5 * 67 and st["paths"] == SAT and st["paths_kept"] == 5
    with pytest.raises(GGError) as e:  # one pair of 2^63 paths: a count that no 32-bit scan holds
        gg.bfs64_all_paths(csr, [s_id], [0, 0], [vid[layers[64][0]], vid[layers[3][0]]])
    assert e.value.code == GG_ERR_TOO_LARGE
    with pytest.raises(GGError) as e:  # nor does 2^40 kept paths of one pair
        gg.bfs64_all_paths(csr, [s_id], [0, 0], [vid[layers[64][0]], vid[layers[3][0]]], path_limit=1 << 40)
    assert e.value.code == GG_ERR_TOO_LARGE
    got0, _, st = check_batch(gg, csr, [s_id], [0, 0], [vid[layers[64][0]], vid[layers[3][0]]], path_limit=1 << 40,
                              materialise=False)
    assert got0[3].tolist() == [1 << 40, 4] and st["rows"] == (65 << 40) + 16
    csr.close()


def test_chain_of_260_then_a_diamond_needs_two_byte_distances(gg):
    n = 260
    vid = datagen.person_ids(n + 3, 12)
    chain, a, b, t = vid[:n], vid[n], vid[n + 1], vid[n + 2]
    src = np.concatenate([chain[:-1], [chain[-1], chain[-1], a, b]])
    dst = np.concatenate([chain[1:], [a, b, t, t]])
    csr = build(gg, vid, src, dst)
    got0, got1, st = check_batch(gg, csr, [chain[0], chain[100]], [0, 1, 0, 1], [t, t, chain[254], chain[3]])
    assert got0[1].tolist() == [261, 161, 254] and got0[2].tolist() == [2, 2, 1]
    assert int(got1[2].max()) == 261 and got1[0].size == 2 * 262 + 2 * 162 + 255
    check_batch(gg, csr, [chain[0]], [0, 0], [t, chain[200]], 254)  # bounded at the one-byte limit: the far pair is cut
    csr.close()


def test_64_sources_on_a_ring_see_one_vertex_at_64_distances(gg):
    n = 70
    vid = datagen.person_ids(n, 4)
    ring = np.arange(n)
    twice = ring[::5]  # every fifth ring edge is there twice: sigma doubles along the way
    src = np.concatenate([ring, twice, [0, 10, 20]])
    dst = np.concatenate([(ring + 1) % n, (twice + 1) % n, [35, 45, 55]])  # and three chords
    csr = build(gg, vid, vid[src], vid[dst])
    sources = vid[:64]
    dist, _ = gg.bfs64(csr, sources, -1)
    assert np.unique(dist[:, 69]).size >= 30
    lane, t = all_pairs(sources, vid)
    got0, got1, st = check_batch(gg, csr, sources, lane, t, path_limit=4)
    assert int(got0[2].max()) > 1000
    check_batch(gg, csr, sources, lane, t, materialise=False)
    csr.close()


def test_explicit_rowids_against_append_positions(gg):
    vid, src, dst = datagen.small_graph(200, 500, 13, dup_edges=30)
    sources = vid[:30]
    lane, t = all_pairs(sources, vid)
    csr = build(gg, vid, src, dst)
    _, plain, _ = check_batch(gg, csr, sources, lane, t)
    csr.close()
    rowid = np.arange(src.size, dtype=np.int64) * 3 + 1000
    csr = build(gg, vid, src, dst, rowid)
    _, explicit, _ = check_batch(gg, csr, sources, lane, t)
    csr.close()
    for c in range(4):
        assert np.array_equal(plain[c], explicit[c])
    hop = plain[4] >= 0
    assert np.array_equal(explicit[4][hop], rowid[plain[4][hop]]) and np.all(explicit[4][~hop] == -1)


def test_errors_each_followed_by_a_call_that_succeeds(gg):
    vid, src, dst = datagen.small_graph(100, 300, 21)
    gg.set_edge_rowid(False)
    csr = build(gg, vid, src, dst)
    with pytest.raises(GGError) as e:  # edges without rowids
        gg.bfs64_all_paths(csr, vid[:3], [0, 1, 2], vid[3:6])
    assert e.value.code == GG_ERR_STATE
    check_batch(gg, csr, vid[:3], [0, 1, 2], vid[3:6], edges=False)  # without edges the same CSR serves
    check_batch(gg, csr, vid[:3], [0, 1, 2], vid[3:6], materialise=False)  # and the count needs none
    csr.close()
    gg.set_edge_rowid(True)
    gg.staging_clear()
    gg.append_vertices(vid)
    gg.append_edges(src, dst)
    shard = gg.build_csr_shard(0, 2)
    with pytest.raises(GGError) as e:
        gg.bfs64_all_paths(shard, vid[:3], [0, 1, 2], vid[3:6], edges=False)
    assert e.value.code == GG_ERR_STATE
    shard.close()
    csr = gg.build_csr()
    check_batch(gg, csr, vid[:3], [0, 1, 2], vid[3:6])
    with pytest.raises(GGError) as e:  # a pair that names a source the batch does not have
        gg.bfs64_all_paths(csr, vid[:2], [0, 2], vid[:2])
    assert e.value.code == GG_ERR_INVALID_ARG
    check_batch(gg, csr, vid[:3], [0, 1, 2], vid[3:6])
    # 2^32 pairs: refused before a pair is read
    i64p, u32p = C.POINTER(C.c_int64), C.POINTER(C.c_uint32)
    ids, lanes = np.array(vid[:1], np.int64), np.zeros(1, np.uint32)
    st, res = gg.lib.gg_bfs64_all_paths.argtypes[11]._type_(), C.c_void_p()
    rc = gg.lib.gg_bfs64_all_paths(gg.ctx, csr.handle, ids.ctypes.data_as(i64p), 1, -1, lanes.ctypes.data_as(u32p),
                                   ids.ctypes.data_as(i64p), 1 << 32, 0, 1, 1, C.byref(st), C.byref(res))
    assert rc == GG_ERR_TOO_LARGE and res.value is None
    # neither stats nor a result, and materialising without a result
    rc = gg.lib.gg_bfs64_all_paths(gg.ctx, csr.handle, ids.ctypes.data_as(i64p), 1, -1, lanes.ctypes.data_as(u32p),
                                   ids.ctypes.data_as(i64p), 1, 0, 0, 0, None, None)
    assert rc == GG_ERR_INVALID_ARG
    rc = gg.lib.gg_bfs64_all_paths(gg.ctx, csr.handle, ids.ctypes.data_as(i64p), 1, -1, lanes.ctypes.data_as(u32p),
                                   ids.ctypes.data_as(i64p), 1, 0, 0, 1, C.byref(st), None)
    assert rc == GG_ERR_INVALID_ARG
    # stats only
    rc = gg.lib.gg_bfs64_all_paths(gg.ctx, csr.handle, ids.ctypes.data_as(i64p), 1, -1, lanes.ctypes.data_as(u32p),
                                   ids.ctypes.data_as(i64p), 1, 0, 0, 0, C.byref(st), None)
    assert rc == 0 and (st.pairs_reached, st.paths, st.paths_kept, st.rows) == (1, 1, 1, 1)
    check_batch(gg, csr, vid[:3], [0, 1, 2], vid[3:6])
    csr.close()


def test_the_result_answers_its_own_calls_only(gg):
    vid, src, dst = datagen.small_graph(100, 300, 21)
    csr = build(gg, vid, src, dst)
    lib = gg.lib
    i64p, u32p, i32p, u64p = C.POINTER(C.c_int64), C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_uint64)
    ids, lanes = np.array(vid[:1], np.int64), np.zeros(1, np.uint32)
    mine, other = C.c_void_p(), C.c_void_p()
    assert lib.gg_bfs64_all_paths(gg.ctx, csr.handle, ids.ctypes.data_as(i64p), 1, -1, lanes.ctypes.data_as(u32p),
                                  ids.ctypes.data_as(i64p), 1, 0, 1, 1, None, C.byref(mine)) == 0
    bst = lib.gg_bfs64_paths.argtypes[9]._type_()
    assert lib.gg_bfs64_paths(gg.ctx, csr.handle, ids.ctypes.data_as(i64p), 1, -1, lanes.ctypes.data_as(u32p),
                              ids.ctypes.data_as(i64p), 1, 1, C.byref(bst), C.byref(other)) == 0
    try:
        n, got, nl = C.c_uint64(), C.c_uint32(), C.c_int()
        a, b, c, d = (np.zeros(8, np.int64) for _ in range(4))
        s32, u1, u2 = np.zeros(8, np.int32), np.zeros(8, np.uint64), np.zeros(8, np.uint64)
        p = lambda x: x.ctypes.data_as(i64p)  # noqa: E731
        ptrs3 = (i64p * 3)(p(a), p(b), p(c))
        refused = [
            lib.gg_result_rows(mine, 0, C.byref(n)),
            lib.gg_result_rows(mine, 1, C.byref(n)),
            lib.gg_result_fetch(mine, 0, 0, 8, ptrs3, C.byref(got)),
            lib.gg_result_fetch_edges(mine, 1, 0, 8, ptrs3, C.byref(got)),
            lib.gg_bfs64_paths_rows(mine, C.byref(n)),
            lib.gg_bfs64_paths_fetch(mine, 0, 8, p(a), s32.ctypes.data_as(i32p), p(b), p(c), C.byref(got)),
            lib.gg_walk_closure_levels(mine, u1.ctypes.data_as(u64p), 8, C.byref(nl)),
            lib.gg_walk_closure_fetch(mine, 0, 8, p(a), p(b), s32.ctypes.data_as(i32p), C.byref(got)),
            lib.gg_reach_closure_levels(mine, u1.ctypes.data_as(u64p), 8, C.byref(nl)),
            lib.gg_reach_closure_fetch(mine, 0, 8, p(a), p(b), s32.ctypes.data_as(i32p), C.byref(got)),
            lib.gg_level_sets_levels(mine, u1.ctypes.data_as(u64p), 8, C.byref(nl)),
            lib.gg_level_sets_fetch(mine, 0, 8, p(a), p(b), s32.ctypes.data_as(i32p), C.byref(got)),
            lib.gg_khop_aggregate_rows(mine, 1, C.byref(n)),
            lib.gg_khop_pair_counts_rows(mine, 1, C.byref(n)),
            lib.gg_khop_pair_counts_fetch(mine, 1, 0, 8, p(a), p(b), u1.ctypes.data_as(u64p), C.byref(got)),
            lib.gg_components_rows(mine, 0, C.byref(n)),
            lib.gg_components_fetch(mine, 0, 8, p(a), p(b), u1.ctypes.data_as(u64p), C.byref(got)),
            lib.gg_components_fetch_sizes(mine, 0, 8, p(a), u1.ctypes.data_as(u64p), C.byref(got)),
            lib.gg_triangles_fetch_edges(mine, 0, 8, ptrs3, C.byref(got)),
            # and the three calls refuse every other result
            lib.gg_bfs64_all_paths_rows(other, 0, C.byref(n)),
            lib.gg_bfs64_all_paths_fetch_pairs(other, 0, 8, p(a), s32.ctypes.data_as(i32p), u1.ctypes.data_as(u64p),
                                               u2.ctypes.data_as(u64p), C.byref(got)),
            lib.gg_bfs64_all_paths_fetch(other, 0, 8, p(a), p(b), s32.ctypes.data_as(i32p), p(c), p(d), C.byref(got)),
        ]
        assert refused == [GG_ERR_STATE] * len(refused)
        assert lib.gg_bfs64_all_paths_rows(mine, 2, C.byref(n)) == GG_ERR_INVALID_ARG
        assert lib.gg_bfs64_all_paths_rows(mine, 1, C.byref(n)) == 0 and n.value == 1
        assert lib.gg_bfs64_all_paths_fetch(mine, 0, 8, p(a), p(b), s32.ctypes.data_as(i32p), p(c), None, C.byref(got)) == 0
        assert got.value == 1 and (a[0], b[0], s32[0], c[0]) == (0, 0, 0, vid[0])
        assert lib.gg_bfs64_all_paths_fetch(mine, 1, 8, p(a), p(b), s32.ctypes.data_as(i32p), p(c), None, C.byref(got)) == 0
        assert got.value == 0  # past the end
        assert lib.gg_bfs64_all_paths_fetch_pairs(mine, 0, 8, None, None, u1.ctypes.data_as(u64p), None, C.byref(got)) == 0
        assert got.value == 1 and u1[0] == 1
    finally:
        lib.gg_result_destroy(mine)
        lib.gg_result_destroy(other)
    check_batch(gg, csr, vid[:3], [0, 1, 2], vid[3:6])
    csr.close()
