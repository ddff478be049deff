"""GG.shortest_paths (gg_bfs64_paths) against the numpy restatement of the relation (tests/shortest_path_ref.py), row for
row: which shortest path is reported — the predecessor with the smallest dense index, the parallel edge appended first —
is part of the contract, so the comparison is exact, not up to a choice of path."""
import numpy as np
import pytest

from duckdb_pgq_amd import GGError, datagen
from tests import deep_graphs
from tests import shortest_path_ref as ref
from tests.test_golden import NAMES, bfs_cases, load

pytestmark = pytest.mark.gpu

GG_ERR_INVALID_ARG, GG_ERR_STATE = -1, -6


def build(gg, vid, src, dst, rowid=None):
    gg.staging_clear()
    gg.append_vertices(np.asarray(vid, np.int64))
    gg.append_edges(np.asarray(src, np.int64), np.asarray(dst, np.int64), rowid)
    return gg.build_csr()


def check(gg, csr, s, t, max_hops=-1, edges=True):
    """the device's rows equal the restatement's; their number is the sum of d + 1 over the pairs gg_bfs64 reaches"""
    s, t = np.asarray(s, np.int64), np.asarray(t, np.int64)
    off, nbr, eid, vid = csr.export()
    want = ref.shortest_paths(off, nbr, eid, vid, s, t, max_hops, edges)
    got = gg.shortest_paths(csr, s, t, max_hops, edges)
    for name, g, w in zip(("pair", "step", "vertex", "edge"), got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), name
    # row count from the distances of the existing BFS, one batch of sources at a time
    total = 0
    uniq = np.unique(s)
    dense = {int(v): i for i, v in enumerate(vid)}
    for b0 in range(0, uniq.size, 64):
        batch = uniq[b0:b0 + 64]
        dist, _ = gg.bfs64(csr, batch, max_hops)
        lane = {int(v): i for i, v in enumerate(batch)}
        for a, b in zip(s, t):
            if int(a) in lane and int(b) in dense:
                d = int(dist[lane[int(a)], dense[int(b)]])
                total += d + 1 if d >= 0 else 0
    assert got[0].size == total
    return got


def all_pairs(sources, vid):
    return np.repeat(sources, vid.size), np.tile(vid, len(sources))


@pytest.mark.parametrize("name", NAMES)
def test_goldens(gg, name):
    g = load(name)
    vid, src, dst = g["vid"], g["src"], g["dst"]
    csr = build(gg, vid, src, dst)
    for sources, max_hops, rel in bfs_cases(g):
        got = check(gg, csr, rel[:, 0], rel[:, 1], max_hops)  # every friends_shortest row of the compiled reference
        starts = np.flatnonzero(got[1] == 0)
        lengths = np.diff(np.append(starts, got[0].size)) - 1
        assert np.array_equal(lengths, rel[:, 2])
    csr.close()


@pytest.mark.parametrize("name", deep_graphs.SMALL)
@pytest.mark.parametrize("max_hops", [-1, 3])
def test_deep_graph_shapes(gg, name, max_hops):
    vid, src, dst = deep_graphs.shape(name)
    csr = build(gg, vid, src, dst)
    sources = datagen.pick_sources(vid, 20, 31)
    s, t = all_pairs(sources, vid)
    check(gg, csr, s, t, max_hops)
    csr.close()


def test_skewed_star_plus_chain(gg):
    # a hub with 3000 spokes in both directions (rows longer than any lane group) and a 40-chain hanging off one spoke
    n, L = 3000, 40
    hub, spokes, chain = 0, np.arange(1, n + 1), np.arange(n + 1, n + 1 + L)
    src = np.concatenate([np.full(n, hub), spokes, [spokes[-1]], chain[:-1]])
    dst = np.concatenate([spokes, np.full(n, hub), [chain[0]], chain[1:]])
    vid = datagen.person_ids(n + 1 + L, 9)
    csr = build(gg, vid, vid[src], vid[dst])
    s = vid[np.array([hub, 1, 2, chain[0], 5, n])]
    ss, tt = all_pairs(s, vid)
    check(gg, csr, ss, tt)
    csr.close()


def test_parallel_edges_the_one_appended_first_wins(gg):
    # 1 -> 2 three times among other rows, 2 -> 3 twice; both orders of explicit rowids
    src, dst = np.array([1, 5, 1, 2, 1, 2, 5]), np.array([2, 2, 2, 3, 2, 3, 3])
    vid = np.array([3, 5, 1, 2, 8])
    csr = build(gg, vid, src, dst)
    pair, step, vtx, edge = check(gg, csr, [1, 1, 5], [3, 2, 3])
    assert edge.tolist() == [-1, 0, 3, -1, 0, -1, 6]
    csr.close()
    rowid = np.array([70, 60, 50, 40, 30, 20, 10])  # the CSR keeps append order: the first appended still wins
    csr = build(gg, vid, src, dst, rowid)
    pair, step, vtx, edge = check(gg, csr, [1, 1, 5], [3, 2, 3])
    assert edge.tolist() == [-1, 70, 40, -1, 70, -1, 10]
    csr.close()


def test_self_loops_isolated_vertices_and_source_equals_target(gg):
    vid = np.array([10, 11, 12, 13, 14])
    src, dst = np.array([10, 10, 11, 12, 12]), np.array([10, 11, 12, 12, 10])  # 13, 14 isolated
    csr = build(gg, vid, src, dst)
    s, t = all_pairs(vid, vid)
    pair, step, vtx, edge = check(gg, csr, s, t)
    own = {int(p): (int(v), int(e)) for p, st, v, e in zip(pair, step, vtx, edge) if s[p] == t[p]}
    assert own == {0: (10, -1), 6: (11, -1), 12: (12, -1), 18: (13, -1), 24: (14, -1)}  # one row each, no loop edge
    csr.close()


def test_unreachable_cut_missing_and_duplicate_pairs(gg):
    vid, src, dst = datagen.small_graph(400, 700, 77, dangling=6, dup_edges=20)
    csr = build(gg, vid, src, dst)
    rng = np.random.default_rng(5)
    s = vid[rng.integers(0, vid.size, 300)]
    t = vid[rng.integers(0, vid.size, 300)]
    s[::17] = -5            # ids that are no vertex, on either side
    t[::19] = vid.max() + 3
    s, t = np.concatenate([s, s[:40], s[:40]]), np.concatenate([t, t[:40], t[:40]])  # duplicates, apart
    for max_hops in (-1, 0, 1, 2, 4):
        check(gg, csr, s, t, max_hops)
    check(gg, csr, s, t, -1, edges=False)
    assert gg.shortest_paths(csr, [], [])[0].size == 0
    csr.close()


def test_more_than_64_distinct_sources(gg):
    vid, src, dst = datagen.ldbc_knows(3000, 40_000, 3)
    csr = build(gg, vid, src, dst)
    rng = np.random.default_rng(6)
    s = vid[rng.integers(0, 200, 5000)]  # 200 distinct sources: four batches, pairs of a batch scattered
    t = vid[rng.integers(0, vid.size, 5000)]
    assert np.unique(s).size > 128
    check(gg, csr, s, t, 4)
    csr.close()


def test_chain_of_300_vertices_needs_two_byte_distances(gg):
    n = 300
    vid = datagen.person_ids(n, 12)
    order = np.arange(n)
    csr = build(gg, vid, vid[order[:-1]], vid[order[1:]])
    pair, step, vtx, edge = check(gg, csr, [vid[0], vid[0], vid[10], vid[299]], [vid[299], vid[254], vid[290], vid[0]])
    assert pair.size == 300 + 255 + 281 and step.max() == 299
    check(gg, csr, [vid[0], vid[0]], [vid[299], vid[200]], 254)  # bounded at the one-byte limit: the far pair is cut
    csr.close()


def test_explicit_rowids_against_append_positions(gg):
    vid, src, dst = datagen.small_graph(200, 500, 13, dup_edges=30)
    s, t = all_pairs(vid[:30], vid)
    csr = build(gg, vid, src, dst)
    plain = check(gg, csr, s, t)
    csr.close()
    rowid = np.arange(src.size, dtype=np.int64) * 3 + 1000
    csr = build(gg, vid, src, dst, rowid)
    explicit = check(gg, csr, s, t)
    csr.close()
    for c in range(3):
        assert np.array_equal(plain[c], explicit[c])
    hop = plain[3] >= 0
    assert np.array_equal(explicit[3][hop], rowid[plain[3][hop]]) and np.all(explicit[3][~hop] == -1)


def test_edges_without_rowids_and_shards_are_refused(gg):
    vid, src, dst = datagen.small_graph(100, 300, 21)
    gg.set_edge_rowid(False)
    csr = build(gg, vid, src, dst)
    with pytest.raises(GGError) as e:
        gg.shortest_paths(csr, vid[:3], vid[3:6])
    assert e.value.code == GG_ERR_STATE
    check(gg, csr, vid[:10], vid[10:20], -1, edges=False)  # without edges the same CSR serves
    csr.close()
    gg.set_edge_rowid(True)
    gg.staging_clear()
    gg.append_vertices(vid)
    gg.append_edges(src, dst)
    shard = gg.build_csr_shard(0, 2)
    with pytest.raises(GGError) as e:
        gg.shortest_paths(shard, vid[:3], vid[3:6], -1, edges=False)
    assert e.value.code == GG_ERR_STATE
    shard.close()
    csr = gg.build_csr()
    with pytest.raises(GGError) as e:  # a pair that names a source the batch does not have
        gg.bfs64_paths(csr, vid[:2], [0, 2], vid[:2])
    assert e.value.code == GG_ERR_INVALID_ARG
    check(gg, csr, vid[:3], vid[3:6])  # the context is usable afterwards
    csr.close()
