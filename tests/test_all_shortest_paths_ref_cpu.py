"""The restatement of the all-shortest-paths relation (tests/all_shortest_paths_ref.py) against brute force — every walk of
d edge rows, enumerated — on tiny graphs with parallel rows and self-loops, against the single pinned path
(tests/shortest_path_ref.py), and at the saturation boundary.  No GPU."""
import itertools

import numpy as np
import pytest

from tests import all_shortest_paths_ref as ref
from tests import shortest_path_ref as one

SAT = (1 << 64) - 1


def tiny_graph(seed):
    """at most 8 vertices, parallel rows, self-loops, rows that name no vertex; explicit rowids in descending order"""
    rng = np.random.default_rng(seed)
    V = int(rng.integers(3, 9))
    vid = rng.permutation(np.arange(20, 20 + V))
    E = int(rng.integers(V, 2 * V + 3))
    src, dst = vid[rng.integers(0, V, E)], vid[rng.integers(0, V, E)]
    src = np.concatenate([src, src[:3], [vid[0], 999]])  # three parallel rows, a self-loop, a dangling row
    dst = np.concatenate([dst, dst[:3], [vid[0], vid[1]]])
    rowid = 1000 - np.arange(src.size)
    return vid, src, dst, rowid


def brute_force(off, nbr, eid, s, t, d):
    """every walk of d entries from s to t as [(vertex, entry or -1)], step 0 first, sorted by the pinned key: from the
    target backwards, (source dense index, forward CSR position) of each entry"""
    row = np.repeat(np.arange(off.size - 1), np.diff(off))
    walks = []
    for w in itertools.product(range(nbr.size), repeat=d):
        if d and (row[w[0]] != s or nbr[w[-1]] != t):
            continue
        if any(nbr[a] != row[b] for a, b in zip(w[:-1], w[1:])):
            continue
        walks.append(w)
    walks.sort(key=lambda w: [(int(row[e]), e) for e in reversed(w)])
    return [[(s, -1)] + [(int(nbr[e]), e) for e in w] for w in walks]


@pytest.mark.parametrize("seed", range(12))
def test_count_and_rank_order_against_brute_force(seed):
    vid, src, dst, rowid = tiny_graph(seed)
    off, nbr, eid, v2 = ref.csr_of(vid, src, dst, rowid)
    V = v2.size
    b = ref.Batch(off, nbr, list(range(V)))
    seen_many = False
    for s in range(V):
        for t in range(V):
            got = b.count(s, t)
            if got is None:
                continue
            d, sg = got
            if d > 4:
                continue  # (nbr.size ** d walks to look through)
            want = brute_force(off, nbr, eid, s, t, d)
            assert sg == len(want) >= 1
            seen_many |= sg > 1
            assert [b.unrank(s, t, r) for r in range(sg)] == want
            assert b.first_paths(s, t, sg) == want
            assert b.first_paths(s, t, 1) == want[:1]
    assert seen_many or seed  # (seed 0 is known to have pairs with several paths)


@pytest.mark.parametrize("seed", range(12))
def test_tables_and_path_zero_is_the_pinned_path(seed):
    vid, src, dst, rowid = tiny_graph(seed)
    off, nbr, eid, v2 = ref.csr_of(vid, src, dst, rowid)
    s, t = np.repeat(v2, v2.size), np.tile(v2, v2.size)
    s, t = np.append(s, [999, v2[0]]), np.append(t, [v2[0], 999])  # ids that are no vertex
    for max_hops in (-1, 2):
        pair, path, step, vtx, edge = ref.all_shortest_paths(off, nbr, eid, v2, s, t, max_hops)
        assert step.dtype == np.int32 and pair.dtype == path.dtype == vtx.dtype == edge.dtype == np.int64
        key = list(zip(pair.tolist(), path.tolist(), step.tolist()))
        assert key == sorted(key)
        first = path == 0
        want = one.shortest_paths(off, nbr, eid, v2, s, t, max_hops)
        for g, w in zip((pair[first], step[first], vtx[first], edge[first]), want):
            assert np.array_equal(g, w)
        lim = ref.all_shortest_paths(off, nbr, eid, v2, s, t, max_hops, path_limit=1)
        for g, w in zip((lim[0], lim[2], lim[3], lim[4]), want):
            assert np.array_equal(g, w)
        cp, ch, cn = ref.shortest_path_counts(off, nbr, v2, s, t, max_hops)
        assert cn.dtype == np.uint64 and ch.dtype == np.int32
        starts = np.flatnonzero(step == 0)
        n_of = np.bincount(pair[starts], minlength=s.size)
        assert np.array_equal(cp, np.flatnonzero(n_of)) and np.array_equal(cn, n_of[cp].astype(np.uint64))
        no_edges = ref.all_shortest_paths(off, nbr, eid, v2, s, t, max_hops, edges=False)
        assert np.all(no_edges[4] == -1) and np.array_equal(no_edges[3], vtx)


def same(a, b):
    assert a[2] == b[2]
    assert (a[1] is None) == (b[1] is None)
    for x, y in zip(a[0] + (a[1] or ()), b[0] + (b[1] or ())):
        assert x.dtype == y.dtype and np.array_equal(x, y)


@pytest.mark.parametrize("seed", range(12))
def test_the_numpy_form_of_the_tables_equals_the_plain_one(seed):
    vid, src, dst, rowid = tiny_graph(seed)
    arrays = ref.csr_of(vid, src, dst, rowid)
    sources = np.append(arrays[3], [999, arrays[3][0]])  # an id that is no vertex, a source twice
    lane, t = np.repeat(np.arange(sources.size), vid.size + 1), np.tile(np.append(arrays[3], 998), sources.size)
    for kw in ({}, {"max_hops": 2, "path_limit": 2}, {"edges": False, "max_hops": 0}, {"materialise": False}):
        same(ref.batch_tables(*arrays, sources, lane, t, plain=False, **kw),
             ref.batch_tables(*arrays, sources, lane, t, plain=True, **kw))
    same(ref.batch_tables(*arrays, sources, [], [], plain=False), ref.batch_tables(*arrays, sources, [], [], plain=True))
    same(ref.batch_tables(*arrays, [], [], [], plain=False), ref.batch_tables(*arrays, [], [], [], plain=True))


def test_the_numpy_form_on_a_random_graph_with_parallel_rows():
    from duckdb_pgq_amd import datagen
    vid, src, dst = datagen.small_graph(400, 700, 77, dangling=6, dup_edges=20)
    arrays = ref.csr_of(vid, src, dst)
    lane, t = np.repeat(np.arange(64), vid.size), np.tile(vid, 64)
    got = ref.batch_tables(*arrays, vid[:64], lane, t, plain=False)
    same(got, ref.batch_tables(*arrays, vid[:64], lane, t, plain=True))
    assert (got[2]["paths"], got[2]["rows"], int(got[0][2].max())) == (27_146, 289_680, 32)


def test_batch_stats_and_limit_on_a_diamond_with_parallel_rows():
    # 0 -> 1 twice, 0 -> 2, 1 -> 3, 2 -> 3 twice, 3 -> 3: sigma(0, 3) = 2 * 1 + 1 * 2 = 4
    vid = np.array([10, 11, 12, 13])
    src, dst = np.array([10, 10, 10, 11, 12, 12, 13]), np.array([11, 12, 11, 13, 13, 13, 13])
    off, nbr, eid, v2 = ref.csr_of(vid, src, dst)
    t0, t1, st = ref.batch_tables(off, nbr, eid, v2, [10, 77, 10], [0, 1, 2, 0, 0], [13, 13, 13, 10, 55])
    assert [c.tolist() for c in t0] == [[0, 2, 3], [2, 2, 0], [4, 4, 1], [4, 4, 1]]
    assert st == {"pairs_reached": 3, "paths": 9, "paths_kept": 9, "rows": 25,
                  # level 1: in-rows of 11 (2 entries) and 12 (1), all from 10; level 2: 13's (1 + 2 + the loop), 3 gathered
                  "sigma_entries": 3 + 4, "sigma_gathered": 3 + 3}
    # rank order at 13: entries (11, row 3), (12, row 4), (12, row 5); under 11 the rows 0, 2 of 10 -> 11
    first = t1[0] == 0
    assert t1[4][first].tolist() == [-1, 0, 3, -1, 2, 3, -1, 1, 4, -1, 1, 5]
    assert t1[1][first].tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3]
    t0, t1, st = ref.batch_tables(off, nbr, eid, v2, [10], [0, 0], [13, 10], path_limit=3)
    assert t0[2].tolist() == [4, 1] and t0[3].tolist() == [3, 1]
    assert (st["paths"], st["paths_kept"], st["rows"]) == (5, 4, 10)
    assert t1[4].tolist() == [-1, 0, 3, -1, 2, 3, -1, 1, 4, -1]


def test_saturation_boundary_on_the_ladder():
    vid, src, dst, layers = ref.ladder()
    off, nbr, eid, v2 = ref.csr_of(vid, src, dst)
    b = ref.Batch(off, nbr, [0])
    assert b.count(0, layers[64][0]) == (64, 1 << 63) and b.count(0, layers[64][1]) == (64, 1 << 63)
    assert b.count(0, layers[65][0]) == (65, SAT) and b.count(0, layers[66][0]) == (66, SAT)
    assert b.count(0, layers[63][1]) == (63, 1 << 62)
    t_id, near = int(v2[layers[66][0]]), int(v2[layers[64][0]])
    t0, t1, st = ref.batch_tables(off, nbr, eid, v2, [v2[0]], [0, 0], [t_id, near])
    assert t1 is None  # 2^32 rows or more
    assert t0[2].tolist() == [SAT, 1 << 63] and st["paths"] == SAT and st["rows"] == SAT
    t0, t1, st = ref.batch_tables(off, nbr, eid, v2, [v2[0]], [0], [t_id], path_limit=5)
    assert t0[3].tolist() == [5] and st["paths_kept"] == 5 and st["rows"] == 5 * 67 and st["paths"] == SAT
    assert [b.unrank(0, layers[66][0], r) for r in range(5)] == b.first_paths(0, layers[66][0], 5)
    # the first five by rank differ in the three layers next to the source only (the low bits of the rank)
    paths = t1[3].reshape(5, 67)
    assert np.all(paths[:, 4:] == paths[0, 4:]) and len({tuple(p) for p in paths.tolist()}) == 5
