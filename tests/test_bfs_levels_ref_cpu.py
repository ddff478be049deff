"""The level-by-level BFS reference (tests/bfs_levels_ref.py) and the direction-steering shapes (tests/bfs_shapes.py),
checked without a GPU: the reference against three graphs worked by hand and against the C oracle's bfs64 on the
suite's random graphs, and every shape's built-for direction sequence against the reference -- a shape that stops
steering fails here, before tests/test_gpu_bfs_levels.py compares the device with it."""
import numpy as np
import pytest

from duckdb_pgq_amd import datagen
from tests import bfs_shapes as shapes
from tests.bfs_levels_ref import DONE, PULL, PUSH, bfs_levels


def test_diamond_with_a_parallel_row_a_self_loop_and_dangling_rows_by_hand():
    """0 -> 1, 0 -> 2, 1 -> 3, 2 -> 3, 3 -> 3, 0 -> 1 again, and two rows with an endpoint that is no vertex (dropped:
    E = 6).  Lanes: 0 at vertex 0, 1 at vertex 2, 2 at a stranger, 3 at vertex 0 again."""
    src = [0, 0, 1, 2, 3, 0, 9, 1]
    dst = [1, 2, 3, 3, 3, 1, 0, -4]
    r = bfs_levels(4, src, dst, [0, 2, 77, 0])
    assert r.E == 6
    assert r.dist.tolist() == [[0, 1, 1, 2], [-1, -1, 0, 1], [-1, -1, -1, -1], [0, 1, 1, 2]]
    # seed: vertices 0 (lanes 0 and 3, active once) and 2; out-degrees 3 (the parallel row counts) and 1
    # level 1: vertex 1 gains lanes 0, 3; vertex 2 gains 0, 3; vertex 3 gains lane 1      -> degrees 1 + 1 + 1
    # level 2: vertex 3 gains lanes 0, 3                                                   -> its self loop
    # level 3: the self loop offers nothing new
    assert r.n_active == [2, 3, 1, 0] and r.te == [4, 3, 1, 0] and r.reached == [3, 5, 2, 0]
    assert r.levels == 3
    # 4 * 8 > 6, 3 * 8 > 6, 1 * 8 > 6: every level pulls
    assert r.directions == [PULL, PULL, PULL] and r.cur == [0, 1, 0, 1] and r.after == DONE
    assert r.totals == {"levels": 3, "traversed_edges": 8, "active_vertices": 6, "reached_pairs": 10}
    assert r.steps.tolist() == [[2, 4, 3, 0], [3, 3, 5, 1], [1, 1, 2, 0], [0, 0, 0, 1]]


def test_bounded_chain_with_ballast_by_hand():
    """0 -> 1 -> 2 -> 3 and a 40-row clique-ish block on 4..8 that no source reaches: E = 43, te = 1, 8 <= 43: push.
    max_hops cuts the search with a frontier left; max_hops = 0 runs no level."""
    blk = [(a, b) for a in range(4, 9) for b in range(4, 9) for _ in range(2) if a != b]
    src = [0, 1, 2] + [a for a, _ in blk]
    dst = [1, 2, 3] + [b for _, b in blk]
    r = bfs_levels(9, src, dst, [0, 1], max_hops=2)
    assert r.E == 43 and r.levels == 2
    assert r.dist.tolist() == [[0, 1, 2, -1] + [-1] * 5, [-1, 0, 1, 2] + [-1] * 5]
    assert r.n_active == [2, 2, 2] and r.te == [2, 2, 1] and r.reached == [2, 2, 2]
    assert r.directions == [PUSH, PUSH] and r.cur == [0, 0, 0] and r.after == PUSH  # (the bound cut a push off)
    assert r.totals == {"levels": 2, "traversed_edges": 4, "active_vertices": 4, "reached_pairs": 6}
    r0 = bfs_levels(9, src, dst, [0, 1], max_hops=0)
    assert r0.levels == 0 and r0.directions == [] and r0.n_active == [2] and r0.reached == [2]
    assert r0.totals == {"levels": 0, "traversed_edges": 0, "active_vertices": 0, "reached_pairs": 2}
    full = bfs_levels(9, src, dst, [0, 1])
    assert full.levels == 4 and full.n_active == [2, 2, 2, 1, 0] and full.te == [2, 2, 1, 0, 0]
    assert full.directions == [PUSH] * 4  # (te = 0 pushes too, and finds nothing)


def test_push_then_pull_by_hand():
    """0 -> 1, then 1 -> {2..9}, each of those -> 10, and a 14-row tail 11 -> 12 repeated: E = 1 + 8 + 8 + 14 = 31.
    te: 1 (8 <= 31: push), 8 (64 > 31: pull), 8 (pull), 0 (push, nothing).  One lane: cur flips on the pulls only."""
    src = [0] + [1] * 8 + list(range(2, 10)) + [11] * 14
    dst = [1] + list(range(2, 10)) + [10] * 8 + [12] * 14
    r = bfs_levels(13, src, dst, [0])
    assert r.E == 31
    assert r.dist.tolist() == [[0, 1] + [2] * 8 + [3, -1, -1]]
    assert r.n_active == [1, 1, 8, 1, 0] and r.te == [1, 8, 8, 0, 0] and r.reached == [1, 1, 8, 1, 0]
    assert r.directions == [PUSH, PULL, PULL, PUSH] and r.cur == [0, 0, 1, 0, 0]
    # the same graph under another threshold: with factor 2 only te = 8 * 2 > 31 fails everywhere
    assert bfs_levels(13, src, dst, [0], factor=2).directions == [PUSH] * 4
    assert bfs_levels(13, src, dst, [0], factor=32).directions == [PULL, PULL, PULL, PUSH]


@pytest.mark.parametrize("V,E,seed,max_hops,dangling,dup",
                         [(30, 60, 1, 5, 3, 0), (100, 300, 2, 3, 3, 0), (100, 300, 2, 0, 3, 0), (64, 2000, 3, 2, 3, 0),
                          (3000, 40000, 4, -1, 3, 0), (40, 30, 4, 6, 3, 0), (400, 700, 77, -1, 6, 20),
                          (200, 500, 13, -1, 0, 30), (120, 900, 31, 4, 6, 15), (1, 0, 1, -1, 0, 0)])
def test_reference_equals_the_oracle_on_the_suites_random_graphs(orc, V, E, seed, max_hops, dangling, dup):
    """distances and the four totals of the oracle's bfs64, sources as the parity tests draw them: up to 64 with a
    stranger and a repeat"""
    vid, src, dst = datagen.small_graph(V, E, seed, dangling=dangling, dup_edges=dup)
    rc, g = orc.csr_build(vid, src, dst)
    assert rc == 0
    sources = np.concatenate([datagen.pick_sources(vid, 61, seed), np.array([999], np.int64), vid[:2]])[:64]
    o_dist, o_st = g.bfs64(g.lookup(sources), max_hops)
    pos = {int(x): i for i, x in enumerate(vid)}
    dense = lambda ids: [pos.get(int(x), -1) for x in ids]  # noqa: E731
    r = bfs_levels(V, dense(src), dense(dst), dense(sources), max_hops)
    assert r.E == g.E
    assert np.array_equal(r.dist, o_dist)
    assert r.totals == o_st
    g.close()


@pytest.mark.parametrize("name", sorted(shapes.BUILDERS))
def test_every_shape_steers_the_directions_it_was_built_for(name):
    s = shapes.shape(name)
    r = bfs_levels(s.V, s.src, s.dst, s.sources)
    assert r.directions == s.directions, (name, r.n_active, r.te, r.E)
    assert r.after == DONE
    both = {PUSH, PULL}
    assert set(s.directions) <= both
    if s.symmetric:
        half = s.src.size // 2
        assert np.array_equal(s.src[:half], s.dst[half:]) and np.array_equal(s.dst[:half], s.src[half:])


def test_shapes_hold_the_edges_they_promise():
    """what the GPU tests rely on beyond the sequence: row lengths, vertex counts, hub positions, lanes per row"""
    for layout in ("front", "corners"):
        s = shapes.shape("push_rows_" + layout)
        deg = np.bincount(s.src, minlength=s.V)
        assert deg[s.sources].tolist() == shapes.HUB_DEGREES
        r = bfs_levels(s.V, s.src, s.dst, s.sources)
        assert int((r.dist >= 0).sum(axis=0).max()) >= 6  # several lanes meet in one vertex's word
    assert {0, 63, 64, shapes.shape("push_rows_corners").V - 1} <= set(shapes.shape("push_rows_corners").sources.tolist())
    for v in "abc":
        s = shapes.shape("pull_rows_" + v)
        indeg = np.bincount(s.dst, minlength=s.V)
        assert set(shapes.IN_DEGREES) <= set(indeg.tolist())
    s = shapes.shape("pull_rows_c")
    r = bfs_levels(s.V, s.src, s.dst, s.sources)
    indeg = np.bincount(s.dst, minlength=s.V)
    for g in range(8):  # every group slot of a wavefront sees every in-degree
        assert set(indeg[64 + g::8].tolist()) == set(shapes.IN_DEGREES)
    for t in range(64, s.V):  # a row of d entries brings exactly the lanes 0 .. min(d, 64) - 1
        assert np.flatnonzero(r.dist[:, t] == 1).tolist() == list(range(min(int(indeg[t]), 64)))
    s = shapes.shape("pull_rows_a")
    roff, rnbr = shapes.reverse_rows(s.V, s.src, s.dst)
    srcs = set(s.sources.tolist())
    for t in np.flatnonzero(np.bincount(s.dst, minlength=s.V)[:14] > 0):
        if t >= 2:
            row = rnbr[roff[t]:roff[t + 1]]
            assert row[-1] in srcs and not (set(row[:-1].tolist()) & srcs)
    for v in shapes.V_EDGES:
        assert shapes.shape(f"star_push_V{v}").V % 128 == v % 128
        if v > 1:
            assert shapes.shape(f"star_pull_V{v}").V == v
    s = shapes.shape("deep_all_lanes")
    r = bfs_levels(s.V, s.src, s.dst, s.sources)
    assert r.levels == 333 and all(m == PULL for m in r.mode[268:333])
    assert np.all(r.dist.max(axis=1) > 255) and int(r.dist[63].max()) == 269 and int(r.dist[0].max()) == 332


def test_long_chain_in_closed_form():
    """what the 65 535-vertex chain of the GPU test is compared with, held to the reference on a shorter one"""
    s = shapes.long_chain(1000, lanes=4)
    r = bfs_levels(s.V, s.src, s.dst, s.sources)
    assert r.levels == 1000 and r.directions == s.directions
    assert np.array_equal(r.dist, np.tile(np.arange(1000, dtype=np.int32), (4, 1)))
    assert r.n_active == [1] * 1000 + [0] and r.te == [1] * 999 + [0, 0] and r.reached == [4] * 1000 + [0]
