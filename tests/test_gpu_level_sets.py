"""gg_level_sets (for L = 1, 2, ... the set of (class, vertex) that L edges lead to from the seeds) against exact level
sets written here from the definition: the rows a UNION recursive CTE with a depth counter adds to its anchor when its
arm joins the CTE with one table (the friends CTE of bi-10-shortestpath.sql).  Rows must match in the documented order —
by level, then ascending (class, dense vertex index) — on every (set, order) combination that exists and on auto."""
import ctypes

import numpy as np
import pytest

from duckdb_pgq_amd import GGError, datagen

pytestmark = pytest.mark.gpu

GG_ERR_INVALID_ARG = -1
GG_ERR_STATE = -6
# (set_mode, order_mode): bitmap + sort, bitmap + compact, hash + sort, auto
COMBINATIONS = ((1, 1), (1, 2), (2, 1), (0, 0))


def exact_levels(src, dst, vid, seeds, classes, max_levels=-1):
    """(class, vertex id, level) of every member of every level >= 1, in gg_level_sets' order.  vid: ids by dense index.
    An unbounded run must end by itself (the caller passes an acyclic graph)."""
    dense = {int(v): i for i, v in enumerate(vid.tolist())}
    adj = {}
    for s, d in zip(src.tolist(), dst.tolist()):
        adj.setdefault(s, set()).add(d)
    cur = {(int(c), int(s)) for s, c in zip(seeds, classes) if int(s) in dense}
    rows, level = [], 0
    while cur and (max_levels < 0 or level < max_levels):
        level += 1
        cur = {(c, w) for c, u in cur for w in adj.get(u, ())}
        rows += [(c, w, level) for c, w in sorted(cur, key=lambda t: (t[0], dense[t[1]]))]
    if not rows:
        return np.empty(0, np.int64), np.empty(0, np.int64), np.empty(0, np.int32)
    a = np.array(rows, np.int64)
    return a[:, 0], a[:, 1], a[:, 2].astype(np.int32)


def build(gg, src, dst):
    gg.staging_clear()
    gg.append_edges(np.asarray(src, np.int64), np.asarray(dst, np.int64))
    gg.vertices_from_edges()
    return gg.build_csr()


def level_sets(gg, csr, seeds, classes, n_classes=None, max_levels=-1):
    res = gg.level_sets(csr, seeds, classes, n_classes, max_levels)
    try:
        got = res.fetch()
        per_level = res.rows()
        assert res.levels() == len(per_level)
        assert sum(per_level) == got[0].size
        assert all(res.rows(L + 1) == n for L, n in enumerate(per_level))
        assert all(n > 0 for n in per_level)
        return got, per_level
    finally:
        res.close()


def check(gg, src, dst, seeds, classes=None, max_levels=-1, n_classes=None):
    """the level sets on every combination equal the exact ones, rows in order; returns the rows per level"""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    seeds = np.asarray(seeds, np.int64)
    classes = np.zeros(seeds.size, np.uint32) if classes is None else np.asarray(classes, np.uint32)
    csr = build(gg, src, dst)
    try:
        vid = csr.export()[3]
        e_cls, e_vid, e_lev = exact_levels(src, dst, vid, seeds, classes, max_levels)
        per_level = None
        for combination in COMBINATIONS:
            gg.debug_level_sets(*combination)
            (cls, v, lev), got_levels = level_sets(gg, csr, seeds, classes, n_classes, max_levels)
            np.testing.assert_array_equal(lev, e_lev, err_msg=f"combination {combination}")
            np.testing.assert_array_equal(cls, e_cls, err_msg=f"combination {combination}")
            np.testing.assert_array_equal(v, e_vid, err_msg=f"combination {combination}")
            assert per_level is None or got_levels == per_level
            per_level = got_levels
        return per_level
    finally:
        gg.debug_level_sets(0, 0)
        csr.close()


def test_path(gg):
    ids = 100 + 7 * np.arange(9)
    assert check(gg, ids[:-1], ids[1:], ids[:1]) == [1] * 8
    assert check(gg, ids[:-1], ids[1:], [ids[3], ids[6]]) == [2, 2, 1, 1, 1]  # two starts in one class


def test_cycle_with_a_bound_repeats_with_its_period(gg):
    n = 5
    ids = 10 + np.arange(n)
    src, dst = ids, np.roll(ids, -1)
    assert check(gg, src, dst, ids[:1], max_levels=13) == [1] * 13
    csr = build(gg, src, dst)
    try:
        (cls, v, lev), _ = level_sets(gg, csr, ids[:1], np.zeros(1, np.uint32), max_levels=13)
        assert v.tolist() == [int(ids[L % n]) for L in range(1, 14)]  # level L and level L + 5 are the same set
    finally:
        csr.close()


def test_bipartite_alternates_and_non_bipartite_saturates(gg):
    # mirrored 4 x 4 grid (bipartite): from a corner the even and the odd side alternate for ever
    cell = lambda r, c: 1000 + 4 * r + c  # noqa: E731
    e = [(cell(r, c), cell(r, c + 1)) for r in range(4) for c in range(3)]
    e += [(cell(r, c), cell(r + 1, c)) for r in range(3) for c in range(4)]
    src = [a for a, b in e] + [b for a, b in e]
    dst = [b for a, b in e] + [a for a, b in e]
    per_level = check(gg, src, dst, [cell(0, 0)], max_levels=12)
    assert per_level[6:] == [8] * 6
    # one more edge closes an odd cycle: every level from some depth on is all 16 vertices
    src2, dst2 = src + [cell(0, 0), cell(1, 1)], dst + [cell(1, 1), cell(0, 0)]
    per_level = check(gg, src2, dst2, [cell(0, 0)], max_levels=12)
    assert per_level[-3:] == [16] * 3


def test_self_loop(gg):
    # 1 -> 1, 1 -> 2, 2 -> 3: the loop keeps 1 in every level
    assert check(gg, [1, 1, 2], [1, 2, 3], [1], max_levels=6) == [2, 3, 3, 3, 3, 3]


def test_hub(gg):
    leaves = 5000 + np.arange(3000)
    hub = np.full(leaves.size, 7, np.int64)
    src, dst = np.concatenate([hub, leaves]), np.concatenate([leaves, hub])  # mirrored star
    assert check(gg, src, dst, [7], max_levels=4) == [3000, 1, 3000, 1]
    assert check(gg, src, dst, leaves[:40], max_levels=3) == [1, 3000, 1]


def test_duplicate_seeds_and_seeds_that_are_no_vertices(gg):
    rng = np.random.default_rng(5)
    ids = 10**6 + rng.choice(10**5, 200, replace=False)
    src, dst = ids[rng.integers(0, 200, 500)], ids[rng.integers(0, 200, 500)]
    once = check(gg, src, dst, ids[:3], max_levels=4)
    assert check(gg, src, dst, [ids[0], ids[1], ids[0], ids[2], ids[1], ids[0]], max_levels=4) == once
    assert check(gg, src, dst, [-5, ids[0], 42, ids[1], ids[2], 2**62], max_levels=4) == once
    assert check(gg, src, dst, [-5, 42], max_levels=4) == []


def test_one_vertex_seeded_in_two_classes(gg):
    rng = np.random.default_rng(6)
    ids = 500 + 3 * np.arange(60)
    src, dst = ids[rng.integers(0, 60, 150)], ids[rng.integers(0, 60, 150)]
    one = check(gg, src, dst, [ids[0]], [0], max_levels=5)
    two = check(gg, src, dst, [ids[0], ids[0], ids[7]], [0, 2, 2], max_levels=5, n_classes=4)  # classes 1 and 3 empty
    assert one and all(b >= a for a, b in zip(one, two))


@pytest.mark.parametrize("n_vertices", [33, 45, 100, 3])
def test_words_straddle_classes(gg, n_vertices):
    """V is no multiple of 32 and there are >= 3 classes: words (and 16-byte groups) hold bits of several classes"""
    rng = np.random.default_rng(n_vertices)
    ids = 77 + 5 * np.arange(n_vertices)
    m = 4 * n_vertices
    src, dst = ids[rng.integers(0, n_vertices, m)], ids[rng.integers(0, n_vertices, m)]
    src, dst = np.concatenate([src, ids]), np.concatenate([dst, np.roll(ids, -1)])  # every id is a vertex: V = n_vertices
    n_classes = 7
    seeds = ids[rng.integers(0, n_vertices, 12)]
    classes = rng.integers(0, n_classes, 12)
    per_level = check(gg, src, dst, seeds, classes, max_levels=5, n_classes=n_classes)
    assert len(per_level) == 5


def test_sink_vertex_is_emitted_and_never_expanded(gg):
    # what a NULL next is staged as: a vertex without out-edges
    sink = -(2**40)
    assert check(gg, [1, 2, 2, 3], [2, sink, 3, sink], [1, sink], [0, 1]) == [1, 2, 1]


def test_max_levels_0_and_1_and_no_seed(gg):
    ids = 100 + np.arange(6)
    assert check(gg, ids[:-1], ids[1:], ids[:2], max_levels=0) == []
    assert check(gg, ids[:-1], ids[1:], ids[:2], max_levels=1) == [2]
    assert check(gg, ids[:-1], ids[1:], []) == []
    assert check(gg, ids[:-1], ids[1:], [], max_levels=3) == []


def test_unbounded_acyclic_graph_ends_by_itself(gg):
    rng = np.random.default_rng(9)
    n = 400
    ids = 10**4 + rng.permutation(n) * 11  # dense order is not id order
    a, b = rng.integers(0, n, 1500), rng.integers(0, n, 1500)
    keep = a != b
    lo, hi = np.minimum(a, b)[keep], np.maximum(a, b)[keep]  # edges run from the lower to the higher position: a DAG
    per_level = check(gg, ids[lo], ids[hi], ids[:20], rng.integers(0, 3, 20))
    assert len(per_level) >= 3


def test_unbounded_cycle_is_an_error_and_the_context_stays_usable(gg):
    ids = 10 + np.arange(6)
    src, dst = np.append(ids[:-1], ids[-1]), np.append(ids[1:], ids[2])  # a tail into a cycle
    csr = build(gg, src, dst)
    try:
        for combination in COMBINATIONS:
            gg.debug_level_sets(*combination)
            with pytest.raises(GGError) as err:
                gg.level_sets(csr, ids[:1], np.zeros(1, np.uint32))
            assert err.value.code == GG_ERR_STATE and "cycle" in str(err.value)
            (_, v, _), per_level = level_sets(gg, csr, ids[:1], np.zeros(1, np.uint32), max_levels=7)
            assert per_level == [1] * 7 and v[:5].tolist() == ids[1:].tolist()
    finally:
        gg.debug_level_sets(0, 0)
        csr.close()


def test_hash_set_with_the_compact_route_is_refused(gg):
    with pytest.raises(GGError) as err:
        gg.debug_level_sets(2, 2)
    assert err.value.code == GG_ERR_INVALID_ARG
    for bad in ((3, 0), (0, 3), (-1, 0)):
        with pytest.raises(GGError):
            gg.debug_level_sets(*bad)
    ids = 100 + np.arange(6)
    assert check(gg, ids[:-1], ids[1:], ids[:1]) == [1] * 5  # the refused call changed nothing


def test_a_class_out_of_range_is_refused(gg):
    csr = build(gg, [1, 2], [2, 3])
    try:
        with pytest.raises(GGError) as err:
            gg.level_sets(csr, [1], [2], n_classes=2)
        assert err.value.code == GG_ERR_INVALID_ARG
    finally:
        csr.close()


def test_random_graphs_many_classes(gg):
    rng = np.random.default_rng(21)
    for n, e, k in ((50, 120, 3), (700, 2000, 9), (4000, 9000, 40)):
        ids = 10**9 + rng.choice(10**8, n, replace=False).astype(np.int64) * 3
        src, dst = ids[rng.integers(0, n, e)], ids[rng.integers(0, n, e)]
        src, dst = np.concatenate([src, dst[: e // 2]]), np.concatenate([dst, src[: e // 2]])  # half of it mirrored
        seeds = ids[rng.integers(0, n, 2 * k)]
        per_level = check(gg, src, dst, seeds, rng.integers(0, k, 2 * k), max_levels=6, n_classes=k)
        assert len(per_level) == 6


def test_sf1_knows_against_numpy(gg):
    """datagen's SF1 knows, 8 persons in 8 classes, 4 levels: per class np.unique of dst[np.isin(src, frontier)]"""
    vid, src, dst = datagen.ldbc("sf1")
    gg.staging_clear()
    gg.append_vertices(vid)
    gg.append_edges(src, dst)
    csr = gg.build_csr()
    try:
        dense_of = csr.export()[3]
        order = np.argsort(dense_of)
        seeds = datagen.pick_sources(vid, 8, 3)
        classes = np.arange(8, dtype=np.uint32)
        expect = []
        frontier = [np.array([s]) for s in seeds]
        for level in range(1, 5):
            for c in range(8):
                frontier[c] = np.unique(dst[np.isin(src, frontier[c])])
                index = order[np.searchsorted(dense_of[order], frontier[c])]  # dense index of every member
                by_index = np.argsort(index)
                expect.append((np.full(frontier[c].size, c), frontier[c][by_index], np.full(frontier[c].size, level)))
        e_cls, e_vid, e_lev = (np.concatenate([t[i] for t in expect]) for i in range(3))
        for combination in COMBINATIONS:
            gg.debug_level_sets(*combination)
            (cls, v, lev), per_level = level_sets(gg, csr, seeds, classes, max_levels=4)
            assert len(per_level) == 4 and per_level[-1] > per_level[0]
            np.testing.assert_array_equal(lev, e_lev, err_msg=f"combination {combination}")
            np.testing.assert_array_equal(cls, e_cls, err_msg=f"combination {combination}")
            np.testing.assert_array_equal(v, e_vid, err_msg=f"combination {combination}")
    finally:
        gg.debug_level_sets(0, 0)
        csr.close()


def test_forest_equals_reach_closure_and_walk_closure_counts(gg):
    """Edges parent -> child, every vertex under at most one parent, the distinct roots seeded each in its own class:
    every (class, vertex) occurs at exactly one level, so the level sets are the reachability closure's rows (no seed
    seen), level by level, and there are as many of them per level as walks."""
    rng = np.random.default_rng(33)
    n = 3000
    ids = 10**7 + rng.permutation(n).astype(np.int64) * 13
    parent = np.array([rng.integers(0, i) if i >= 25 else -1 for i in range(n)])  # 25 roots
    child = np.flatnonzero(parent >= 0)
    src, dst = ids[parent[child]], ids[child]
    perm = rng.permutation(src.size)
    src, dst = src[perm], dst[perm]
    roots = ids[:25]
    classes = np.arange(25, dtype=np.uint32)
    csr = build(gg, src, dst)
    try:
        reach = gg.reach_closure(csr, roots, classes, np.zeros(25, bool))
        walks = gg.walk_closure(csr, roots)
        try:
            r_cls, r_vid, r_lev = reach.fetch()
            r_levels, w_levels = reach.rows(), walks.rows()
        finally:
            reach.close()
            walks.close()
        assert sum(r_levels) == n - 25
        for combination in COMBINATIONS:
            gg.debug_level_sets(*combination)
            (cls, v, lev), per_level = level_sets(gg, csr, roots, classes)
            assert per_level == r_levels == w_levels
            np.testing.assert_array_equal(cls, r_cls)
            np.testing.assert_array_equal(v, r_vid)
            np.testing.assert_array_equal(lev, r_lev)
    finally:
        gg.debug_level_sets(0, 0)
        csr.close()


def test_other_results_refuse_the_level_set_calls(gg):
    csr = build(gg, [1, 2], [2, 3])
    try:
        reach = gg.reach_closure(csr, [1], [0])
        levels = gg.level_sets(csr, [1], [0])
        try:
            n = ctypes.c_int()
            assert gg.lib.gg_level_sets_levels(reach.handle, None, 0, ctypes.byref(n)) == GG_ERR_INVALID_ARG
            assert gg.lib.gg_reach_closure_levels(levels.handle, None, 0, ctypes.byref(n)) == GG_ERR_INVALID_ARG
            assert gg.lib.gg_walk_closure_levels(levels.handle, None, 0, ctypes.byref(n)) == GG_ERR_INVALID_ARG
            assert levels.rows() == [1, 1]
        finally:
            reach.close()
            levels.close()
    finally:
        csr.close()
