"""gg_reach_closure (every (class, vertex) reachable from a seed list, each pair once) against an exact closure written
here from its definition: the rows a UNION recursive CTE adds to its distinct anchor rows when its arm joins the CTE
with one table (reachability over knows, interactive-complex-12.sql's extended_tags).  Rows must match in the
documented order: by level, then ascending (class, dense vertex index) inside a level — on both visited-set forms."""
import numpy as np
import pytest

from duckdb_pgq_amd import GGError

pytestmark = pytest.mark.gpu

GG_ERR_INVALID_ARG = -1


def exact_reach(src, dst, vid, seeds, classes, seen):
    """(class, vertex id, level) of every row after the anchor's, in the closure's order.  vid: ids by dense index."""
    dense = {int(v): i for i, v in enumerate(vid.tolist())}
    adj = {}
    for s, d in zip(src.tolist(), dst.tolist()):
        adj.setdefault(s, []).append(d)
    seeds = [int(s) for s in seeds]
    classes = [int(c) for c in classes]
    visited = {(c, s) for s, c, m in zip(seeds, classes, seen) if m and s in dense}
    frontier = list(zip(classes, seeds))
    rows, level = [], 0
    while True:
        level += 1
        new = {(c, w) for c, u in frontier for w in adj.get(u, ()) if (c, w) not in visited}
        if not new:
            break
        visited |= new
        frontier = sorted(new, key=lambda t: (t[0], dense[t[1]]))
        rows += [(c, w, level) for c, w in frontier]
    if not rows:
        return np.empty(0, np.int64), np.empty(0, np.int64), np.empty(0, np.int32)
    a = np.array(rows, np.int64)
    return a[:, 0], a[:, 1], a[:, 2].astype(np.int32)


def build(gg, src, dst):
    gg.staging_clear()
    gg.append_edges(np.asarray(src, np.int64), np.asarray(dst, np.int64))
    gg.vertices_from_edges()
    return gg.build_csr()


def reach(gg, csr, seeds, classes, seen, n_classes=None):
    res = gg.reach_closure(csr, seeds, classes, seen, n_classes)
    try:
        got = res.fetch()
        per_level = res.rows()
        assert res.levels() == len(per_level)
        assert sum(per_level) == got[0].size
        assert all(res.rows(L + 1) == n for L, n in enumerate(per_level))
        return got, per_level
    finally:
        res.close()


def check(gg, src, dst, seeds, classes=None, seen=None, forms=((1, 0), (2, 0))):
    """the closure on every visited-set form in `forms` ((mode, first hash slots) pairs) equals the exact one"""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    seeds = np.asarray(seeds, np.int64)
    classes = np.zeros(seeds.size, np.uint32) if classes is None else np.asarray(classes, np.uint32)
    seen = np.ones(seeds.size, bool) if seen is None else np.asarray(seen, bool)
    csr = build(gg, src, dst)
    try:
        vid = csr.export()[3]
        e_cls, e_vid, e_lev = exact_reach(src, dst, vid, seeds, classes, seen)
        per_level = None
        for mode, slots in forms:
            gg.debug_reach_visited(mode, slots)
            (cls, v, lev), got_levels = reach(gg, csr, seeds, classes, seen)
            np.testing.assert_array_equal(lev, e_lev, err_msg=f"mode {mode}")
            np.testing.assert_array_equal(cls, e_cls, err_msg=f"mode {mode}")
            np.testing.assert_array_equal(v, e_vid, err_msg=f"mode {mode}")
            assert per_level is None or got_levels == per_level
            per_level = got_levels
        return per_level
    finally:
        gg.debug_reach_visited(0, 0)
        csr.close()


def random_graph(rng, n_vertices, n_edges, base=10**9):
    """cycles, self-loops, multi-edges and mirrored edges over sparse ids"""
    ids = base + rng.choice(10**8, n_vertices, replace=False).astype(np.int64) * 3
    a = rng.integers(0, n_vertices, n_edges)
    b = rng.integers(0, n_vertices, n_edges)
    src, dst = list(ids[a]), list(ids[b])
    for v in ids[rng.integers(0, n_vertices, max(1, n_edges // 50))]:  # self-loops
        src.append(v)
        dst.append(v)
    k = max(1, n_edges // 20)  # multi-edges
    src += src[:k]
    dst += dst[:k]
    h = len(src) // 3  # mirrored edges: the reverse of a third of them
    src, dst = src + dst[:h], dst + src[:h]
    perm = rng.permutation(len(src))
    return np.array(src, np.int64)[perm], np.array(dst, np.int64)[perm], ids


def test_random_graphs_one_class(gg):
    rng = np.random.default_rng(11)
    for n, e in ((20, 30), (300, 450), (5000, 9000)):
        src, dst, ids = random_graph(rng, n, e)
        per_level = check(gg, src, dst, ids[:1])
        assert per_level, (n, e)
        check(gg, src, dst, ids[:5])  # several seeds, one class


def test_several_classes_one_with_several_seeds(gg):
    rng = np.random.default_rng(12)
    src, dst, ids = random_graph(rng, 2000, 2600)
    seeds = np.concatenate([ids[:6], ids[100:103]])
    classes = [0, 1, 2, 3, 4, 5, 3, 3, 7]  # class 3 has three seeds; class 6 has none
    check(gg, src, dst, seeds, classes)


def test_seeds_not_vertices_unseen_seeds_and_duplicates(gg):
    """an unseen seed is a row of the level that reaches it again; a seed that is no vertex reaches nothing"""
    src, dst = [1, 2, 3, 3, 4], [2, 3, 1, 4, 4]
    per_level = check(gg, src, dst, [1], seen=[False])
    assert per_level == [1, 1, 2]  # level 3 reaches 1 again (unseen) and 4
    check(gg, src, dst, [1, 1, 99, -5, 2**62, 3, 1], classes=[0, 0, 0, 1, 1, 1, 2],
          seen=[True, False, True, False, True, False, False])
    assert check(gg, src, dst, [99, -5]) == []  # no seed is a vertex: no rows


def test_no_seeds(gg):
    assert check(gg, [1, 2], [2, 3], []) == []


def test_hash_set_from_a_tiny_capacity_grows_several_times(gg):
    rng = np.random.default_rng(13)
    src, dst, ids = random_graph(rng, 3000, 5000)
    seeds = ids[:40]
    classes = np.arange(40) % 13
    seen = np.arange(40) % 3 != 0
    check(gg, src, dst, seeds, classes, seen, forms=((1, 0), (2, 0), (2, 2), (2, 7)))


def test_many_classes_take_the_hash_set_by_themselves(gg):
    """one class per seed, as a reply forest's posts: the budget picks the hash set only if n_classes x V is large — the
    automatic choice must agree with both forced forms either way"""
    rng = np.random.default_rng(14)
    src, dst, ids = random_graph(rng, 4000, 4000)
    seeds = ids[:500]
    check(gg, src, dst, seeds, np.arange(500), forms=((0, 0), (1, 0), (2, 0)))


def forest(rng, n, roots, base=10**12):
    """reply forest: message i >= roots replies to a random earlier message; edges parent -> child"""
    ids = base + rng.choice(10**9, n, replace=False).astype(np.int64) * 7
    parent = np.array([rng.integers(0, max(1, min(i, roots + i // 3))) if i >= roots else -1 for i in range(n)])
    src = ids[parent[roots:]]
    dst = ids[roots:]
    perm = rng.permutation(src.size)
    return src[perm], dst[perm], ids


def test_on_forests_the_rows_are_the_walk_closures_ends(gg):
    """on an acyclic forest every walk ends at a distinct vertex: the (seed, end vertex) set of gg_walk_closure is the
    reach closure's (class, vertex) set when every seed is its own class"""
    rng = np.random.default_rng(15)
    for n, roots in ((400, 10), (20000, 300)):
        src, dst, ids = forest(rng, n, roots)
        seeds = ids[:roots]
        check(gg, src, dst, seeds, np.arange(roots))
        csr = build(gg, src, dst)
        try:
            walks = gg.walk_closure(csr, seeds)
            try:
                w_seed, w_rowid, w_lev = walks.fetch()
            finally:
                walks.close()
            (cls, v, lev), _ = reach(gg, csr, seeds, np.arange(roots), None)
        finally:
            csr.close()
        w_end = dst[w_rowid]  # rowid = append position
        walk_set = set(zip(w_seed.tolist(), w_end.tolist(), w_lev.tolist()))
        reach_set = set(zip(cls.tolist(), v.tolist(), lev.tolist()))
        assert len(walk_set) == w_seed.size == cls.size
        assert walk_set == reach_set


def test_errors_and_the_context_stays_usable(gg):
    csr = build(gg, [1, 2], [2, 1])
    try:
        with pytest.raises(GGError) as e:
            gg.reach_closure(csr, [1, 2], [0, 3], None, 2)  # class 3 of 2
        assert e.value.code == GG_ERR_INVALID_ARG
        with pytest.raises(GGError):
            gg.debug_reach_visited(3, 0)
    finally:
        csr.close()
    assert check(gg, [1, 2], [2, 1], [1], seen=[True]) == [1]


def test_kernels_are_launched(gg):
    """the level loop runs the reach kernels (and the shared tile partition and radix sort)"""
    csr = build(gg, [1, 1, 2, 3], [2, 3, 4, 1])
    gg.profile_reset()
    gg.profile_select(None)
    gg.profile(True)
    try:
        gg.debug_reach_visited(2, 0)
        gg.reach_closure(csr, [1, 2], [0, 1], [True, False]).close()
    finally:
        gg.profile(False)
        csr.close()
    names = set(gg.profile_get())
    assert {"reach_deg", "reach_expand", "reach_emit", "reach_insert", "tile_partition"} <= names, names
