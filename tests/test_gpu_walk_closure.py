"""gg_walk_closure (every walk from a seed list, level by level, to no fixed depth) against an exact closure written
here: the rows a UNION ALL recursive CTE adds to its anchor when its arm joins the CTE with one table (bi-9.sql post_all,
interactive-short-6.sql chain).  Rows must match in the documented order: by level, then parent row, then CSR order
(the edge rows' append order) inside the parent's vertex row."""
import numpy as np
import pytest

from duckdb_pgq_amd import GGError

pytestmark = pytest.mark.gpu

GG_ERR_STATE = -6


def exact_closure(src, dst, rowid, seeds, max_levels=None):
    """(seed index, edge rowid, level) of every walk of >= 1 edges, in the closure's order"""
    out = {}
    for s, d, r in zip(src.tolist(), dst.tolist(), rowid.tolist()):  # CSR order inside a row: the append order
        out.setdefault(s, []).append((r, d))
    cur = [(i, s) for i, s in enumerate(np.asarray(seeds, np.int64).tolist())]
    rows, level = [], 0
    while cur and (max_levels is None or level < max_levels):
        level += 1
        nxt = [(i, r, d) for i, v in cur for r, d in out.get(v, ())]
        rows += [(i, r, level) for i, r, _ in nxt]
        cur = [(i, d) for i, _, d in nxt]
    if not rows:
        return np.empty(0, np.int64), np.empty(0, np.int64), np.empty(0, np.int32)
    a = np.array(rows, np.int64)
    return a[:, 0], a[:, 1], a[:, 2].astype(np.int32)


def closure(gg, src, dst, rowid, seeds, max_levels=None):
    """stage the edges key -> next with their rowids, vertex set = endpoints, run the closure, fetch every row"""
    gg.staging_clear()
    gg.append_edges(src, dst, rowid)
    gg.vertices_from_edges()
    csr = gg.build_csr()
    try:
        res = gg.walk_closure(csr, seeds, max_levels)
        try:
            got = res.fetch()
            per_level = res.rows()
            assert res.levels() == len(per_level)
            assert sum(per_level) == got[0].size
            assert all(res.rows(L + 1) == n for L, n in enumerate(per_level))
            return got, per_level
        finally:
            res.close()
    finally:
        csr.close()


def check(gg, src, dst, seeds, max_levels=None, rowid=None):
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    rowid = np.arange(src.size, dtype=np.int64) if rowid is None else np.asarray(rowid, np.int64)
    (seed, rid, lev), per_level = closure(gg, src, dst, rowid, seeds, max_levels)
    e_seed, e_rid, e_lev = exact_closure(src, dst, rowid, seeds, max_levels)
    assert seed.size == e_seed.size, (seed.size, e_seed.size)
    np.testing.assert_array_equal(lev, e_lev)
    np.testing.assert_array_equal(seed, e_seed)
    np.testing.assert_array_equal(rid, e_rid)
    assert per_level == [int((e_lev == L).sum()) for L in range(1, (int(e_lev.max()) if e_lev.size else 0) + 1)]
    return per_level


def forest(rng, n, roots, chain=0, base=10**12):
    """reply forest: message i > roots replies to a random earlier message; plus a chain of `chain` replies.  Edges
    parent -> child (bi-9's key m_c_replyof, next m_messageid).  Ids are sparse."""
    ids = base + rng.choice(10**9, n + chain, replace=False).astype(np.int64) * 7
    parent = np.array([rng.integers(0, max(1, min(i, roots + i // 3))) if i >= roots else -1 for i in range(n)])
    src = [ids[parent[i]] for i in range(roots, n)]
    dst = [ids[i] for i in range(roots, n)]
    prev = ids[0]
    for j in range(chain):
        src.append(prev)
        dst.append(ids[n + j])
        prev = ids[n + j]
    perm = rng.permutation(len(src))
    return np.array(src, np.int64)[perm], np.array(dst, np.int64)[perm], ids


def test_random_forests_with_deep_chains(gg):
    rng = np.random.default_rng(5)
    for n, roots, chain in ((300, 12, 45), (5000, 40, 70), (20000, 500, 0)):
        src, dst, ids = forest(rng, n, roots, chain)
        per_level = check(gg, src, dst, ids[:roots])
        assert len(per_level) >= (chain if chain else 1)
    # every message as a seed: each reply appears once per ancestor
    src, dst, ids = forest(rng, 2000, 20, 41)
    assert len(check(gg, src, dst, ids)) >= 41


def test_dags_with_shared_descendants(gg):
    """a vertex reached along several walks appears once per walk"""
    rng = np.random.default_rng(9)
    layers = [np.arange(L * 1000, L * 1000 + w, dtype=np.int64) for L, w in enumerate((4, 12, 30, 40, 25, 6))]
    src, dst = [], []
    for a, b in zip(layers, layers[1:]):
        for v in a:
            for w in rng.choice(b, size=min(b.size, 5), replace=False):
                src.append(v)
                dst.append(w)
    src, dst = np.array(src), np.array(dst)
    perm = rng.permutation(src.size)
    # explicit rowids that are not the append positions: the rows carry them, the order stays the append order
    rowid = rng.choice(10**6, src.size, replace=False).astype(np.int64)
    per_level = check(gg, src[perm], dst[perm], layers[0], rowid=rowid[perm])
    assert len(per_level) == 5 and per_level[-1] > layers[-1].size  # shared descendants, several walks each
    check(gg, src, dst, np.concatenate([layers[0], layers[2]]))


def test_hub_with_200k_children(gg):
    """one hub post with 200 000 replies (and replies to some of those): spread over many tiles"""
    rng = np.random.default_rng(3)
    hub, kids = 77, np.arange(1000, 201000, dtype=np.int64)
    grand = np.arange(10**6, 10**6 + 30000, dtype=np.int64)
    src = np.concatenate([np.full(kids.size, hub), rng.choice(kids, grand.size), [5, 5]])
    dst = np.concatenate([kids, grand, [6, hub]])
    perm = rng.permutation(src.size)
    per_level = check(gg, src[perm], dst[perm], [5, hub, 6])
    assert per_level[:2] == [2 + 200000, 200000 + 30000]


def test_seeds_that_are_not_vertices_and_duplicates(gg):
    src, dst = np.array([1, 1, 2, 3, 3]), np.array([2, 3, 4, 4, 5])
    check(gg, src, dst, [99, 1, 1, -5, 3, 2**62, 1])
    check(gg, src, dst, [99, -5])  # no seed is a vertex: no rows


def test_empty_anchor(gg):
    src, dst = np.array([1, 2]), np.array([2, 3])
    assert check(gg, src, dst, []) == []


def test_max_levels_cuts_the_walks(gg):
    rng = np.random.default_rng(1)
    src, dst, ids = forest(rng, 3000, 10, 50)
    for k in (0, 1, 2, 7, 49):
        per_level = check(gg, src, dst, ids[:10], max_levels=k)
        assert len(per_level) == k
    # a cycle under a bound is a finite recursion
    check(gg, [1, 2, 3], [2, 3, 1], [1, 2], max_levels=10)


def test_an_unbounded_cycle_is_refused_and_the_context_stays_usable(gg):
    src, dst = np.array([1, 2, 3, 3]), np.array([2, 3, 1, 4])
    with pytest.raises(GGError) as e:
        closure(gg, src, dst, np.arange(4, dtype=np.int64), [1])
    assert e.value.code == GG_ERR_STATE and "cycle" in str(e.value)
    # a cycle that no seed reaches does not matter
    check(gg, [1, 2, 3, 10], [2, 3, 1, 11], [10])
    check(gg, [5, 6], [6, 7], [5])


def test_kernels_are_launched(gg):
    """the level loop runs the three closure kernels (and the shared tile partition)"""
    gg.staging_clear()
    gg.append_edges(np.array([1, 1, 2]), np.array([2, 3, 4]))
    gg.vertices_from_edges()
    csr = gg.build_csr()
    gg.profile_reset()
    gg.profile_select(None)
    gg.profile(True)
    try:
        gg.walk_closure(csr, [1]).close()
    finally:
        gg.profile(False)
        csr.close()
    names = set(gg.profile_get())
    assert {"closure_deg", "closure_expand", "closure_emit", "tile_partition"} <= names, names
