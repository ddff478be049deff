"""Sparse multigraphs on which walks of 5 to 8 hops stay enumerable (tests/test_oracle_cpu.py, tests/test_gpu_deep_walks.py).

Every shape returns (vid, src, dst) int64 arrays: vertex ids in a shuffled table order (dense index = table position),
edge rows that may repeat, loop on a vertex, or name an id that is not a vertex (dangling rows, dropped by the build).
"""
from __future__ import annotations

import functools

import numpy as np

from duckdb_pgq_amd import datagen

FUNNEL_SOURCES = 70_000  # > 65 536: the frontier of every level past the first is large enough for the product forms


def _tables(V, s, d, seed, dangling=0):
    vid = datagen.person_ids(V, seed)
    src, dst = vid[np.asarray(s, np.int64)], vid[np.asarray(d, np.int64)]
    if dangling:
        rng = np.random.default_rng(seed + 1)
        at = rng.choice(src.size, dangling, replace=False)
        stranger = vid.max() + 1 + np.arange(dangling, dtype=np.int64)
        half = dangling // 2
        src[at[:half]] = stranger[:half]
        dst[at[half:]] = stranger[half:]
    return vid, src, dst


def multigraph():
    """Random sparse multigraph, mean out-degree ~1.6: self-loops, 40 repeated rows, 8 dangling rows."""
    return datagen.small_graph(300, 480, 5101, dangling=8, dup_edges=40)


def cycle_chords():
    """One 500-cycle with 40 chords, three self-loops and a few parallel rows: walks never die out."""
    n = 500
    rng = np.random.default_rng(5102)
    s = list(range(n)) + list(rng.integers(0, n, 40)) + [7, 7, 250]
    d = [(i + 1) % n for i in range(n)] + list(rng.integers(0, n, 40)) + [7, 7, 250]
    s += [3, 3, 100]  # parallel copies of cycle rows
    d += [4, 4, 101]
    return _tables(n, s, d, 5102, dangling=4)


def hub():
    """60 roots whose chains of 3, 4 or 5 rows lead to one hub of out-degree 200 (two of its rows doubled); the hub's
    leaves mostly lead on to another leaf, so the walks fan out at depth 4 to 6."""
    rng = np.random.default_rng(5103)
    s, d = [], []
    H = 0
    nxt = 1
    for r in range(60):
        length = 3 + r % 3
        chain = list(range(nxt, nxt + length))
        nxt += length
        for a, b in zip(chain, chain[1:] + [H]):
            s.append(a)
            d.append(b)
    leaves = list(range(nxt, nxt + 200))
    nxt += 200
    s += [H] * 202
    d += leaves + leaves[:2]
    for i, v in enumerate(leaves):
        if i % 4:
            s.append(v)
            d.append(leaves[int(rng.integers(0, 200))])
    return _tables(nxt, s, d, 5103, dangling=2)


def dying():
    """Four layers of 100 vertices, each edge one layer down: no walk is longer than 3 hops, so from the fourth level
    on every frontier is empty."""
    rng = np.random.default_rng(5104)
    s, d = [], []
    for layer in range(3):
        for i in range(100):
            for _ in range(int(rng.integers(0, 3))):
                s.append(layer * 100 + i)
                d.append((layer + 1) * 100 + int(rng.integers(0, 100)))
    return _tables(400, s, d, 5104, dangling=2)


def funnel():
    """70 000 sources with one row each into 64 funnel vertices, which point at each other (four of them twice): every
    level past the first holds 70 000 walks or more — both above 65 536 and above an eighth of the edge table."""
    F = 64
    s = list(range(F, F + FUNNEL_SOURCES))
    d = [i % F for i in range(FUNNEL_SOURCES)]
    s += list(range(F)) + [0, 9, 21, 40]
    d += [(5 * a + 1) % F for a in range(F)] + [(5 * a + 2) % F for a in (0, 9, 21, 40)]
    return _tables(F + FUNNEL_SOURCES, s, d, 5105)


def funnel_wide():
    """The funnel without the doubled rows (70 064 walks per level) next to 600 000 rows that end in a sink: the levels
    are above 65 536 but below an eighth of the edge table."""
    F = 64
    n = F + FUNNEL_SOURCES
    s = list(range(F, n)) + list(range(F))
    d = [i % F for i in range(FUNNEL_SOURCES)] + [(5 * a + 1) % F for a in range(F)]
    sink, ballast = n, n + 1 + np.arange(600, dtype=np.int64)
    s = np.concatenate([np.array(s, np.int64), np.repeat(ballast, 1000)])
    d = np.concatenate([np.array(d, np.int64), np.full(600_000, sink, np.int64)])
    return _tables(n + 601, s, d, 5106)


SHAPES = {f.__name__: f for f in (multigraph, cycle_chords, hub, dying, funnel, funnel_wide)}
# (the oracle restatements enumerate every walk through a hash-join chain: the small shapes only)
SMALL = ["multigraph", "cycle_chords", "hub", "dying"]


@functools.lru_cache(maxsize=None)
def shape(name):
    vid, src, dst = SHAPES[name]()
    for a in (vid, src, dst):
        a.setflags(write=False)
    return vid, src, dst


def sources_of(name, vid):
    """A source list: repeats, ids that are no vertex; on the funnels, exactly the funnel's sources."""
    if name.startswith("funnel"):
        return vid[64:64 + FUNNEL_SOURCES]
    pick = datagen.pick_sources(vid, max(1, vid.size // 3), 77)
    return np.concatenate([pick, pick[:5], np.array([-1, vid.max() + 17], np.int64)])


EXT_HUB_ROWS = 300  # the rows of the long key: more than a workgroup has threads


@functools.lru_cache(maxsize=None)
def ext_table(name, seed: int = 0xE18):
    """A second edge table (key -> next) over the vertices of a small shape, modelled on extend_ref.ext_table and sized for
    walk tables of 4 to 8 hops: (src, dst, rowid, info).  info: hub (the key of EXT_HUB_ROWS rows: of the sources that
    start a 7-hop walk, the one that stands in the fewest cells of columns 0, 3 and 7 of that table, so that its rows
    are joined but the output stays small; on a shape without such walks, the first vertex), stranger (a key that is no
    vertex), base (the next ids that are no vertex ids start there)."""
    from tests import edge_filter_ref, triangles_ref

    vid, s, d = shape(name)
    rng = np.random.RandomState(seed)
    V = vid.size
    g = triangles_ref.TriangleGraph(vid, s, d)
    deep = edge_filter_ref.walks(g, sources_of(name, vid), 7)
    starts = np.unique(deep[:, 0])
    cells = np.bincount(deep[:, [0, 3, 7]].reshape(-1), minlength=V)
    hub = int(vid[starts[np.argmin(cells[starts])]]) if starts.size else int(vid[0])
    others = vid[vid != hub]
    light = rng.choice(others, V // 4, replace=False)
    n_light = rng.randint(1, 4, light.size)
    src = np.concatenate([np.repeat(light, n_light), np.full(EXT_HUB_ROWS, hub, np.int64)])
    src = src[rng.permutation(src.size)]  # the rows of a key are not adjacent in append order
    base = int(vid.max()) + 1_000_000
    stranger = int(vid.max()) + 500_000
    dst = base + rng.permutation(src.size).astype(np.int64)
    dst[::7] = vid[rng.randint(0, V, dst[::7].size)]  # next ids that are vertex ids
    # a negative next id, on a row that is neither doubled below nor one of every seventh
    dst[[i for i in range(src.size) if i % 7 and src[i] != hub][0]] = -4242
    # parallel rows (same key, same next), and a key that is no vertex
    twice = np.nonzero(src == hub)[0][:5]
    src = np.concatenate([src, src[twice], np.full(3, stranger, np.int64)])
    dst = np.concatenate([dst, dst[twice], base + np.array([1, 2, 2], np.int64)])
    rowid = (src.size - np.arange(src.size, dtype=np.int64)) * 3 + 5
    info = {"hub": hub, "stranger": stranger, "base": base}
    # what the tests rely on
    keys, per = np.unique(src, return_counts=True)
    per_key = dict(zip(keys.tolist(), per.tolist()))
    vertices = set(vid.tolist())
    assert per_key[hub] == EXT_HUB_ROWS + 5 > 256
    at_hub = np.nonzero(src == hub)[0]
    assert (np.diff(at_hub) > 1).any()  # not adjacent in append order
    with_rows = [k for k in per_key if k in vertices and k != hub]
    assert len(with_rows) == V // 4 and all(1 <= per_key[k] <= 3 for k in with_rows)
    pairs = np.stack([src, dst], axis=1)
    assert pairs.shape[0] - np.unique(pairs, axis=0).shape[0] >= 5
    assert stranger not in vertices and per_key[stranger] == 3
    assert np.isin(dst[:-8:7], vid).all() and (dst < 0).sum() == 1
    assert not np.array_equal(rowid, np.arange(src.size)) and np.unique(rowid).size == rowid.size
    for a in (src, dst, rowid):
        a.setflags(write=False)
    return src, dst, rowid, info
