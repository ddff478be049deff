"""The 64-lane BFS restated level by level in numpy, for tests/test_gpu_bfs_levels.py.

It shares nothing with the C oracle (oracle/gg_oracle.c) nor with the kernels: one bool row of 64 lanes per vertex, the
edge table read as the build reads it (a row whose source or destination is no vertex is dropped; parallel rows and self
loops are kept), and one plain expansion per level, whatever direction the device would take.  Besides the distances it
reports what gg_debug_bfs_steps reports per level -- the vertices that gained a lane (n_active), their out-degrees
counted with multiplicity (te) and the new (lane, vertex) cells (reached) -- and, derived from those alone, the
direction the device's rule gives every level (done if n_active == 0, pull if te * factor > E, else push) and the
word buffer `cur` that rule leaves the frontier in (the parity of the pulls so far).

Vertices are dense indices 0..V-1; a source outside that range is no vertex and leaves its lane empty.  Work per level
is proportional to the frontier's rows, so chains of thousands of levels stay cheap."""
import numpy as np

LANES = 64
PUSH, PULL, DONE = "push", "pull", "done"


class Levels:
    """dist int32 [n_src, V]; n_active / te / reached: Python ints for entry 0 (the seed) .. entry `levels`; mode[l] for
    l = 1..levels (mode[0] is None); after[levels]: what a level levels + 1 would have been (DONE, or the direction the
    bound max_hops cut off); cur[l] for l = 0..levels."""

    def __init__(self, dist, n_active, te, reached, E, factor):
        self.dist, self.n_active, self.te, self.reached, self.E, self.factor = dist, n_active, te, reached, E, factor
        self.levels = len(n_active) - 1
        rule = [DONE if a == 0 else (PULL if t * factor > E else PUSH) for a, t in zip(n_active, te)]
        self.mode = [None] + rule[:-1]
        self.after = rule[-1]
        self.cur = [0]
        for m in self.mode[1:]:
            self.cur.append(self.cur[-1] ^ (1 if m == PULL else 0))

    @property
    def directions(self):
        return self.mode[1:]

    @property
    def totals(self):
        """gg_bfs_stats: the frontiers of the levels that ran are entries 0 .. levels - 1; every entry reached cells"""
        return {"levels": self.levels, "traversed_edges": sum(self.te[:self.levels]),
                "active_vertices": sum(self.n_active[:self.levels]), "reached_pairs": sum(self.reached)}

    @property
    def steps(self):
        """the rows gg_debug_bfs_steps returns"""
        return np.array([self.n_active, self.te, self.reached, self.cur], np.uint64).T.reshape(-1, 4)


def kept_rows(V, src, dst):
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    keep = (src >= 0) & (src < V) & (dst >= 0) & (dst < V)
    return src[keep], dst[keep]


def bfs_levels(V, src, dst, sources, max_hops=-1, factor=8):
    sources = [int(s) for s in sources]
    assert len(sources) <= LANES
    ksrc, kdst = kept_rows(V, src, dst)
    E = int(ksrc.size)
    order = np.argsort(ksrc, kind="stable")
    nbr = kdst[order]
    deg = np.bincount(ksrc, minlength=V).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(deg)])

    seen = np.zeros((V, LANES), bool)  # the lane matrix, one row per vertex
    dist = np.full((len(sources), V), -1, np.int32)
    for lane, s in enumerate(sources):
        if 0 <= s < V:
            seen[s, lane] = True
            dist[lane, s] = 0
    act = np.flatnonzero(seen.any(axis=1))  # a vertex seeded by several lanes is active once
    bits = seen[act].copy()                 # the lanes each active vertex gained at this level
    n_active, te, reached = [int(act.size)], [int(deg[act].sum())], [int(bits.sum())]
    level = 0
    while n_active[-1] and (max_hops < 0 or level < max_hops):
        level += 1
        rows = np.repeat(np.arange(act.size), deg[act])  # which active vertex each walked entry belongs to
        first = np.repeat(off[act] - np.concatenate([[0], np.cumsum(deg[act])[:-1]]), deg[act])
        tgt = nbr[first + np.arange(rows.size)]
        cand, pos = np.unique(tgt, return_inverse=True)
        got = np.zeros((cand.size, LANES), bool)
        np.logical_or.at(got, pos.reshape(-1), bits[rows])
        new = got & ~seen[cand]
        keep = new.any(axis=1)
        act, bits = cand[keep], new[keep]
        seen[act] |= bits
        vi, li = np.nonzero(bits)
        dist[li, act[vi]] = level
        n_active.append(int(act.size))
        te.append(int(deg[act].sum()))
        reached.append(int(bits.sum()))
    return Levels(dist, n_active, te, reached, E, factor)
