"""numpy restatement of the shortest-path relation of include/gg.h (gg_bfs64_paths).  Pure Python, no GPU.

Inputs are the arrays gg_csr_export gives (the oracle's CSR build gives the same ones, test_csr_build_bit_exact):
off[V + 1], nbr[E] dense destination per entry, eid[E] edge rowid per entry, vid[V] vertex id by dense index.

For a source s and a vertex x with BFS distance d >= 1:
    pred(s, x)  the in-neighbour u of x with dist(s, u) == d - 1 that has the smallest dense index: the first such entry
                of x's reverse row when the rows list the sources of the edges into x ascending by (u, rowid) — a stable
                sort of the CSR entries by destination
    edge(s, x)  the first entry of pred(s, x)'s forward row, in CSR order, whose destination is x; its rowid
The path of (s, t) is p_d = t, p_{i-1} = pred(s, p_i); one row (pair index, step i, vid[p_i], edge into p_i or -1) per step.
"""
from __future__ import annotations

import numpy as np


def reverse_rows(off, nbr):
    """(roff, rnbr): row x = the sources u of the entries u -> x, in ascending (u, CSR position) order."""
    V = off.size - 1
    row = np.repeat(np.arange(V, dtype=np.int64), np.diff(off))
    order = np.argsort(nbr, kind="stable")
    roff = np.zeros(V + 1, np.int64)
    np.cumsum(np.bincount(np.asarray(nbr, np.int64), minlength=V), out=roff[1:])
    return roff, row[order]


def bfs_dist(off, nbr, s: int, max_hops: int = -1):
    """dist[V] from dense vertex s over the forward rows, -1 where there is no path of at most max_hops edges."""
    off = np.asarray(off, np.int64)
    V = off.size - 1
    dist = np.full(V, -1, np.int64)
    dist[s] = 0
    frontier = np.array([s], np.int64)
    level = 0
    while frontier.size and (max_hops < 0 or level < max_hops):
        level += 1
        lo, lens = off[frontier], off[frontier + 1] - off[frontier]
        idx = np.repeat(lo - (np.cumsum(lens) - lens), lens) + np.arange(int(lens.sum()), dtype=np.int64)  # every row entry
        nxt = np.unique(np.asarray(nbr, np.int64)[idx])
        nxt = nxt[dist[nxt] < 0]
        dist[nxt] = level
        frontier = nxt
    return dist


def shortest_paths(off, nbr, eid, vid, src_ids, dst_ids, max_hops: int = -1, edges: bool = True, dist_of=None):
    """(pair_index int64, step int32, vertex int64, edge int64) in (pair, step) order.  dist_of(dense source) may supply
    the distances (an int array over the vertices, -1: unreached) instead of bfs_dist."""
    off, nbr = np.asarray(off, np.int64), np.asarray(nbr, np.int64)
    roff, rnbr = reverse_rows(off, nbr)
    dense = {int(v): i for i, v in enumerate(vid)}
    cache = {}
    pair, step, vtx, edge = [], [], [], []
    for p, (s_id, t_id) in enumerate(zip(src_ids, dst_ids)):
        s, t = dense.get(int(s_id)), dense.get(int(t_id))
        if s is None or t is None:
            continue
        if s not in cache:
            cache[s] = np.asarray(dist_of(s) if dist_of else bfs_dist(off, nbr, s, max_hops), np.int64)
        dist = cache[s]
        d = int(dist[t])
        if d < 0 or (0 <= max_hops < d):
            continue
        rows = []
        x = t
        for i in range(d, 0, -1):
            ins = rnbr[roff[x]:roff[x + 1]]
            closer = ins[dist[ins] == i - 1]
            assert closer.size, "distances and CSR disagree"
            u = int(closer[0])
            at = int(off[u]) + int(np.flatnonzero(nbr[off[u]:off[u + 1]] == x)[0])
            rows.append((i, int(vid[x]), int(eid[at]) if edges else -1))
            x = u
        assert x == s
        rows.append((0, int(vid[s]), -1))
        for i, v, e in reversed(rows):
            pair.append(p)
            step.append(i)
            vtx.append(v)
            edge.append(e)
    return (np.array(pair, np.int64), np.array(step, np.int32), np.array(vtx, np.int64), np.array(edge, np.int64))
