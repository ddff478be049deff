"""numpy / Python restatement of the all-shortest-paths relation of include/gg.h (gg_bfs64_all_paths).  No GPU.

Inputs are the arrays gg_csr_export gives: off[V + 1], nbr[E] dense destination per entry, eid[E] edge rowid per entry,
vid[V] vertex id by dense index.  For lane s and a vertex x at BFS distance d:

    sigma(s, s) = 1
    sigma(s, x) = sum over the ENTRIES u -> x of x's reverse row with dist(s, u) == d - 1 of sigma(s, u)       (d >= 1)

with Python ints, min'd to 2^64 - 1 after every addition (saturating addition is associative: the order does not matter).
Path number r of a pair is unranked from the target backwards: x's reverse row in ascending (source dense index, forward
CSR position) order, an entry one level closer is taken if r < sigma(s, u), else r -= sigma(s, u).
"""
from __future__ import annotations

import numpy as np

from tests.shortest_path_ref import bfs_dist

SAT = (1 << 64) - 1


def reverse_rows_pos(off, nbr):
    """(roff, rnbr, rpos): row x = the entries u -> x ascending by (u, forward CSR position); rpos that position."""
    off, nbr = np.asarray(off, np.int64), np.asarray(nbr, np.int64)
    V = off.size - 1
    row = np.repeat(np.arange(V, dtype=np.int64), np.diff(off))
    order = np.argsort(nbr, kind="stable")
    roff = np.zeros(V + 1, np.int64)
    np.cumsum(np.bincount(nbr, minlength=V), out=roff[1:])
    return roff, row[order], order.astype(np.int64)


class Batch:
    """One batch of at most 64 sources (dense indices, or None for an id that is no vertex): distances and sigma per
    lane, and the two counters of the count passes."""

    def __init__(self, off, nbr, lanes, max_hops=-1, dist_of=None):
        self.off, self.nbr = np.asarray(off, np.int64), np.asarray(nbr, np.int64)
        self.V = self.off.size - 1
        self.roff, self.rnbr, self.rpos = reverse_rows_pos(self.off, self.nbr)
        self.lanes = list(lanes)
        assert len(self.lanes) <= 64
        self.dist = []  # per lane an int64 array, -1: unreached
        cache = {}
        for s in self.lanes:
            if s is None:
                self.dist.append(np.full(self.V, -1, np.int64))
                continue
            if s not in cache:
                cache[s] = np.asarray(dist_of(s) if dist_of else bfs_dist(self.off, self.nbr, s, max_hops), np.int64)
            self.dist.append(cache[s])
        self.sigma = [self._sigma(l) for l in range(len(self.lanes))]
        self.sigma_entries, self.sigma_gathered = self._counters()

    def _ins(self, x):
        return self.rnbr[self.roff[x]:self.roff[x + 1]]

    def _sigma(self, l):
        dist = self.dist[l]
        sg = {}
        if self.lanes[l] is None:
            return sg
        sg[self.lanes[l]] = 1
        order = np.argsort(dist, kind="stable")
        for x in order[dist[order] >= 1]:
            x, d = int(x), int(dist[x])
            total = 0
            for u in self._ins(x):
                if dist[u] == d - 1:
                    total = min(SAT, total + sg[int(u)])
            sg[x] = total
        return sg

    def _counters(self):
        """sigma_entries: per level L the in-rows of the vertices some lane has at L; sigma_gathered: of those entries the
        ones whose source some lane THAT HAS THE VERTEX AT L has at L - 1."""
        if not self.lanes:
            return 0, 0
        D = np.stack(self.dist)  # [lanes][V]
        entries = gathered = 0
        top = int(D.max())
        for L in range(1, top + 1):
            at = D == L
            for x in np.flatnonzero(at.any(axis=0)):
                ins = self._ins(x)
                entries += ins.size
                if ins.size:
                    lanes = np.flatnonzero(at[:, x])
                    gathered += int((D[np.ix_(lanes, ins)] == L - 1).any(axis=0).sum())
        return entries, gathered

    def count(self, l, t):
        """(d, sigma) of lane l's paths to dense vertex t, or None."""
        if t is None or self.dist[l][t] < 0:
            return None
        return int(self.dist[l][t]), self.sigma[l][t]

    def unrank(self, l, t, r):
        """[(vertex, forward CSR position of the edge into it or -1)] of path r, step 0 first."""
        dist, sg = self.dist[l], self.sigma[l]
        x, rows = t, []
        for i in range(int(dist[t]), 0, -1):
            for k in range(int(self.roff[x]), int(self.roff[x + 1])):
                u = int(self.rnbr[k])
                if dist[u] != i - 1:
                    continue
                if r < sg[u]:
                    rows.append((x, int(self.rpos[k])))
                    x = u
                    break
                r -= sg[u]
            else:
                raise AssertionError("distances and CSR disagree")
        assert x == self.lanes[l]
        rows.append((x, -1))
        return rows[::-1]

    def first_paths(self, l, t, n):
        """the first n paths of (l, t) in rank order (the same rows as unrank(0..n - 1), by one depth-first walk)"""
        dist = self.dist[l]
        out = []
        if n <= 0:
            return out
        tail = []  # (vertex, position of the edge into it) of steps d, d - 1, ... above the cursor
        stack = [(t, int(dist[t]), int(self.roff[t]))]  # (vertex, its step, cursor in its reverse row)
        while stack:
            x, i, k = stack.pop()
            if i == 0:
                out.append([(x, -1)] + tail[::-1])
                if len(out) >= n:
                    return out
                tail.pop() if tail else None
                continue
            while k < self.roff[x + 1] and dist[self.rnbr[k]] != i - 1:
                k += 1
            if k == self.roff[x + 1]:  # the row is done: back to the step above
                tail.pop() if tail else None
                continue
            stack.append((x, i, k + 1))
            tail.append((x, int(self.rpos[k])))
            stack.append((int(self.rnbr[k]), i - 1, int(self.roff[self.rnbr[k]])))
        return out


def _tables_plain(b, dense, vid, eid, pair_lane, pair_dst, path_limit, edges, materialise):
    """the relation as stated, pair by pair and path by path, with Python ints"""
    t0 = ([], [], [], [])
    st = {"pairs_reached": 0, "paths": 0, "paths_kept": 0, "rows": 0}
    todo = []
    for p, (l, t_id) in enumerate(zip(pair_lane, pair_dst)):
        got = b.count(int(l), dense.get(int(t_id)))
        if got is None:
            continue
        d, sg = got
        kept = min(sg, path_limit) if path_limit else sg
        for col, v in zip(t0, (p, d, sg, kept)):
            col.append(v)
        st["pairs_reached"] += 1
        st["paths"] = min(SAT, st["paths"] + sg)
        st["paths_kept"] = min(SAT, st["paths_kept"] + kept)
        st["rows"] = min(SAT, st["rows"] + min(SAT, kept * (d + 1)))
        todo.append((p, int(l), dense[int(t_id)], kept))
    t0 = (np.array(t0[0], np.int64), np.array(t0[1], np.int32), np.array(t0[2], np.uint64), np.array(t0[3], np.uint64))
    if not materialise or st["paths_kept"] >= 1 << 32 or st["rows"] >= 1 << 32:
        return t0, None, st
    cols = ([], [], [], [], [])
    for p, l, t, kept in todo:
        for r, path in enumerate(b.first_paths(l, t, kept)):
            for i, (x, at) in enumerate(path):
                for col, v in zip(cols, (p, r, i, int(vid[x]), int(eid[at]) if edges and at >= 0 else -1)):
                    col.append(v)
    t1 = tuple(np.array(c, np.int32 if k == 2 else np.int64) for k, c in enumerate(cols))
    return t0, t1, st


def _tables_small(b, dense, vid, eid, pair_lane, pair_dst, path_limit, edges, materialise):
    """the same tables with numpy, for batches whose every sigma is below 2^31 (nothing saturates, int64 holds every
    prefix): all paths advance one step at a time, each choosing its entry by a search in the running sum of sigma over
    the entries that lie one level closer (per lane, in reverse-row order).
    test_all_shortest_paths_ref_cpu.py holds it against _tables_plain."""
    D = np.stack(b.dist) if b.lanes else np.zeros((0, b.V), np.int64)
    S = np.zeros(D.shape, np.int64)
    for l, sg in enumerate(b.sigma):
        if sg:
            S[l, list(sg.keys())] = list(sg.values())
    lane = np.asarray(pair_lane, np.int64)
    t = np.array([dense.get(int(x), -1) for x in pair_dst], np.int64)
    ok = t >= 0
    ok[ok] = D[lane[ok], t[ok]] >= 0
    pair = np.flatnonzero(ok)
    lane, t = lane[pair], t[pair]
    d, sg = D[lane, t], S[lane, t]
    kept = np.minimum(sg, path_limit) if path_limit else sg
    st = {"pairs_reached": int(pair.size), "paths": int(sg.sum()), "paths_kept": int(kept.sum()),
          "rows": int((kept * (d + 1)).sum())}
    t0 = (pair.astype(np.int64), d.astype(np.int32), sg.astype(np.uint64), kept.astype(np.uint64))
    if not materialise or st["paths_kept"] >= 1 << 32 or st["rows"] >= 1 << 32:
        return t0, None, st
    # per lane the entries u -> x with dist(u) == dist(x) - 1, in reverse-row order, and the running sum of their sigma
    rrow = np.repeat(np.arange(b.V), np.diff(b.roff))
    ql, qk = np.nonzero((D[:, b.rnbr] == D[:, rrow] - 1) & (D[:, rrow] >= 1))  # ascending by (lane, x, row position)
    w = S[ql, b.rnbr[qk]]
    run = np.cumsum(w)
    qn = np.bincount(ql * b.V + rrow[qk], minlength=D.shape[0] * b.V)
    qoff = np.cumsum(qn) - qn
    # one element per kept path
    of = np.repeat(np.arange(pair.size), kept)
    rank = np.arange(of.size) - np.repeat(np.cumsum(kept) - kept, kept)
    e_lane, x, i, r = lane[of], t[of].copy(), d[of].copy(), rank.copy()
    out = []  # (pair, path, step, dense vertex, forward position or -1)
    while True:
        act = np.flatnonzero(i >= 1)
        if not act.size:
            break
        seg = e_lane[act] * b.V + x[act]
        assert np.all(qn[seg] > 0), "distances and CSR disagree"
        base = run[qoff[seg]] - w[qoff[seg]]  # the running sum before the segment
        k = np.searchsorted(run, base + r[act], side="right")  # the first entry whose prefix exceeds the rank
        assert np.all(k < qoff[seg] + qn[seg]), "distances and CSR disagree"
        out.append((pair[of[act]], rank[act], i[act], x[act], b.rpos[qk[k]]))
        r[act] -= run[k] - w[k] - base
        x[act] = b.rnbr[qk[k]]
        i[act] -= 1
    out.append((pair[of], rank, np.zeros(of.size, np.int64), x, np.full(of.size, -1, np.int64)))
    cols = [np.concatenate([o[c] for o in out]) for c in range(5)]
    order = np.lexsort((cols[2], cols[1], cols[0]))
    cols = [c[order] for c in cols]
    at = cols[4]
    edge = np.where(at >= 0, np.asarray(eid, np.int64)[np.maximum(at, 0)], -1) if edges else np.full(at.size, -1, np.int64)
    vtx = np.asarray(vid, np.int64)[cols[3]]
    return t0, (cols[0].astype(np.int64), cols[1].astype(np.int64), cols[2].astype(np.int32), vtx, edge.astype(np.int64)), st


def make_batch(off, nbr, vid, sources, max_hops=-1, dist_of=None):
    dense = {int(v): i for i, v in enumerate(vid)}
    return Batch(off, nbr, [dense.get(int(s)) for s in sources], max_hops, dist_of)


def batch_tables(off, nbr, eid, vid, sources, pair_lane, pair_dst, max_hops=-1, path_limit=0, edges=True,
                 materialise=True, dist_of=None, plain=None, batch=None):
    """What gg_bfs64_all_paths returns for one batch: (table 0, table 1, stats).  table 0 = (pair int64, hops int32, paths
    uint64, kept uint64); table 1 = (pair int64, path int64, step int32, vertex int64, edge int64) or None when it would
    hold 2^32 rows or more (GG_ERR_TOO_LARGE) or materialise is False; stats = the six counters that are not the BFS's.
    plain: True the relation as stated (slow), False its numpy form, None the numpy form where nothing can saturate.
    batch: make_batch of the same graph, sources and bound, to share among calls."""
    dense = {int(v): i for i, v in enumerate(vid)}
    b = batch or make_batch(off, nbr, vid, sources, max_hops, dist_of)
    small = all(v < 1 << 31 for sg in b.sigma for v in sg.values())
    if plain is None:
        plain = not small
    assert plain or small
    tables = _tables_plain if plain else _tables_small
    t0, t1, st = tables(b, dense, vid, eid, pair_lane, pair_dst, int(path_limit), edges, materialise)
    st["sigma_entries"], st["sigma_gathered"] = b.sigma_entries, b.sigma_gathered
    return t0, t1, st


def all_shortest_paths(off, nbr, eid, vid, src, dst, max_hops=-1, path_limit=0, edges=True):
    """GG.all_shortest_paths: any number of pairs, rows ascending by (pair, path, step).  A pair's rows do not depend on
    the batch it is in, so one batch per distinct source does."""
    parts = []
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    for s in np.unique(src):
        members = np.flatnonzero(src == s)
        _, t1, _ = batch_tables(off, nbr, eid, vid, [s], np.zeros(members.size, np.int64), dst[members], max_hops,
                                path_limit, edges)
        parts.append((members[t1[0]],) + t1[1:])
    if not parts:
        return tuple(np.empty(0, np.int32 if k == 2 else np.int64) for k in range(5))
    cols = [np.concatenate([p[c] for p in parts]) for c in range(5)]
    order = np.argsort(cols[0], kind="stable")
    return tuple(c[order] for c in cols)


def shortest_path_counts(off, nbr, vid, src, dst, max_hops=-1):
    """GG.shortest_path_counts: (pair int64, hops int32, paths uint64) of the reached pairs, ascending by pair."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    eid = np.zeros(np.asarray(nbr).size, np.int64)
    rows = []
    for s in np.unique(src):
        members = np.flatnonzero(src == s)
        t0, _, _ = batch_tables(off, nbr, eid, vid, [s], np.zeros(members.size, np.int64), dst[members], max_hops,
                                materialise=False)
        rows.append((members[t0[0]], t0[1], t0[2]))
    if not rows:
        return np.empty(0, np.int64), np.empty(0, np.int32), np.empty(0, np.uint64)
    cols = [np.concatenate([r[c] for r in rows]) for c in range(3)]
    order = np.argsort(cols[0], kind="stable")
    return tuple(c[order] for c in cols)


def csr_of(vid, src, dst, rowid=None):
    """The arrays gg_csr_export gives for these tables (rows whose endpoints are vertices, grouped by source in append
    order; eid the given rowid or the append position)."""
    dense = {int(v): i for i, v in enumerate(vid)}
    keep = [(dense[int(a)], dense[int(b)], int(rowid[k]) if rowid is not None else k)
            for k, (a, b) in enumerate(zip(src, dst)) if int(a) in dense and int(b) in dense]
    V = len(dense)
    keep.sort(key=lambda e: e[0])  # stable: append order inside a row
    off = np.zeros(V + 1, np.int64)
    for a, _, _ in keep:
        off[a + 1] += 1
    off = np.cumsum(off)
    return (off, np.array([b for _, b, _ in keep], np.int64), np.array([e for _, _, e in keep], np.int64),
            np.asarray(vid, np.int64))


def ladder(layers=65, width=2):
    """Layer 0 = {s}, `layers` layers of `width` vertices, then {t}; consecutive layers fully joined.  (vid, src, dst)."""
    ids, nxt = [[0]], 1
    for _ in range(layers):
        ids.append(list(range(nxt, nxt + width)))
        nxt += width
    ids.append([nxt])
    src, dst = [], []
    for a, b in zip(ids[:-1], ids[1:]):
        for u in a:
            for v in b:
                src.append(u)
                dst.append(v)
    return np.arange(nxt + 1, dtype=np.int64) + 100, np.array(src, np.int64) + 100, np.array(dst, np.int64) + 100, ids
