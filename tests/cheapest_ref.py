"""gg_cheapest64 restated in plain python integers (include/gg.h): the yardstick of the device kernels.

Weights are integers >= 0, one per edge row in append order (the weights of dangling rows are never read).  Lane i is
sources[i] (every listed position its own lane; an id that is no vertex has no rows).  With cost_0 = 0 at the lane's vertex
and nothing elsewhere,
    cost_r(x) = min(cost_{r-1}(x), min over the edge rows u -> x of cost_{r-1}(u) (+) w(row)),
(+) saturating at INT64_MAX, in strict rounds: round r reads nothing round r wrote.  A round that lowers no cell ends the
search; so does max_hops >= 0 if it comes first.  hops(x) = the round that wrote the final cost.  One row (lane, id(x), cost,
hops) per reached cell whose id passes the target list, ascending by (lane, dense index).

Three independent statements of the answer: the rounds (cheapest), a heap Dijkstra over (cost, hops) pairs (dijkstra) and
the reference's own SQL (sql_cheapest)."""
import heapq

import numpy as np

INT64_MAX = (1 << 63) - 1
LANES = 64


def hashed_weights(n: int, lo: int = 1, hi: int = 100) -> np.ndarray:
    """a fixed hash of the row number into lo..hi"""
    r = np.arange(n, dtype=np.uint64)
    h = (r * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(40)
    return (h % np.uint64(hi - lo + 1)).astype(np.int64) + lo


class WeightedGraph:
    """(vid, src, dst, w) with the dangling edge rows dropped: su, dv, wk are the kept rows as dense indices and python
    integer weights, in append order; out[u] = [(v, w)] per kept row u -> v."""

    def __init__(self, vid, src, dst, w):
        self.vid = np.asarray(vid, np.int64)
        self.V = int(self.vid.size)
        self.index = {int(v): i for i, v in enumerate(self.vid.tolist())}
        src, dst = np.asarray(src, np.int64).tolist(), np.asarray(dst, np.int64).tolist()
        w = [int(x) for x in (w.tolist() if hasattr(w, "tolist") else w)]
        assert len(src) == len(dst) == len(w)
        self.su, self.dv, self.wk, self.kept = [], [], [], []
        for r, (s, d, x) in enumerate(zip(src, dst, w)):
            if s in self.index and d in self.index:
                assert x >= 0
                self.su.append(self.index[s]), self.dv.append(self.index[d]), self.wk.append(x), self.kept.append(r)
        self.E = len(self.su)
        self.out = [[] for _ in range(self.V)]
        for u, v, x in zip(self.su, self.dv, self.wk):
            self.out[u].append((v, x))
        self.outdeg = [len(o) for o in self.out]

    def entry_weights(self) -> np.ndarray:
        """the kept rows' weights in the order gg_csr_export shows: by source, a row's entries in append order"""
        order = np.argsort(np.asarray(self.su, np.int64), kind="stable")
        return np.array([self.wk[i] for i in order.tolist()], np.int64)


def _allowed(g, targets):
    if targets is None:
        return None
    return {g.index[int(t)] for t in np.asarray(targets, np.int64).reshape(-1).tolist() if int(t) in g.index}


def cheapest(g, sources, max_hops: int = -1, targets=None) -> dict:
    """{"rows": (src_index int64, ids int64, cost list of ints, hops list of ints), "rounds", "reached_pairs",
    "cells_lowered", "entries_pulled", "rows_gathered"}.  sources: any number of ids; every batch of 64 runs its own rounds
    and the statistics are summed the way GG.cheapest_path_lengths sums them."""
    sources = [int(s) for s in np.asarray(sources, np.int64).reshape(-1).tolist()]
    allowed = _allowed(g, targets)
    st = {"rounds": 0, "reached_pairs": 0, "cells_lowered": 0, "entries_pulled": 0, "rows_gathered": 0}
    idx, ids, costs, hopss = [], [], [], []
    limit = 0 if g.E == 0 else (g.V if max_hops < 0 or max_hops > g.V else max_hops)
    for base in range(0, len(sources), LANES):
        batch = sources[base:base + LANES]
        cost = [{g.index[s]: 0} if s in g.index else {} for s in batch]
        hops = [{v: 0 for v in c} for c in cost]
        fresh = [dict(c) for c in cost]  # per lane: the cells lowered in the last round and their values
        st["reached_pairs"] += sum(len(c) for c in cost)
        for r in range(1, limit + 1):
            st["rounds"] += 1
            st["entries_pulled"] += g.E
            alive = set()
            for f in fresh:
                alive.update(f)
            st["rows_gathered"] += sum(g.outdeg[u] for u in alive)
            lowered_round = 0
            nxt = []
            for lane, f in enumerate(fresh):
                cand = {}
                for u, c in f.items():
                    for v, x in g.out[u]:
                        s = min(c + x, INT64_MAX)
                        if v not in cand or s < cand[v]:
                            cand[v] = s
                low = {v: s for v, s in cand.items() if v not in cost[lane] or s < cost[lane][v]}
                st["reached_pairs"] += sum(1 for v in low if v not in cost[lane])
                nxt.append(low)
                lowered_round += len(low)
            for lane, low in enumerate(nxt):  # (only now: a round reads nothing it wrote)
                cost[lane].update(low)
                hops[lane].update({v: r for v in low})
            fresh = nxt
            st["cells_lowered"] += lowered_round
            if not lowered_round:
                break
        for lane, c in enumerate(cost):
            for v in sorted(c):
                if allowed is None or v in allowed:
                    idx.append(base + lane), ids.append(int(g.vid[v])), costs.append(c[v]), hopss.append(hops[lane][v])
    st["rows"] = (np.array(idx, np.int64), np.array(ids, np.int64), costs, hopss)
    return st


def dijkstra(g, source: int, max_edges=None) -> dict:
    """{dense: (cost, hops)} from one source id by a binary heap over (cost, hops) pairs compared lexicographically: the
    cheapest cost and, among the walks of that cost, the fewest edges.  No bound on the edges (the fixpoint)."""
    assert max_edges is None
    if int(source) not in g.index:
        return {}
    s = g.index[int(source)]
    best = {s: (0, 0)}
    heap = [(0, 0, s)]
    done = set()
    while heap:
        c, h, u = heapq.heappop(heap)
        if u in done:
            continue
        done.add(u)
        for v, x in g.out[u]:
            key = (min(c + x, INT64_MAX), h + 1)
            if v not in best or key < best[v]:
                best[v] = key
                heapq.heappush(heap, (key[0], key[1], v))
    return best


def same(a, b) -> bool:
    """two (src_index, ids, cost, hops) tuples hold the same rows in the same order"""
    return (np.array_equal(np.asarray(a[0], np.int64), np.asarray(b[0], np.int64))
            and np.array_equal(np.asarray(a[1], np.int64), np.asarray(b[1], np.int64))
            and [int(x) for x in a[2]] == [int(x) for x in b[2]] and [int(x) for x in a[3]] == [int(x) for x in b[3]])


def id_rows(rows, sources) -> list:
    """the rows as sorted (source id, vertex id, cost, hops) tuples — what a SQL statement returns"""
    s = np.asarray(sources, np.int64).reshape(-1)
    return sorted((int(s[i]), int(v), int(c), int(h)) for i, v, c, h in
                  zip(np.asarray(rows[0]).tolist(), np.asarray(rows[1]).tolist(), rows[2], rows[3]))


def sql_cheapest(max_hops: int, sources=None, targets=None, weight: str = "k_weight") -> str:
    """the reference statement over person(p_personid) and knows(k_person1id, k_person2id, <weight>): every walk of at most
    max_hops edges from the listed persons as a UNION ALL recursive CTE, then min(cost) per (s, v) and min(hops) among the
    rows of that cost.  sources / targets: distinct ids as IN lists; None: every person."""
    anchor = "" if sources is None else " WHERE p_personid IN (" + ", ".join(str(int(s)) for s in sources) + ")"
    cut = "" if targets is None else " AND b.v IN (" + ", ".join(str(int(t)) for t in targets) + ")"
    return (
        "WITH RECURSIVE w(s, v, cost, hops) AS ("
        f"SELECT p_personid, p_personid, CAST(0 AS BIGINT), 0 FROM person{anchor} "
        f"UNION ALL SELECT w.s, k.k_person2id, w.cost + k.{weight}, w.hops + 1 FROM w, knows k, person p "
        f"WHERE w.v = k.k_person1id AND k.k_person2id = p.p_personid AND w.hops < {int(max_hops)}), "
        "best AS (SELECT s, v, min(cost) AS cost FROM w GROUP BY s, v) "
        "SELECT b.s, b.v, b.cost, min(w.hops) FROM best b, w "
        f"WHERE w.s = b.s AND w.v = b.v AND w.cost = b.cost{cut} GROUP BY b.s, b.v, b.cost")
