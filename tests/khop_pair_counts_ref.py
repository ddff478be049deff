"""gg_khop_pair_counts restated in plain python integers (include/gg.h): the yardstick of the device kernels.

Lane i is sources[i] (every listed position its own lane; an id that is no vertex has no rows).  With w_0 = the indicator of
the lane's vertex and w_h(v) = the sum over the edge rows u -> v of w_{h-1}(u), w_h(v) is the number of h-walks from the
lane's source to v, wrapped mod 2^64 per level.  Level h has one row (lane, id(v), w_h(v)) per lane and vertex with a count
that is not 0 and — if there is a target list — an id in it; the filter never enters the recurrence.  Rows ascend by (lane,
dense index).  Built on tests/triangles_ref.TriangleGraph (su, dv: the kept edge rows as dense indices)."""
import numpy as np

M64 = 1 << 64
LANES = 64


def pair_counts(g, k_max: int, sources, targets=None) -> dict:
    """{"rows": {h: (src_index int64, ids int64, walks list of ints)} for h = 1..k_max, "entries_pulled",
    "rows_gathered"}.  sources: any number of ids (the device call takes 64 a batch; the statistics are summed the way
    GG.khop_pair_counts sums them: every batch of 64 runs its own k_max passes)."""
    sources = [int(s) for s in np.asarray(sources, np.int64).reshape(-1).tolist()]
    allowed = None
    if targets is not None:
        allowed = {g.index[int(t)] for t in np.asarray(targets, np.int64).reshape(-1).tolist() if int(t) in g.index}
    E = int(g.su.size)
    outdeg = np.diff(g.off).tolist()
    out_rows = {}  # u -> [(v, number of edge rows u -> v)], made on first use

    def out_row(u):
        if u not in out_rows:
            vs = np.nonzero(g.A[u])[0]
            out_rows[u] = list(zip(vs.tolist(), g.A[u, vs].tolist()))
        return out_rows[u]

    per_lane = []  # per lane: {h: {dense: walks}}
    entries_pulled = rows_gathered = 0
    for base in range(0, len(sources), LANES):
        batch = sources[base:base + LANES]
        state = [{g.index[s]: 1} if s in g.index else {} for s in batch]  # per lane: dense -> count, the non-zero ones
        levels = [dict() for _ in batch]
        for h in range(1, k_max + 1):
            if E:
                entries_pulled += E
                alive = set()
                for w in state:
                    alive.update(w)
                rows_gathered += sum(outdeg[u] for u in alive)  # the entries u -> v with any lane of w_{h-1}(u) alive
            nxt = []
            for lane, w in enumerate(state):
                n = {}
                for u, c in w.items():
                    for v, mult in out_row(u):
                        n[v] = n.get(v, 0) + c * mult
                n = {v: c % M64 for v, c in n.items() if c % M64}
                nxt.append(n)
                levels[lane][h] = n
            state = nxt
        per_lane += levels
    rows = {}
    for h in range(1, k_max + 1):
        idx, ids, walks = [], [], []
        for lane, lv in enumerate(per_lane):
            for v in sorted(lv[h]):
                if allowed is None or v in allowed:
                    idx.append(lane), ids.append(int(g.vid[v])), walks.append(lv[h][v])
        rows[h] = (np.array(idx, np.int64), np.array(ids, np.int64), walks)
    return {"rows": rows, "entries_pulled": entries_pulled, "rows_gathered": rows_gathered}


def group_walk_rows(g, sources, hops: int, walks_fn) -> tuple:
    """brute force: per listed source the group-by over its dense walk rows (walks_fn: tests/edge_filter_ref.walks);
    the same triple as pair_counts()["rows"][hops], without targets"""
    idx, ids, walks = [], [], []
    for lane, s in enumerate(np.asarray(sources, np.int64).reshape(-1).tolist()):
        rows = walks_fn(g, [s], hops)
        cnt = np.bincount(rows[:, -1], minlength=g.V) if rows.shape[0] else np.zeros(g.V, np.int64)
        for v in np.nonzero(cnt)[0].tolist():
            idx.append(lane), ids.append(int(g.vid[v])), walks.append(int(cnt[v]))
    return np.array(idx, np.int64), np.array(ids, np.int64), walks


def same(a, b) -> bool:
    """two (src_index, ids, walks) triples hold the same rows in the same order"""
    return (np.array_equal(np.asarray(a[0], np.int64), np.asarray(b[0], np.int64))
            and np.array_equal(np.asarray(a[1], np.int64), np.asarray(b[1], np.int64))
            and [int(x) for x in a[2]] == [int(x) for x in b[2]])


def filtered(rows, g, targets) -> tuple:
    """the rows of a triple whose end vertex is listed"""
    allowed = {int(t) for t in np.asarray(targets, np.int64).reshape(-1).tolist() if int(t) in g.index}
    keep = [i for i, v in enumerate(np.asarray(rows[1]).tolist()) if v in allowed]
    return (np.asarray(rows[0], np.int64)[keep], np.asarray(rows[1], np.int64)[keep], [int(rows[2][i]) for i in keep])


def sql_pair_counts(h: int, sources=None, targets=None) -> str:
    """the chain person p0, knows k1, person p1, ... with count(*) GROUP BY p0.p_personid, p_h.p_personid over tables
    person(p_personid) and knows — the pair form of benchmark/ldbc/queries/bi-14.sql:103-112.  sources / targets: distinct
    ids as IN lists (an IN list does not multiply); None: every person."""
    frm, cond = ["person p0"], []
    for i in range(1, h + 1):
        frm += [f"knows k{i}", f"person p{i}"]
        cond += [f"p{i - 1}.p_personid = k{i}.k_person1id", f"k{i}.k_person2id = p{i}.p_personid"]
    if sources is not None:
        cond.append("p0.p_personid IN (" + ", ".join(str(int(s)) for s in sources) + ")")
    if targets is not None:
        cond.append(f"p{h}.p_personid IN (" + ", ".join(str(int(t)) for t in targets) + ")")
    return (f"SELECT p0.p_personid, p{h}.p_personid, count(*) FROM {', '.join(frm)} WHERE " + " AND ".join(cond)
            + f" GROUP BY p0.p_personid, p{h}.p_personid")
