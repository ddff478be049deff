"""gg_khop_aggregate restated in plain python integers (include/gg.h): the yardstick of the device kernel.

The result is GROUP BY over the h-hop walk table: per level h one row (vertex id, walks, total) per group.  With
a_0(v) = (1, weight(v)) and a_h(u) = the sum over the edge rows u -> v of a_{h-1}(v), a_h(u) is (count, sum of the end
vertices' weights) over the h-walks from u; over the transposed rows it is (count, sum of the start vertices' weights) over
the h-walks into u.  A source list seeds level 0 with its multiplicities for "end" and multiplies the final value for
"start".  walks wraps mod 2^64, total mod 2^128 (two's complement); a group exists iff its wrapped count is not 0; the
groups of a level come in dense (vertex-table) order.  Built on tests/triangles_ref.TriangleGraph (su, dv: the kept edge
rows as dense indices)."""
import numpy as np

GROUPS = ("start", "end")
M64, M128 = 1 << 64, 1 << 128


def wrap128(t: int) -> int:
    """t mod 2^128 as a two's-complement value"""
    t %= M128
    return t - M128 if t >= M128 >> 1 else t


def multiplicity(g, sources):
    """how often every dense index is listed (None: once each); ids that are no vertices contribute nothing"""
    if sources is None:
        return [1] * g.V
    m = [0] * g.V
    for s in np.asarray(sources, np.int64).reshape(-1).tolist():
        if int(s) in g.index:
            m[g.index[int(s)]] += 1
    return m


def aggregate(g, k_max: int, group_by: str, sources=None, weights=None) -> dict:
    """{h: (ids int64 array, walks list of ints, totals list of ints)} for h = 1..k_max"""
    assert group_by in GROUPS
    w = [1] * g.V if weights is None else [int(x) for x in np.asarray(weights).tolist()]
    assert len(w) == g.V
    m = multiplicity(g, sources)
    su, dv = g.su.tolist(), g.dv.tolist()
    if group_by == "start":
        cnt, tot = [1] * g.V, list(w)
        into, frm = su, dv  # a_h(u) += a_{h-1}(v) for every edge row u -> v
    else:
        cnt, tot = list(m), [a * b for a, b in zip(m, w)]
        into, frm = dv, su  # a_h(v) += a_{h-1}(u)
    out = {}
    for h in range(1, k_max + 1):
        ncnt, ntot = [0] * g.V, [0] * g.V
        for a, b in zip(into, frm):
            ncnt[a] += cnt[b]
            ntot[a] += tot[b]
        cnt, tot = ncnt, ntot
        if group_by == "start":
            fc, ft = [a * b for a, b in zip(m, cnt)], [a * b for a, b in zip(m, tot)]
        else:
            fc, ft = cnt, tot
        fc = [c % M64 for c in fc]
        keep = [i for i in range(g.V) if fc[i]]
        out[h] = (g.vid[keep] if keep else np.empty(0, np.int64), [fc[i] for i in keep], [wrap128(ft[i]) for i in keep])
    return out


def group_rows(g, dense_walks: np.ndarray, group_by: str, weights=None) -> tuple:
    """brute force: the group-by over dense walk rows [N, h + 1]; same triple as aggregate()[h]"""
    rows = np.asarray(dense_walks, np.int64)
    assert rows.shape[0] < 1 << 31  # the sums of 32-bit halves below stay inside int64
    w = np.ones(g.V, np.int64) if weights is None else np.asarray(weights, np.int64)
    key, val = (rows[:, 0], rows[:, -1]) if group_by == "start" else (rows[:, -1], rows[:, 0])
    cnt = np.bincount(key, minlength=g.V)
    lo, hi = np.zeros(g.V, np.int64), np.zeros(g.V, np.int64)
    np.add.at(lo, key, w[val] & 0xFFFFFFFF)  # the weights in an unsigned low and a signed high half, summed apart
    np.add.at(hi, key, w[val] >> 32)
    keep = np.nonzero(cnt)[0].tolist()
    return (g.vid[keep] if keep else np.empty(0, np.int64), [int(cnt[k]) for k in keep],
            [wrap128((int(hi[k]) << 32) + int(lo[k])) for k in keep])


def same(a, b) -> bool:
    """two (ids, walks, totals) triples hold the same rows in the same order"""
    return (np.array_equal(np.asarray(a[0], np.int64), np.asarray(b[0], np.int64))
            and [int(x) for x in a[1]] == [int(x) for x in b[1]] and [int(x) for x in a[2]] == [int(x) for x in b[2]])


def sql_khop_aggregate(h: int, group_by: str, sources=None, weighted: bool = True) -> str:
    """the chain person p0, knows k1, person p1, ... with count(*), sum(p?.p_score) GROUP BY one end, over tables
    person(p_personid, p_score) and knows — the shape of benchmark/ldbc/queries/bi-8.sql:41-53.  sources: distinct ids (an
    IN list does not multiply); None: every person.  Without weights the total is the count."""
    assert group_by in GROUPS
    frm, cond = ["person p0"], []
    for i in range(1, h + 1):
        frm += [f"knows k{i}", f"person p{i}"]
        cond += [f"p{i - 1}.p_personid = k{i}.k_person1id", f"k{i}.k_person2id = p{i}.p_personid"]
    if sources is not None:
        cond.append("p0.p_personid IN (" + ", ".join(str(int(s)) for s in sources) + ")")
    key, val = (0, h) if group_by == "start" else (h, 0)
    total = f"sum(p{val}.p_score)" if weighted else "sum(1)"
    return (f"SELECT p{key}.p_personid, count(*), {total} FROM {', '.join(frm)} WHERE " + " AND ".join(cond)
            + f" GROUP BY p{key}.p_personid")
