"""gg_result_group_by restated in plain numpy / python integers (include/gg.h): the yardstick of the device kernels.

The rows of a walk table are grouped by one column whose cells are looked up among the ids of the key's table (in
vertex-table order): a row whose key is no such id forms no group.  Per group: walks = its rows, total = the sum of
weights[position of the weight cell among the weight table's ids] (a cell that is no such id weighs 0), wrapped to 128
bits two's complement; without weights total = walks.  Groups ascend by the key's position in the key's table."""
import numpy as np

from tests import khop_aggregate_ref as K


def _positions(ids: np.ndarray, cells: np.ndarray) -> np.ndarray:
    """position of every cell among ids (distinct), -1 if absent"""
    ids, cells = np.asarray(ids, np.int64), np.asarray(cells, np.int64)
    if ids.size == 0 or cells.size == 0:
        return np.full(cells.shape, -1, np.int64)
    order = np.argsort(ids, kind="stable")
    at = np.clip(np.searchsorted(ids[order], cells), 0, ids.size - 1)
    return np.where(ids[order][at] == cells, order[at], -1).astype(np.int64)


def group_by(table, key_col: int, key_ids, weight_col=None, weight_ids=None, weights=None):
    """((ids int64 array, walks list of ints, totals list of ints), stats without "route").  table: id rows [N, h + 1];
    key_ids / weight_ids (None: key_ids): the tables' ids in vertex-table order; weights: one integer per weight id."""
    table = np.asarray(table, np.int64)
    key_ids = np.asarray(key_ids, np.int64)
    n = table.shape[0]
    u = _positions(key_ids, table[:, key_col]) if n else np.empty(0, np.int64)
    live = u >= 0
    keys, inverse, counts = np.unique(u[live], return_inverse=True, return_counts=True)
    walks = [int(c) for c in counts.tolist()]
    if weight_col is None:
        assert weights is None
        totals = list(walks)
    else:
        wids = key_ids if weight_ids is None else np.asarray(weight_ids, np.int64)
        w = [int(x) for x in np.asarray(weights).tolist()]
        assert len(w) == wids.size
        wv = _positions(wids, table[:, weight_col])[live] if n else np.empty(0, np.int64)
        sums = [0] * keys.size
        for g, v in zip(inverse.tolist(), wv.tolist()):
            if v >= 0:
                sums[g] += w[v]
        totals = [K.wrap128(s) for s in sums]
    stats = {"rows_in": int(n), "rows_grouped": int(live.sum()), "groups": int(keys.size)}
    return (key_ids[keys], walks, totals), stats


def group_by_brute(table, key_col: int, key_ids, weight_col=None, weight_ids=None, weights=None):
    """the same by python loops and dictionaries (small inputs)"""
    key_ids = [int(x) for x in np.asarray(key_ids, np.int64).tolist()]
    wids = key_ids if weight_ids is None else [int(x) for x in np.asarray(weight_ids, np.int64).tolist()]
    kpos = {v: i for i, v in enumerate(key_ids)}
    wpos = {v: i for i, v in enumerate(wids)}
    w = None if weights is None else [int(x) for x in np.asarray(weights).tolist()]
    cnt, tot, grouped = {}, {}, 0
    rows = np.asarray(table, np.int64).tolist()
    for r in rows:
        if r[key_col] not in kpos:
            continue
        k = kpos[r[key_col]]
        grouped += 1
        cnt[k] = cnt.get(k, 0) + 1
        if weight_col is None:
            add = 1
        else:
            add = w[wpos[r[weight_col]]] if r[weight_col] in wpos else 0
        tot[k] = tot.get(k, 0) + add
    order = sorted(cnt)
    level = (np.array([key_ids[k] for k in order], np.int64), [cnt[k] for k in order], [K.wrap128(tot[k]) for k in order])
    return level, {"rows_in": len(rows), "rows_grouped": grouped, "groups": len(order)}


def hub_weights(ids, hub: int, seed: int = 0x6B0):
    """one int64 weight per id: mostly small and of both signs, some of the extremes +-(2^63 - 1) and -2^63, and -2^63 on
    the hub — a few hundred rows of which carry the low half past 2^64 many times and leave the high half negative"""
    ids = np.asarray(ids, np.int64)
    rng = np.random.RandomState(seed)
    w = rng.randint(-1000, 1000, ids.size).astype(np.int64)
    big = np.array([np.iinfo(np.int64).max, -np.iinfo(np.int64).max, np.iinfo(np.int64).min], np.int64)
    at = rng.choice(ids.size, max(ids.size // 8, 3), replace=False)
    w[at] = big[np.arange(at.size) % 3]
    w[np.nonzero(ids == hub)[0]] = np.iinfo(np.int64).min
    return w


def sql_extend_group(hops: int, from_col: int, key_col: int, sources, n=None) -> str:
    """count(*) per value of column key_col of the `hops`-hop walks joined with message on v_from_col = m_creatorid
    (column hops + 1 is m_messageid), in the order the table function gives: ORDER BY 2 DESC, 1 [LIMIT n] — the tail of
    benchmark/ldbc/queries/interactive-complex-4.sql:1-22 with the key's id in the place of the tag's name"""
    from tests import extend_ref as X

    key = "m.m_messageid" if key_col == hops + 1 else f"p{key_col}.p_personid"
    sql = X.sql_extend(hops, from_col, sources, select=f"{key}, count(*)") + " GROUP BY 1 ORDER BY 2 DESC, 1"
    return sql + (f" LIMIT {int(n)}" if n is not None else "")
