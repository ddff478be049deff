"""gg_result_group_tuples restated in numpy and Python ints (include/gg.h): the yardstick of the device kernels.

GROUP BY the columns `cols` of the rows of a walk table, cells compared as raw int64 values.  One output row per distinct
tuple, in input order of the tuples' first rows (tests/distinct_ref.py's rows and order), with count(*), count(x), sum(x)
mod 2^128 split into (lo, hi), min(x) and max(x) over the value of a row (tests/value_rows_ref.row_values); a group
without a valued row reports 0 for sum, min and max.  The count form (value_col None) reports 0 in every value column."""
import numpy as np

from tests import value_rows_ref as R

MASK64, MASK128 = (1 << 64) - 1, (1 << 128) - 1


def split128(total: int):
    """a Python int mod 2^128 as (lo uint64, hi int64) in two's complement"""
    t = total & MASK128
    lo, hi = t & MASK64, t >> 64
    return lo, hi - (1 << 64) if hi >= 1 << 63 else hi


def group_tuples(rows, cols, value_col=None, vertex_ids=None, values=None, valid=None):
    """({"keys" [G, len(cols)], "rows", "valued" uint64 [G], "sum": Python ints mod 2^128 read as signed, "lo" uint64,
    "hi" int64, "min", "max" int64 [G]}, stats without slots, probe_steps and route, which are the device's business)"""
    rows = np.asarray(rows, np.int64)
    cols = [int(c) for c in cols]
    assert rows.ndim == 2 and 1 <= len(cols) <= rows.shape[1] and len(set(cols)) == len(cols)
    N = rows.shape[0]
    chosen = rows[:, cols]
    if value_col is None:
        has, x = np.zeros(N, bool), np.zeros(N, np.int64)
    else:
        has, x = R.row_values(rows, value_col, vertex_ids, values, valid)
    if N == 0:
        first, inverse = np.empty(0, np.int64), np.empty(0, np.int64)
    else:
        _, first, inverse = np.unique(chosen, axis=0, return_index=True, return_inverse=True)
        order = np.argsort(first, kind="stable")  # sorted tuple number -> place in first-occurrence order
        place = np.empty(order.size, np.int64)
        place[order] = np.arange(order.size)
        first, inverse = first[order], place[np.asarray(inverse).reshape(-1)]
    G = first.size
    n_rows = np.bincount(inverse, minlength=G).astype(np.uint64)
    n_valued = np.bincount(inverse[has], minlength=G).astype(np.uint64)
    mn, mx = np.full(G, np.iinfo(np.int64).max, np.int64), np.full(G, np.iinfo(np.int64).min, np.int64)
    np.minimum.at(mn, inverse[has], x[has])
    np.maximum.at(mx, inverse[has], x[has])
    mn[n_valued == 0] = 0
    mx[n_valued == 0] = 0
    totals = [0] * G
    for g, v in zip(inverse[has].tolist(), x[has].tolist()):
        totals[g] += v
    halves = [split128(t) for t in totals]
    sums = np.empty(G, object)
    sums[:] = [(hi << 64) + lo for lo, hi in halves]
    out = {"keys": chosen[first].reshape(G, len(cols)), "rows": n_rows, "valued": n_valued, "sum": sums,
           "lo": np.array([h[0] for h in halves], np.uint64), "hi": np.array([h[1] for h in halves], np.int64),
           "min": mn, "max": mx}
    return out, {"rows_in": int(N), "rows_valued": int(has.sum()), "groups": int(G)}


def group_tuples_brute(rows, cols, value_col=None, vertex_ids=None, values=None, valid=None):
    """the same by a python loop over a dict (small inputs); the value of a row by a dict of the vertex table"""
    rows = np.asarray(rows, np.int64)
    where = {} if vertex_ids is None else {int(v): i for i, v in enumerate(np.asarray(vertex_ids, np.int64).tolist())}
    ok = None if valid is None else R.valid_bits(valid, len(where))
    groups, valued_rows = {}, 0
    for r in rows.tolist():
        t = tuple(r[c] for c in cols)
        g = groups.setdefault(t, {"rows": 0, "xs": []})
        g["rows"] += 1
        if value_col is not None:
            d = where.get(r[value_col])
            if d is not None and (ok is None or ok[d]):
                g["xs"].append(int(values[d]))
                valued_rows += 1
    G = len(groups)
    halves = [split128(sum(g["xs"])) for g in groups.values()]
    sums = np.empty(G, object)
    sums[:] = [(hi << 64) + lo for lo, hi in halves]
    out = {"keys": np.array([list(t) for t in groups], np.int64).reshape(G, len(cols)),
           "rows": np.array([g["rows"] for g in groups.values()], np.uint64),
           "valued": np.array([len(g["xs"]) for g in groups.values()], np.uint64), "sum": sums,
           "lo": np.array([h[0] for h in halves], np.uint64), "hi": np.array([h[1] for h in halves], np.int64),
           "min": np.array([min(g["xs"]) if g["xs"] else 0 for g in groups.values()], np.int64),
           "max": np.array([max(g["xs"]) if g["xs"] else 0 for g in groups.values()], np.int64)}
    return out, {"rows_in": int(rows.shape[0]), "rows_valued": valued_rows, "groups": G}


def same(a: dict, b: dict) -> bool:
    """two answers agree in the keys, their order and all six aggregates ("lo" / "hi" only where both carry them)"""
    names = ["keys", "rows", "valued", "min", "max"] + [k for k in ("lo", "hi") if k in a and k in b]
    return (all(np.array_equal(a[k], b[k]) for k in names)
            and [int(s) for s in a["sum"]] == [int(s) for s in b["sum"]])
