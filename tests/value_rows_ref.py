"""gg_result_filter_value and gg_result_top_rows restated in plain numpy (include/gg.h): the yardstick of the device kernels.

The value of a row: its cell in value_col looked up in the id dictionary of the values' vertex table; the row has the
value values[d] iff the cell is vertex d and bit d of `valid` (uint64 words, None: every bit) is set.  A row without a value
passes no predicate.  Each function has a python-loop twin for small inputs."""
import numpy as np

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
SIGN = np.uint64(1 << 63)


def valid_bits(valid, V: int) -> np.ndarray:
    """bool per vertex"""
    if valid is None:
        return np.ones(V, bool)
    words = np.asarray(valid, np.uint64)
    assert words.size == (V + 63) // 64
    i = np.arange(V, dtype=np.uint64)
    return ((words[(i >> np.uint64(6)).astype(np.int64)] >> (i & np.uint64(63))) & np.uint64(1)).astype(bool)


def pack_valid(bits) -> np.ndarray:
    """bool per vertex -> ceil(V / 64) uint64 words"""
    bits = np.asarray(bits, bool)
    words = np.zeros((bits.size + 63) // 64, np.uint64)
    for i in np.nonzero(bits)[0].tolist():
        words[i >> 6] |= np.uint64(1 << (i & 63))
    return words


def row_values(table, value_col: int, vertex_ids, values, valid=None):
    """(has [N] bool, x [N] int64; x is 0 where the row has no value)"""
    table = np.asarray(table, np.int64)
    vertex_ids, values = np.asarray(vertex_ids, np.int64), np.asarray(values, np.int64)
    N = table.shape[0]
    if N == 0 or vertex_ids.size == 0:
        return np.zeros(N, bool), np.zeros(N, np.int64)
    cells = table[:, value_col]
    order = np.argsort(vertex_ids, kind="stable")
    keys = vertex_ids[order]
    at = np.clip(np.searchsorted(keys, cells), 0, keys.size - 1)
    d = order[at]
    has = (keys[at] == cells) & valid_bits(valid, vertex_ids.size)[d]
    return has, np.where(has, values[d], 0).astype(np.int64)


def passes(has, x, lo: int, hi: int, mode: str):
    inside = (x >= np.int64(max(lo, I64_MIN))) & (x <= np.int64(min(hi, I64_MAX)))
    return has & (inside if mode == "in" else ~inside)


def filter_rows(table, edge_cols, value_col, vertex_ids, values, valid, lo, hi, mode):
    """(rows in input order, their edge columns (None if edge_cols is None), stats as gg_value_filter_stats)"""
    table = np.asarray(table, np.int64)
    has, x = row_values(table, value_col, vertex_ids, values, valid)
    keep = passes(has, x, lo, hi, mode)
    stats = {"rows_in": int(table.shape[0]), "rows_valued": int(has.sum()), "rows_out": int(keep.sum())}
    return table[keep], None if edge_cols is None else np.asarray(edge_cols, np.int64)[keep], stats


def order_key(x, descending: bool) -> np.ndarray:
    """the value as the unsigned word in which smaller is better: sign bit flipped, complemented (never negated:
    INT64_MIN must order correctly) if descending"""
    k = np.asarray(x, np.int64).view(np.uint64) ^ SIGN
    return ~k if descending else k


def top_rows(table, edge_cols, value_col, vertex_ids, values, valid, lo, hi, mode, descending, tie_col, n):
    """(rows in rank order, their edge columns, stats without select_passes / sort_route).  tie_col None: none."""
    table = np.asarray(table, np.int64)
    has, x = row_values(table, value_col, vertex_ids, values, valid)
    cand = np.nonzero(passes(has, x, lo, hi, mode))[0]
    tie = table[cand, tie_col] if tie_col is not None else np.zeros(cand.size, np.int64)
    order = np.lexsort((cand, tie, order_key(x[cand], descending)))  # last key first: value, tie id, row number
    pick = cand[order[: min(n, cand.size)]]
    stats = {"rows_in": int(table.shape[0]), "rows_valued": int(has.sum()), "candidates": int(cand.size),
             "rows_out": int(pick.size)}
    return table[pick], None if edge_cols is None else np.asarray(edge_cols, np.int64)[pick], stats


# ---- the python-loop twins
def row_values_loop(table, value_col, vertex_ids, values, valid=None):
    index = {}
    for d, v in enumerate(np.asarray(vertex_ids, np.int64).tolist()):
        index.setdefault(v, d)
    words = None if valid is None else [int(w) for w in np.asarray(valid, np.uint64).tolist()]
    vals = np.asarray(values, np.int64).tolist()
    out = []
    for r in np.asarray(table, np.int64).tolist():
        d = index.get(r[value_col])
        if d is None or (words is not None and not (words[d >> 6] >> (d & 63)) & 1):
            out.append(None)
        else:
            out.append(vals[d])
    return out


def passes_loop(x, lo, hi, mode):
    if x is None:
        return False
    return (lo <= x <= hi) if mode == "in" else (x < lo or x > hi)


def filter_rows_loop(table, edge_cols, value_col, vertex_ids, values, valid, lo, hi, mode):
    xs = row_values_loop(table, value_col, vertex_ids, values, valid)
    rows = np.asarray(table, np.int64).tolist()
    keep = [i for i, x in enumerate(xs) if passes_loop(x, lo, hi, mode)]
    width = np.asarray(table).shape[1]
    out = np.array([rows[i] for i in keep], np.int64).reshape(-1, width)
    e = None
    if edge_cols is not None:
        ec = np.asarray(edge_cols, np.int64)
        e = np.array([ec[i].tolist() for i in keep], np.int64).reshape(-1, ec.shape[1])
    return out, e, {"rows_in": len(rows), "rows_valued": sum(x is not None for x in xs), "rows_out": len(keep)}


def top_rows_loop(table, edge_cols, value_col, vertex_ids, values, valid, lo, hi, mode, descending, tie_col, n):
    xs = row_values_loop(table, value_col, vertex_ids, values, valid)
    rows = np.asarray(table, np.int64).tolist()
    cand = [i for i, x in enumerate(xs) if passes_loop(x, lo, hi, mode)]
    cand.sort(key=lambda i: (-xs[i] if descending else xs[i], rows[i][tie_col] if tie_col is not None else 0, i))
    pick = cand[: min(n, len(cand))]
    width = np.asarray(table).shape[1]
    out = np.array([rows[i] for i in pick], np.int64).reshape(-1, width)
    e = None
    if edge_cols is not None:
        ec = np.asarray(edge_cols, np.int64)
        e = np.array([ec[i].tolist() for i in pick], np.int64).reshape(-1, ec.shape[1])
    return out, e, {"rows_in": len(rows), "rows_valued": sum(x is not None for x in xs), "candidates": len(cand),
                    "rows_out": len(pick)}
