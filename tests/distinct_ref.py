"""gg_result_distinct restated in plain numpy (include/gg.h): the yardstick of the device kernels.

SELECT DISTINCT over the columns `cols` of the rows of a walk table: cells are compared as raw int64 values, the output
holds one row per distinct tuple — the first input row that holds it — with the chosen columns in their chosen order, and
the rows keep the input's order."""
import numpy as np


def distinct_rows(rows, cols):
    """(rows [M, len(cols)] in input order, the input row numbers of those rows, stats as gg_distinct_stats reports them
    but for slots and probe_steps, which are the device's business)"""
    rows = np.asarray(rows, np.int64)
    cols = [int(c) for c in cols]
    assert rows.ndim == 2 and 1 <= len(cols) <= rows.shape[1] and len(set(cols)) == len(cols)
    assert all(0 <= c < rows.shape[1] for c in cols)
    chosen = rows[:, cols]
    if rows.shape[0] == 0:
        return chosen.reshape(0, len(cols)), np.empty(0, np.int64), {"rows_in": 0, "rows_out": 0}
    _, first = np.unique(chosen, axis=0, return_index=True)  # (the index of the FIRST occurrence of every tuple)
    first = np.sort(first)
    return chosen[first], first.astype(np.int64), {"rows_in": int(rows.shape[0]), "rows_out": int(first.size)}


def distinct_rows_brute(rows, cols):
    """the same by a python loop over a dict (small inputs)"""
    seen, out, at = {}, [], []
    for i, r in enumerate(np.asarray(rows, np.int64).tolist()):
        t = tuple(r[c] for c in cols)
        if t not in seen:
            seen[t] = i
            out.append(list(t))
            at.append(i)
    return (np.array(out, np.int64).reshape(-1, len(cols)), np.array(at, np.int64),
            {"rows_in": len(rows), "rows_out": len(out)})
