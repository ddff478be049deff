"""gg_cheapest64_paths restated in plain python integers (include/gg.h), on top of tests/cheapest_ref.py: the yardstick of
the trace kernel.

The batch is cheapest(g, sources) at its fixpoint.  For lane s and a vertex x with hops h >= 1 and cost c < INT64_MAX,
pred(s, x) is the first kept edge row u -> x, in ascending (dense index of u, append order), with a cost at u in lane s,
cost(s, u) (+) w(row) == c and hops(s, u) == h - 1; that row is the step's edge.  The path of a pair is t, pred(s, t), ...
back to the source: one row (pair, step, vertex id, edge rowid or -1 at step 0, cost at the step's vertex) per step,
ascending by (pair, step).  The pair table lists (pair, cost, hops, traced) for every pair whose target has a cost; a
saturated pair (cost == INT64_MAX) is listed with traced = 0 and has no path rows.  entries_scanned adds, per step, the
rows of x's in-list up to and including the one taken."""
import numpy as np

from tests import cheapest_ref as CR

INT64_MAX = CR.INT64_MAX


class LostTrace(Exception):
    """a reached, unsaturated vertex without a qualifying in-row: impossible at the fixpoint"""


def in_rows(g) -> list:
    """per dense vertex x: its kept in-rows (u, weight, kept-row index) ascending by (u, append order)"""
    rin = [[] for _ in range(g.V)]
    for k in sorted(range(g.E), key=lambda k: (g.su[k], k)):
        rin[g.dv[k]].append((g.su[k], g.wk[k], k))
    return rin


def cells_of(state) -> dict:
    """{(lane, vertex id): (cost, hops)} of a cheapest() answer"""
    idx, ids, cost, hops = state["rows"]
    return {(int(l), int(v)): (int(c), int(h)) for l, v, c, h in zip(idx.tolist(), ids.tolist(), cost, hops)}


def paths(g, sources, pair_lane, pair_dst, rowid=None, edges: bool = True, state=None, max_hops: int = -1) -> dict:
    """{"rows": (pair, step, vertex, edge, cost), "pairs": (pair, cost, hops, traced), "pairs_reached", "pairs_saturated",
    "n_rows", "entries_scanned", "search"}.  sources: any number of ids, pair_lane indexes them (every batch of 64 is its own
    search, as GG.cheapest_path_lengths runs them); rowid: the edge rows' explicit rowids in append order (None: the append
    position); state: cheapest(g, sources) where the caller has it.  max_hops >= 0 is not part of the relation: it is here
    to show that a bounded state loses pairs (LostTrace)."""
    state = state or CR.cheapest(g, sources, max_hops)
    cells = cells_of(state)
    rin = in_rows(g)
    rows, table = [], []
    scanned = saturated = 0
    for p, (lane, t) in enumerate(zip(np.asarray(pair_lane).tolist(), np.asarray(pair_dst, np.int64).tolist())):
        if (int(lane), int(t)) not in cells:  # unreached, or the source or the target is no vertex
            continue
        c, h = cells[(int(lane), int(t))]
        traced = c < INT64_MAX
        table.append((p, c, h, int(traced)))
        if not traced:
            saturated += 1
            continue
        x = g.index[int(t)]
        back = []
        while h >= 1:
            for k, (u, w, r) in enumerate(rin[x]):
                cu = cells.get((int(lane), int(g.vid[u])))
                if cu is not None and min(cu[0] + w, INT64_MAX) == c and cu[1] == h - 1:
                    break
            else:
                raise LostTrace((p, int(g.vid[x]), c, h))
            scanned += k + 1
            edge = -1 if not edges else int(g.kept[r] if rowid is None else rowid[g.kept[r]])
            back.append((p, h, int(g.vid[x]), edge, c))
            x, (c, h) = u, cu
        back.append((p, 0, int(g.vid[x]), -1, c))
        rows.extend(reversed(back))
    return {"rows": _columns(rows, (np.int64, np.int32, np.int64, np.int64, None)),
            "pairs": _columns(table, (np.int64, None, np.int32, np.int32)),
            "pairs_reached": len(table), "pairs_saturated": saturated, "n_rows": len(rows), "entries_scanned": scanned,
            "search": {k: state[k] for k in ("rounds", "reached_pairs", "cells_lowered", "entries_pulled", "rows_gathered")}}


def _columns(rows, types):
    """tuples -> one column each: a numpy array, or (type None) a list of python integers"""
    cols = list(zip(*rows)) if rows else [()] * len(types)
    return tuple([int(x) for x in c] if t is None else np.array(c, t) for c, t in zip(cols, types))


def pair_paths(g, src, dst, rowid=None, edges: bool = True) -> dict:
    """paths() for pairs (src[i], dst[i]) of any number of sources, grouped as GG.cheapest_paths groups them"""
    uniq, inv = np.unique(np.asarray(src, np.int64), return_inverse=True)
    return paths(g, uniq, inv, dst, rowid, edges)


def same_rows(got, want) -> bool:
    """two column tuples hold the same rows in the same order (integer columns of any width)"""
    return len(got) == len(want) and all([int(x) for x in a] == [int(x) for x in b] for a, b in zip(got, want))


def id_rows(rows, src, dst) -> list:
    """path rows as sorted (src, dst, step, vertex, edge, cost) tuples, the edge of step 0 being -1 — what the SQL table
    function returns, its NULL edge read as -1"""
    s, d = np.asarray(src, np.int64).tolist(), np.asarray(dst, np.int64).tolist()
    return sorted((s[int(p)], d[int(p)], int(i), int(v), int(e), int(c))
                  for p, i, v, e, c in zip(*[list(col) for col in rows]))
