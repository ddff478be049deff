"""gg_result_filter_edge restated in plain numpy (include/gg.h): the yardstick of the device kernel.

Walk rows v0..vh are filtered by the number m of kept edge rows v_from -> v_to of a condition graph: inner repeats the row
m times, semi keeps it if m > 0, anti keeps it if m == 0; the input's order is kept.  An id that is no vertex of the
condition graph has m = 0.  Built on tests/triangles_ref.TriangleGraph: A[u, v] = number of edge rows u -> v, nbr / off =
the out-rows in edge-row order."""
import numpy as np

MODES = ("inner", "semi", "anti")


def walks(g, sources, hops: int) -> np.ndarray:
    """Dense walk rows [N, hops + 1] of g by repeated expansion in CSR order.  sources: ids, with multiplicity, ids that
    are no vertices contribute nothing; None: every vertex."""
    if sources is None:
        starts = np.arange(g.V, dtype=np.int64)
    else:
        starts = np.array([g.index[int(s)] for s in np.asarray(sources, np.int64).tolist() if int(s) in g.index], np.int64)
    rows = starts.reshape(-1, 1)
    for _ in range(hops):
        last = rows[:, -1]
        deg = g.off[last + 1] - g.off[last]
        parent = np.repeat(np.arange(rows.shape[0]), deg)
        within = np.arange(int(deg.sum())) - np.repeat(np.cumsum(deg) - deg, deg)
        child = g.nbr[np.repeat(g.off[last], deg) + within]
        rows = np.concatenate([rows[parent], child.reshape(-1, 1)], axis=1)
    return rows


def dense_of(index_f: dict, ids: np.ndarray) -> np.ndarray:
    """dense index in the condition graph of every id, -1 for ids it does not know"""
    ids = np.asarray(ids, np.int64)
    if not index_f or ids.size == 0:
        return np.full(ids.shape, -1, np.int64)
    keys = np.array(sorted(index_f), np.int64)
    vals = np.array([index_f[int(k)] for k in keys.tolist()], np.int64)
    at = np.clip(np.searchsorted(keys, ids), 0, keys.size - 1)
    return np.where(keys[at] == ids, vals[at], -1)


def multiplicity(id_rows: np.ndarray, A_f: np.ndarray, index_f: dict, from_col: int, to_col: int) -> np.ndarray:
    """m per row: A_f[dense(v_from), dense(v_to)], 0 where either id is unknown to the condition graph"""
    id_rows = np.asarray(id_rows, np.int64)
    u, t = dense_of(index_f, id_rows[:, from_col]), dense_of(index_f, id_rows[:, to_col])
    ok = (u >= 0) & (t >= 0)
    m = np.zeros(id_rows.shape[0], np.int64)
    if ok.any():
        m[ok] = A_f[u[ok], t[ok]]
    return m


def filter_rows(id_rows: np.ndarray, A_f: np.ndarray, index_f: dict, from_col: int, to_col: int, mode: str):
    """(the rows repeated, kept or dropped, in input order; stats as gg_edge_filter_stats reports them)"""
    assert mode in MODES
    id_rows = np.asarray(id_rows, np.int64)
    m = multiplicity(id_rows, A_f, index_f, from_col, to_col)
    out = np.repeat(id_rows, m, axis=0) if mode == "inner" else id_rows[(m > 0) if mode == "semi" else (m == 0)]
    return out, {"rows_in": int(id_rows.shape[0]), "rows_out": int(out.shape[0]), "matches": int(m.sum())}


def filter_graph(g, id_rows, from_col: int, to_col: int, mode: str):
    """filter_rows with g (a TriangleGraph) as the condition graph"""
    return filter_rows(id_rows, g.A, g.index, from_col, to_col, mode)


# ---- the row digest (DESIGN.md "Row digest"), vectorised: tests/oracle_lib.Oracle.digest_rows hashes row by row in
# python, which a table of a million rows cannot afford; tests/test_edge_filter_ref_cpu.py pins the two to each other
_GOLD, _K32 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0x9E3779B1)


def _fmix64(x):
    x = x ^ (x >> np.uint64(33))
    x = x * np.uint64(0xFF51AFD7ED558CCD)
    x = x ^ (x >> np.uint64(33))
    x = x * np.uint64(0xC4CEB9FE1A85EC53)
    return x ^ (x >> np.uint64(33))


def digest_dense_rows(dense_rows: np.ndarray) -> int:
    """sum mod 2^32 of the low halves of the row hashes of dense rows [N, h + 1]"""
    d = np.asarray(dense_rows).astype(np.uint64)
    if d.shape[0] == 0:
        return 0
    with np.errstate(over="ignore"):
        p = d[:, 0].copy()
        for j in range(1, d.shape[1]):
            p = _fmix64(p + _GOLD * np.uint64(j)) ^ (d[:, j] * _K32)
        return int((p & np.uint64(0xFFFFFFFF)).sum(dtype=np.uint64) & np.uint64(0xFFFFFFFF))


# ---- the yardstick statements over person / knows: every walk endpoint a row of person (hard_graph has dangling rows)
def _chain(hops: int):
    frm, cond = ["person p0"], []
    for i in range(1, hops + 1):
        frm += [f"knows k{i}", f"person p{i}"]
        cond += [f"p{i - 1}.p_personid = k{i}.k_person1id", f"k{i}.k_person2id = p{i}.p_personid"]
    return frm, cond


def _sources(sources):
    return [] if sources is None else ["p0.p_personid IN (" + ", ".join(str(int(s)) for s in sources) + ")"]


def select_list(hops: int) -> str:
    return ", ".join(f"p{i}.p_personid" for i in range(hops + 1))


def sql_closed_walks(k: int, sources=None, select: str | None = None) -> str:
    """the k-join statement `knows k1, ..., knows kk WHERE k1.dst = k2.src AND ... AND kk.dst = k1.src` with v0 from a list
    of distinct ids (None: every person): rows (v0..v_{k-1}), one per choice of the k edge rows"""
    frm, cond = _chain(k - 1)
    frm.append(f"knows k{k}")
    cond += [f"p{k - 1}.p_personid = k{k}.k_person1id", f"k{k}.k_person2id = p0.p_personid"]
    return (f"SELECT {select or select_list(k - 1)} FROM {', '.join(frm)} WHERE " + " AND ".join(cond + _sources(sources)))


def sql_exists(hops: int, from_col: int, to_col: int, negate: bool, sources=None, select: str | None = None) -> str:
    """the `hops`-hop walks from a list of distinct ids with [NOT] EXISTS (knows v_from -> v_to): negate with hops = 2,
    from 0, to 2 is the subquery shape of benchmark/ldbc/queries/interactive-complex-10.sql:19-24, the plain form that of
    interactive-complex-7.sql:5"""
    frm, cond = _chain(hops)
    sub = (f"{'NOT ' if negate else ''}EXISTS (SELECT * FROM knows kx WHERE kx.k_person1id = p{from_col}.p_personid "
           f"AND kx.k_person2id = p{to_col}.p_personid)")
    return (f"SELECT {select or select_list(hops)} FROM {', '.join(frm)} WHERE "
            + " AND ".join(cond + _sources(sources) + [sub]))
