"""Triangle rows with the rowids of their three edges (include/gg.h, gg_triangles_edges), restated in plain numpy.

A row is a triple of staged edge rows e1: a -> b, e2: b -> c, e3: c -> a whose endpoints are all vertices, reported as
(a, b, c, e1, e2, e3): ids and rowids.  The rowid of an edge row is the one staged with it, or its append position
(dangling rows count) where none was staged.  The enumeration joins the edge rows themselves, by position — it does not
go through tests.triangles_ref.TriangleGraph.rows, which it is compared against."""
import numpy as np

from tests import triangles_ref as T


def _expand(left_key, right_sorted_key, right_order):
    """the join of left rows with the right rows of equal key: (left index, right position) of every match, left rows in
    order and the matches of one left row in the right side's original order"""
    lo = np.searchsorted(right_sorted_key, left_key, "left")
    hi = np.searchsorted(right_sorted_key, left_key, "right")
    m = hi - lo
    li = np.repeat(np.arange(left_key.size), m)
    within = np.arange(int(m.sum())) - np.repeat(np.cumsum(m) - m, m)
    return li, right_order[np.repeat(lo, m) + within]


def rows(vid, src, dst, rowid=None, order=0, sources=None):
    """[N, 6] int64 (a, b, c, e1, e2, e3).  order 1: only id(a) < id(b) < id(c).  sources: ids a ranges over, with
    multiplicity; ids that are no vertex contribute nothing; None: every vertex once."""
    vid, src, dst = (np.asarray(x, np.int64) for x in (vid, src, dst))
    rid = np.arange(src.size, dtype=np.int64) if rowid is None else np.asarray(rowid, np.int64)
    pos = np.flatnonzero(np.isin(src, vid) & np.isin(dst, vid))  # append positions of the kept rows
    s, d = src[pos], dst[pos]
    by_src = np.argsort(s, kind="stable")
    s_sorted = s[by_src]
    starts = vid if sources is None else np.asarray(sources, np.int64)
    starts = starts[np.isin(starts, vid)]
    _, i1 = _expand(starts, s_sorted, by_src)              # e1: a row leaving a start
    w1, i2 = _expand(d[i1], s_sorted, by_src)              # e2: a row leaving b
    i1 = i1[w1]
    # e3: a row c -> a, found by its (source, destination) pair, each id numbered by its place among the ids ascending
    sv = np.sort(vid)
    code = np.searchsorted(sv, s) * vid.size + np.searchsorted(sv, d)
    by_code = np.argsort(code, kind="stable")
    want = np.searchsorted(sv, d[i2]) * vid.size + np.searchsorted(sv, s[i1])
    w2, i3 = _expand(want, code[by_code], by_code)
    i1, i2 = i1[w2], i2[w2]
    out = np.stack([s[i1], s[i2], s[i3], rid[pos[i1]], rid[pos[i2]], rid[pos[i3]]], axis=1).astype(np.int64)
    if order == 1:
        out = out[(out[:, 0] < out[:, 1]) & (out[:, 1] < out[:, 2])]
    return out


def explicit_rowids(n):
    """injective and not monotone in append order"""
    return 10**12 - 3 * np.arange(n, dtype=np.int64)


def positions_of(rowid_cols, rowid=None):
    """append positions of rowids (explicit_rowids' inverse where `rowid` is given)"""
    if rowid is None:
        return rowid_cols
    back = {int(r): i for i, r in enumerate(np.asarray(rowid).tolist())}
    return np.vectorize(back.__getitem__, otypes=[np.int64])(rowid_cols) if rowid_cols.size else rowid_cols


def graph(n_dangling=50, seed=0xE3):
    """tests.triangles_ref.hard_graph() with n_dangling rows that touch no vertex inserted at seeded random places among
    its first thousand edge rows: append position, index among the kept rows and CSR position of an edge row all differ."""
    vid, src, dst = T.hard_graph()
    rng = np.random.RandomState(seed)
    at = np.sort(rng.randint(0, 1000, n_dangling))
    ghost = np.int64(int(vid.max()) + 1000) + np.arange(n_dangling, dtype=np.int64)
    inside = vid[rng.randint(0, vid.size, n_dangling)]
    flip = rng.randint(0, 2, n_dangling).astype(bool)  # dangling at the source or at the destination
    src = np.insert(src, at, np.where(flip, ghost, inside))
    dst = np.insert(dst, at, np.where(flip, inside, ghost))
    return vid, src, dst


def tiny_graph():
    """at most 6 vertices: a dangling row first, a 3-cycle 1 -> 2 -> 3 -> 1 with 2 -> 3 doubled, two parallel self-loops on
    4 (8 rows (4, 4, 4): every triple of the two rowids), and the 2-cycle 5 <-> 6 with a self-loop on 5"""
    vid = np.array([3, 1, 2, 6, 5, 4], np.int64)
    src = np.array([99, 1, 2, 3, 2, 4, 4, 5, 6, 5], np.int64)
    dst = np.array([1, 2, 3, 1, 3, 4, 4, 6, 5, 5], np.int64)
    return vid, src, dst
