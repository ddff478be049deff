"""Vertex ids at the places where 64-bit ids go wrong, and one graph that carries them under every id dictionary.

EDGE_IDS are 24 int64 values around INT64_MIN, -2^32, -2^31, 0, 2^31, 2^32 and INT64_MAX.  Among them: ids whose low
32-bit half is 0xFFFFFFFF, the value the shared radix sort keeps for "no element" (-1, 2^32 - 1, 2^33 - 1,
INT64_MIN + 2^32 - 1, -2^32 - 1, 0x7FFFFFFEFFFFFFFF, INT64_MAX); ids whose high half with the sign bit flipped is
0xFFFFFFFF (0x7FFFFFFF00000000 and above); both at once (INT64_MAX — and -1, whose plain high half is); INT64_MIN, the
empty-slot key HT_EMPTY of the 16-byte id table; and groups that share a low half (0, 2^32, -2^32,
0x7FFFFFFF00000000) or a high half, so a compare or a lookup that drops a half collides.

edge_graph(kind) is tests/triangles_ref.hard_graph(V=200, rows=3000, hub_fan=80) — parallel rows, self-loops, a 2-cycle,
a hub, dangling rows — plus 24 vertices wired to each other in both directions (552 rows: each of them lies in
2 * C(23, 2) triangles of either orientation and in C(24, 3) = 2024 ordered ones together), six of which are also wired
to the hub; 224 vertices, about 2500 rows.  The vertex table is shuffled, so its order is not the id order.  PLACEMENTS
relabel it; which dictionary gg_csr_build then takes follows from dict_mode_of (csrc/gg_dict.h), which looks at the
smallest and the largest vertex id only.  The dictionary kind cannot be read back through the C-ABI: the rules below
were checked by reading dict_mode_of, not by a run.

  wide        the 24 are EDGE_IDS, the rest random 64-bit ids.  span = INT64_MAX - INT64_MIN = 2^64 - 1: not below
              DIRECT_MAX_RANGE (2^20), and span_bits = 64 > 57 fails packed_fits -> DICT_WIDE16, the 16-byte slots
              whose empty key is INT64_MIN, which is a vertex here (the min_idx slot).
  dense_zero  every id in [-300, 300): span < 2^20 -> DICT_DIRECT.  The window straddles -1 | 0.
  dense_u32   every id in [2^32 - 300, 2^32 + 300): DICT_DIRECT.  Straddles 2^32 - 1 | 2^32.
  dense_max   every id in [INT64_MAX - 599, INT64_MAX]: DICT_DIRECT.  The window ends exactly at INT64_MAX.
  dense_min   every id in [INT64_MIN, INT64_MIN + 600): DICT_DIRECT.  The window starts exactly at INT64_MIN.
  sparse      datagen.person_ids(224, 11) shifted by a constant so that the middle id is -1: the span (~2^40) is what
              tests/test_gpu_derived_reverse._ids("sparse") has -> DICT_PACKED8, 8-byte slots holding id - min.
In the dense windows 224 of the 600 values are vertices; the ids of the dangling rows are among the other 376, inside the
window, so the direct-address array is probed at cells that hold no vertex."""
import numpy as np

from tests import triangles_ref as T

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1

EDGE_IDS = np.array([
    I64_MIN, I64_MIN + 1, I64_MIN + (1 << 32) - 1,
    -(1 << 32) - 1, -(1 << 32), -(1 << 32) + 1,
    -(1 << 31) - 1, -(1 << 31),
    -2, -1, 0, 1,
    (1 << 31) - 1, 1 << 31,
    (1 << 32) - 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 33) - 1,
    0x7FFFFFFEFFFFFFFF, 0x7FFFFFFF00000000, 0x7FFFFFFF00000001, I64_MAX - 1, I64_MAX,
], dtype=np.int64)
N_EDGE = 24
assert EDGE_IDS.size == N_EDGE == np.unique(EDGE_IDS).size

PLACEMENTS = ["wide", "dense_zero", "dense_u32", "dense_max", "dense_min", "sparse"]
WINDOW = 600
# placement -> (first id of the dense window, offsets in it that the 24 wired vertices take)
_DENSE = {
    "dense_zero": (-300, range(300 - 12, 300 + 12)),
    "dense_u32": ((1 << 32) - 300, range(300 - 12, 300 + 12)),
    "dense_max": (I64_MAX - (WINDOW - 1), range(WINDOW - N_EDGE, WINDOW)),
    "dense_min": (I64_MIN, range(0, N_EDGE)),
}
# the edge values each placement is named for: they must be vertices
NAMED = {
    "wide": EDGE_IDS.tolist(),
    "dense_zero": [-2, -1, 0, 1],
    "dense_u32": [(1 << 32) - 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1],
    "dense_max": [I64_MAX - 1, I64_MAX],
    "dense_min": [I64_MIN, I64_MIN + 1],
    "sparse": [-1],
}
# the source list of the issue: four edge values and an id that is a vertex under no placement
NOT_A_VERTEX = 123_456_789_123
LISTED = np.array([-1, I64_MIN, I64_MAX, (1 << 32) - 1, NOT_A_VERTEX], np.int64)


def relabel(vid, src, dst, new_ids):
    """(vid, src, dst) with vid[i] -> new_ids[i] in all three arrays.  An id of src / dst that is no vertex (a dangling row)
    goes to an id that is no vertex of the new set: the distinct old ones, ascending, to the smallest values above
    min(new_ids) that are free — inside [min, max] of the new ids wherever that range has gaps."""
    vid, src, dst = (np.asarray(x, np.int64) for x in (vid, src, dst))
    new_ids = np.asarray(new_ids, np.int64)
    assert new_ids.size == vid.size == np.unique(new_ids).size == np.unique(vid).size
    to = dict(zip(vid.tolist(), new_ids.tolist()))
    taken = set(new_ids.tolist())
    strangers = sorted(set(src.tolist() + dst.tolist()) - set(vid.tolist()))
    free = int(new_ids.min())
    for old in strangers:
        while free in taken:
            free += 1
        assert free <= I64_MAX
        to[old] = free
        taken.add(free)
    m = np.vectorize(to.__getitem__, otypes=[np.int64])
    return new_ids.copy(), m(src), m(dst)


def base_graph():
    """(vid, src, dst, wired, hub) in hard_graph's small positive ids: the 24 wired vertices are `wired`"""
    vid, src, dst = T.hard_graph(V=200, rows=3000, hub_fan=80)
    g = T.TriangleGraph(vid, src, dst)
    hub = int(g.vid[np.bincount(g.dv, minlength=g.V).argmax()])
    first = int(max(vid.max(), src.max(), dst.max())) + 1000
    wired = first + 7 * np.arange(N_EDGE, dtype=np.int64)
    a, b = np.meshgrid(wired, wired, indexing="ij")
    off_diagonal = a != b
    ws, wd = a[off_diagonal], b[off_diagonal]                       # 552 rows: every ordered pair
    to_hub = wired[[0, 5, 9, 15, 19, 23]]
    hs = np.concatenate([to_hub, np.full(to_hub.size, hub, np.int64)])
    hd = np.concatenate([np.full(to_hub.size, hub, np.int64), to_hub])
    rng = np.random.RandomState(0xED6E)
    # the new rows go among the old ones, the new vertices among the old vertices
    src, dst = np.concatenate([src, ws, hs]), np.concatenate([dst, wd, hd])
    p = rng.permutation(src.size)
    vid = np.concatenate([vid, wired])
    return vid[rng.permutation(vid.size)], src[p], dst[p], wired, hub


class EdgeGraph:
    """vid, src, dst of one placement; wired: the ids of the 24 fully wired vertices; named: NAMED[kind]; hub"""

    def __init__(self, kind, vid, src, dst, wired, hub):
        self.kind, self.vid, self.src, self.dst, self.wired, self.hub = kind, vid, src, dst, wired, hub
        self.named = np.array(NAMED[kind], np.int64)
        for a in (self.vid, self.src, self.dst, self.wired, self.named):
            a.setflags(write=False)

    @property
    def tri(self):
        """tests.triangles_ref.TriangleGraph of it (made once)"""
        if not hasattr(self, "_tri"):
            self._tri = T.TriangleGraph(self.vid, self.src, self.dst)
        return self._tri

    def sources(self):
        """a source / seed list drawn from the edge ids: the named values, wired vertices (one twice), the hub, LISTED"""
        return np.concatenate([self.named[:4], self.wired[[3, 11, 3, 20]], [self.hub], LISTED]).astype(np.int64)


def _new_ids(kind, vid, wired):
    """the new id of every vertex, in vid's order"""
    rng = np.random.default_rng(0x1D5 + len(kind))
    is_wired = np.isin(vid, wired)
    n_rest = int((~is_wired).sum())
    out = np.empty(vid.size, np.int64)
    if kind == "wide":
        special = EDGE_IDS
        pool = rng.integers(I64_MIN, I64_MAX, 2 * n_rest, dtype=np.int64, endpoint=True)
        rest = np.setdiff1d(np.unique(pool), EDGE_IDS)
        rest = rest[rng.permutation(rest.size)][:n_rest]
    elif kind in _DENSE:
        lo, taken = _DENSE[kind]
        offs = np.array(list(taken), np.int64)
        others = np.setdiff1d(np.arange(WINDOW, dtype=np.int64), offs)
        special = np.array([lo + int(o) for o in offs.tolist()], np.int64)
        rest = np.array([lo + int(o) for o in rng.choice(others, n_rest, replace=False).tolist()], np.int64)
    elif kind == "sparse":
        from duckdb_pgq_amd import datagen

        ids = np.sort(datagen.person_ids(vid.size, 11))
        ids = ids - (ids[vid.size // 2] + 1)                       # the middle id becomes -1
        mid = np.arange(vid.size // 2 - N_EDGE // 2, vid.size // 2 + N_EDGE // 2)
        special, rest = ids[mid], np.delete(ids, mid)
    else:
        raise AssertionError(kind)
    out[is_wired] = special[rng.permutation(N_EDGE)]
    out[~is_wired] = rest[rng.permutation(n_rest)]
    return out


_made = {}


def edge_graph(kind) -> EdgeGraph:
    """the graph under the placement `kind` (made once per process; its arrays are read-only)"""
    if kind not in _made:
        vid, src, dst, wired, hub = base_graph()
        new = _new_ids(kind, vid, wired)
        to = dict(zip(vid.tolist(), new.tolist()))
        v2, s2, d2 = relabel(vid, src, dst, new)
        _made[kind] = EdgeGraph(kind, v2, s2, d2, np.array([to[int(w)] for w in wired.tolist()], np.int64), to[hub])
    return _made[kind]


def weights_of(eg):
    """one int64 weight per vertex, in vertex-table order: random, of both signs, with the extremes on the named vertices"""
    rng = np.random.RandomState(0xA66)
    w = rng.randint(-(1 << 62), 1 << 62, size=eg.vid.size, dtype=np.int64) * 2 + rng.randint(0, 2, size=eg.vid.size)
    extremes = [I64_MIN, I64_MAX, -1, 0]
    for i, v in enumerate(eg.named.tolist()):
        w[eg.tri.index[v]] = extremes[i % 4]
    return w


TABLE_HOPS = 2
FILTER_COLUMNS = [(2, 0), (0, 2)]  # (from_col, to_col) of gg_result_filter_edge: the walk closes, forwards or backwards


def references(eg) -> dict:
    """what the suite's restatements say about `eg`, fed (vid, src, dst) — computed once per placement, never changed.
    Both tests/test_edge_ids_cpu.py (every answer is non-empty and holds an edge id) and tests/test_gpu_edge_ids.py (the
    device gives the same) read it."""
    if hasattr(eg, "_references"):
        return eg._references
    from tests import components_ref as CC
    from tests import edge_filter_ref as F
    from tests import extend_ref as X
    from tests import group_by_ref as R
    from tests import khop_aggregate_ref as K
    from tests import khop_pair_counts_ref as P

    g, w = eg.tri, weights_of(eg)
    S = eg.sources()
    out = {"weights": w, "sources": S}
    out["triangles"] = {(order, which): g.rows(order, None if which == "all" else S)
                        for order in (0, 1) for which in ("all", "list")}
    out["aggregate"] = {(gb, zero): K.aggregate(g, 2, gb, None, np.zeros_like(w) if zero else w)
                        for gb in K.GROUPS for zero in (False, True)}
    out["pair_targets"] = np.concatenate([eg.wired[::2], eg.named, LISTED])
    out["pair_counts"] = P.pair_counts(g, 2, S, out["pair_targets"])
    out["pair_counts_all"] = P.pair_counts(g, 2, S)
    out["components"] = CC.components(eg.vid, eg.src, eg.dst)
    # the whole graph is one component; the rows between wired vertices (their component's id is one of them) and every
    # ninth row that touches none of them leave many
    ws, wd = np.isin(eg.src, eg.wired), np.isin(eg.dst, eg.wired)
    few = ((np.arange(eg.src.size) % 9 == 0) & ~ws & ~wd) | (ws & wd)
    out["few_rows"] = (eg.src[few], eg.dst[few])
    out["components_few_rows"] = CC.components(eg.vid, *out["few_rows"])
    # the walk table of filter_edge / extend_edge / group_by: the 2-hop rows of a source list of edge ids
    out["table_sources"] = np.concatenate([eg.named[:4], eg.wired[[3, 3]], LISTED]).astype(np.int64)
    out["table_dense"] = F.walks(g, out["table_sources"], TABLE_HOPS)
    table = g.vid[out["table_dense"]]
    out["table"] = table
    out["filter"] = {(fc, tc, mode): F.filter_rows(table, g.A, g.index, fc, tc, mode)
                     for fc, tc in FILTER_COLUMNS for mode in F.MODES}
    out["extend"] = {fc: X.extend_rows(table, eg.src, eg.dst, None, fc, vertices=eg.vid) for fc in range(TABLE_HOPS + 1)}
    out["group_by"] = {(kc, wc): R.group_by(table, kc, eg.vid, wc, None, None if wc is None else w)
                       for kc in range(TABLE_HOPS + 1) for wc in (None, 0, TABLE_HOPS)}
    for a in (w, table, out["table_dense"]):
        a.setflags(write=False)
    eg._references = out
    return out


def path_pairs(eg):
    """(sources, targets) of the shortest-path calls: every ordered pair of the named values, some wired vertices, the
    hub (several shortest paths lead there from a wired vertex), six other vertices and LISTED"""
    ends = np.concatenate([eg.named[:4], eg.wired[1::4], [eg.hub], eg.vid[:6], LISTED]).astype(np.int64)
    return np.repeat(ends, ends.size), np.tile(ends, ends.size)


def tiny_graphs():
    """name -> (vid, src, dst): the vertex counts at which one dropped element empties a sort altogether"""
    none = np.empty(0, np.int64)
    return {
        "one_vertex": (np.array([-1], np.int64), none, none),
        "two_vertices": (np.array([-1, I64_MAX], np.int64), np.array([-1, I64_MAX], np.int64),
                         np.array([I64_MAX, -1], np.int64)),
    }
