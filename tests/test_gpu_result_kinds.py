"""Every kind of device result against every reader of the C ABI: the status code of each (reader, result) pair, and every
fetcher's row slices on its own kind.

One graph serves both tests: 12 vertices with non-contiguous ids and 29 edge rows with explicit rowids — a DAG over nine
of them apart from the mirrored pair 7 <-> 11 and the two parallel rows 41 -> 7, which close 7 -> {11, 20, 21} -> 41 -> 7
(a DAG with a mirrored pair has no closed 3-edge walk, and the triangle results are to hold rows), plus the pair 71 -> 90
and the lone vertex 100, so that there are three components.  Walks from a seed therefore never end, and the closures are
bounded at three levels.

The code table below is written from the rule of include/gg.h, not from a run: a reader that matches the result's kind
answers GG_OK; otherwise GG_ERR_STATE if the result's kind or the reader's is one of the kinds born with a refusal
contract (aggregates, pair counts, components, all shortest paths), and GG_ERR_INVALID_ARG among the five older kinds
(walk tables, walk closure, reach closure, level sets, paths).  gg_triangles_fetch_edges answers GG_ERR_STATE to every
result without triangle edge columns, gg_result_fetch_edges GG_ERR_INVALID_ARG to a table without edge columns, and the
consumers keep the codes their own comments promise: gg_result_group_by, gg_result_filter_value and gg_result_top_rows
answer GG_OK on the four walk-table kinds and GG_ERR_STATE on every other kind, whose level they never get to look at."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GG_OK, GG_ERR_INVALID_ARG, GG_ERR_STATE = 0, -1, -6
CODES = {".": GG_OK, "I": GG_ERR_INVALID_ARG, "S": GG_ERR_STATE}
i64p, i32p, u64p, u32p = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)

VID = np.array([3, 7, 11, 20, 21, 41, 55, 70, 71, 90, 100, 40], np.int64)
_EDGES = [(3, 7), (3, 11), (3, 20), (7, 11), (7, 20), (7, 21), (11, 20), (11, 21), (11, 41), (20, 21), (20, 41), (20, 55),
          (21, 41), (21, 55), (21, 70), (41, 55), (41, 70), (55, 70), (55, 40), (70, 40), (3, 7), (41, 40), (11, 55),
          (20, 70), (3, 21),
          (11, 7),           # the mirrored pair
          (41, 7), (41, 7),  # closes 7 -> {11, 20, 21} -> 41 -> 7, twice
          (71, 90)]          # a second component; 100 is a third
SRC = np.array([e[0] for e in _EDGES], np.int64)
DST = np.array([e[1] for e in _EDGES], np.int64)
ROWID = 1000 + 7 * np.arange(len(_EDGES), dtype=np.int64)
SEEDS = np.array([3, 7, 20], np.int64)
HOPS = 2  # the level every reader with a `hops` argument is asked for: each such result has it

# the results, in the order of the table's columns
KINDS = ["walk", "walk_edges", "tri", "tri_edges", "closure", "reach", "levels", "paths", "agg", "top", "pairs", "comps",
         "all_paths"]
#                                     walk tables|older kinds|kinds with a refusal contract
#                                      W WE T TE | C R L P | A AT PC CC AP
CODE_TABLE = {
    "gg_result_rows":                    "....IIIISSSSS",
    "gg_result_fetch":                   "....IIIISSSSS",
    "gg_result_fetch_edges":             "I.I.IIIISSSSS",  # (tri_edges: e1, e2 are the edges of the 2-hop walk a -> b -> c)
    "gg_triangles_fetch_edges":          "SSS.SSSSSSSSS",
    "gg_walk_closure_levels":            "IIII.IIISSSSS",
    "gg_walk_closure_fetch":             "IIII.IIISSSSS",
    "gg_reach_closure_levels":           "IIIII.IISSSSS",
    "gg_reach_closure_fetch":            "IIIII.IISSSSS",
    "gg_level_sets_levels":              "IIIIII.ISSSSS",
    "gg_level_sets_fetch":               "IIIIII.ISSSSS",
    "gg_bfs64_paths_rows":               "IIIIIII.SSSSS",
    "gg_bfs64_paths_fetch":              "IIIIIII.SSSSS",
    "gg_khop_aggregate_rows":            "SSSSSSSS..SSS",
    "gg_khop_aggregate_fetch":           "SSSSSSSS..SSS",
    "gg_khop_pair_counts_rows":          "SSSSSSSSSS.SS",
    "gg_khop_pair_counts_fetch":         "SSSSSSSSSS.SS",
    "gg_components_rows":                "SSSSSSSSSSS.S",
    "gg_components_fetch":               "SSSSSSSSSSS.S",
    "gg_components_fetch_sizes":         "SSSSSSSSSSS.S",
    "gg_bfs64_all_paths_rows":           "SSSSSSSSSSSS.",
    "gg_bfs64_all_paths_fetch_pairs":    "SSSSSSSSSSSS.",
    "gg_bfs64_all_paths_fetch":          "SSSSSSSSSSSS.",
    # the consumers: a result without fixed-length tables is GG_ERR_STATE to the edge filter and the extension,
    # GG_ERR_INVALID_ARG (a level outside the result's) to the common-neighbour filter and the digest
    "gg_result_filter_edge":             "....SSSSSSSSS",
    "gg_result_filter_common_neighbour": "....IIIIIIIII",
    "gg_result_extend_edge":             "....SSSSSSSSS",
    "gg_result_digest":                  "....IIIIIIIII",
    "gg_khop_aggregate_top":             "SSSSSSSS..SSS",
    # the three younger consumers look at the kind before the level: GG_ERR_STATE to everything but a walk table
    "gg_result_group_by":                "....SSSSSSSSS",
    "gg_result_filter_value":            "....SSSSSSSSS",
    "gg_result_top_rows":                "....SSSSSSSSS",
}


def _p(a, t=i64p):
    return None if a is None else a.ctypes.data_as(t)


def make_results(gg, csr, out, edges=True):
    """one result of each kind through the C ABI into out[name]; edges=False: only the two path results, searched without
    edges, as out[name + "_plain"]"""
    lib, ctx, h = gg.lib, gg.ctx, csr.handle

    def take(name, rc, res):
        assert rc == GG_OK, (name, rc)
        assert res.value is not None, name
        out[name if edges else name + "_plain"] = res

    lanes = np.repeat(np.arange(SEEDS.size, dtype=np.uint32), VID.size)
    targets = np.tile(VID, SEEDS.size)
    bst = lib.gg_bfs64_paths.argtypes[9]._type_()
    res = C.c_void_p()
    take("paths", lib.gg_bfs64_paths(ctx, h, _p(SEEDS), SEEDS.size, -1, _p(lanes, u32p), _p(targets), targets.size,
                                     int(edges), C.byref(bst), C.byref(res)), res)
    res = C.c_void_p()
    take("all_paths", lib.gg_bfs64_all_paths(ctx, h, _p(SEEDS), SEEDS.size, -1, _p(lanes, u32p), _p(targets), targets.size,
                                             0, int(edges), 1, None, C.byref(res)), res)
    if not edges:
        return
    kst = lib.gg_expand_khop_result.argtypes[6]._type_()
    res = C.c_void_p()
    take("walk", lib.gg_expand_khop_result(ctx, h, _p(SEEDS), SEEDS.size, 1, HOPS, C.byref(kst), C.byref(res)), res)
    res = C.c_void_p()
    take("walk_edges", lib.gg_expand_khop_edges(ctx, h, _p(SEEDS), SEEDS.size, HOPS, C.byref(kst), C.byref(res)), res)
    tst = lib.gg_triangles.argtypes[6]._type_()
    res = C.c_void_p()
    take("tri", lib.gg_triangles(ctx, h, None, 0, 0, 1, C.byref(tst), C.byref(res)), res)
    res = C.c_void_p()
    take("tri_edges", lib.gg_triangles_edges(ctx, h, None, 0, 0, C.byref(tst), C.byref(res)), res)
    res = C.c_void_p()
    take("closure", lib.gg_walk_closure(ctx, h, _p(SEEDS), SEEDS.size, 3, C.byref(res)), res)
    classes = np.array([0, 1, 1], np.uint32)
    res = C.c_void_p()
    take("reach", lib.gg_reach_closure(ctx, h, _p(SEEDS), _p(classes, u32p), None, SEEDS.size, 2, C.byref(res)), res)
    res = C.c_void_p()
    take("levels", lib.gg_level_sets(ctx, h, _p(SEEDS), _p(classes, u32p), SEEDS.size, 2, 3, C.byref(res)), res)
    weights = np.arange(VID.size, dtype=np.int64) * 1_000_003 - 5
    res = C.c_void_p()
    take("agg", lib.gg_khop_aggregate(ctx, h, None, 0, 1, HOPS, 0, _p(weights), None, C.byref(res)), res)
    res = C.c_void_p()
    take("top", lib.gg_khop_aggregate_top(ctx, out["agg"], HOPS, 0, 1, 4, None, None, None, C.byref(res)), res)
    res = C.c_void_p()
    take("pairs", lib.gg_khop_pair_counts(ctx, h, _p(SEEDS), SEEDS.size, 1, HOPS, None, 0, None, C.byref(res)), res)
    res = C.c_void_p()
    take("comps", lib.gg_components(ctx, h, None, C.byref(res)), res)
    assert sorted(out) == sorted(KINDS)


@pytest.fixture
def graph(gg):
    gg.staging_clear()
    gg.append_vertices(VID)
    gg.append_edges(SRC, DST, ROWID)
    csr = gg.build_csr()
    results = {}
    try:
        yield gg, csr, results
    finally:
        for res in results.values():
            gg.lib.gg_result_destroy(res)
        csr.close()


class Bufs:
    """destinations of eight entries for a call whose code alone is looked at"""

    def __init__(self):
        self.a, self.b, self.c, self.d = (np.zeros(8, np.int64) for _ in range(4))
        self.s32 = np.zeros(8, np.int32)
        self.u1, self.u2 = np.zeros(8, np.uint64), np.zeros(8, np.uint64)
        self.ptrs = (i64p * 3)(_p(self.a), _p(self.b), _p(self.c))
        self.n, self.got, self.nl = C.c_uint64(), C.c_uint32(), C.c_int()


def call_reader(gg, csr, name, res):
    """the reader or consumer `name` on `res` with every argument present; the code it returns"""
    lib, ctx, b = gg.lib, gg.ctx, Bufs()
    n, got, nl = C.byref(b.n), C.byref(b.got), C.byref(b.nl)
    a, bb, c, d, s32, u1, u2 = _p(b.a), _p(b.b), _p(b.c), _p(b.d), _p(b.s32, i32p), _p(b.u1, u64p), _p(b.u2, u64p)
    made = C.c_void_p()
    try:
        if name == "gg_result_rows":
            return lib.gg_result_rows(res, HOPS, n)
        if name == "gg_result_fetch":
            return lib.gg_result_fetch(res, HOPS, 0, 8, b.ptrs, got)
        if name == "gg_result_fetch_edges":
            return lib.gg_result_fetch_edges(res, HOPS, 0, 8, b.ptrs, got)
        if name == "gg_triangles_fetch_edges":
            return lib.gg_triangles_fetch_edges(res, 0, 8, b.ptrs, got)
        if name in ("gg_walk_closure_levels", "gg_reach_closure_levels", "gg_level_sets_levels"):
            return getattr(lib, name)(res, u1, 8, nl)
        if name in ("gg_walk_closure_fetch", "gg_reach_closure_fetch", "gg_level_sets_fetch"):
            return getattr(lib, name)(res, 0, 8, a, bb, s32, got)
        if name == "gg_bfs64_paths_rows":
            return lib.gg_bfs64_paths_rows(res, n)
        if name == "gg_bfs64_paths_fetch":
            return lib.gg_bfs64_paths_fetch(res, 0, 8, a, s32, bb, c, got)
        if name in ("gg_khop_aggregate_rows", "gg_khop_pair_counts_rows"):
            return getattr(lib, name)(res, HOPS, n)
        if name == "gg_khop_aggregate_fetch":
            return lib.gg_khop_aggregate_fetch(res, HOPS, 0, 8, a, u1, u2, bb, got)
        if name == "gg_khop_pair_counts_fetch":
            return lib.gg_khop_pair_counts_fetch(res, HOPS, 0, 8, a, bb, u1, got)
        if name in ("gg_components_rows", "gg_bfs64_all_paths_rows"):
            return getattr(lib, name)(res, 0, n)
        if name == "gg_components_fetch":
            return lib.gg_components_fetch(res, 0, 8, a, bb, u1, got)
        if name == "gg_components_fetch_sizes":
            return lib.gg_components_fetch_sizes(res, 0, 8, a, u1, got)
        if name == "gg_bfs64_all_paths_fetch_pairs":
            return lib.gg_bfs64_all_paths_fetch_pairs(res, 0, 8, a, s32, u1, u2, got)
        if name == "gg_bfs64_all_paths_fetch":
            return lib.gg_bfs64_all_paths_fetch(res, 0, 8, a, bb, s32, c, d, got)
        if name == "gg_result_filter_edge":
            st = lib.gg_result_filter_edge.argtypes[8]._type_()
            return lib.gg_result_filter_edge(ctx, res, HOPS, csr.handle, HOPS, 0, 0, 0, C.byref(st), None)
        if name == "gg_result_filter_common_neighbour":
            return lib.gg_result_filter_common_neighbour(ctx, res, HOPS, csr.handle, C.byref(made))
        if name == "gg_result_extend_edge":
            st = lib.gg_result_extend_edge.argtypes[7]._type_()
            return lib.gg_result_extend_edge(ctx, res, HOPS, csr.handle, HOPS, 0, 0, C.byref(st), None)
        if name == "gg_result_digest":
            return lib.gg_result_digest(ctx, csr.handle, res, HOPS, n, C.byref(C.c_uint64()))
        if name == "gg_khop_aggregate_top":
            return lib.gg_khop_aggregate_top(ctx, res, HOPS, 0, 1, 3, None, None, None, C.byref(made))
        if name == "gg_result_group_by":
            st = lib.gg_result_group_by.argtypes[8]._type_()
            return lib.gg_result_group_by(ctx, res, HOPS, HOPS, csr.handle, -1, None, None, C.byref(st), C.byref(made))
        if name == "gg_result_filter_value":
            st = lib.gg_result_filter_value.argtypes[11]._type_()
            return lib.gg_result_filter_value(ctx, res, HOPS, HOPS, csr.handle, _p(np.zeros(VID.size, np.int64)), None, -1, 1,
                                              0, 1, C.byref(st), C.byref(made))
        if name == "gg_result_top_rows":
            st = lib.gg_result_top_rows.argtypes[13]._type_()
            return lib.gg_result_top_rows(ctx, res, HOPS, HOPS, csr.handle, _p(np.zeros(VID.size, np.int64)), None, -1, 1, 0,
                                          1, 0, 3, C.byref(st), C.byref(made))
        raise AssertionError(name)
    finally:
        if made.value is not None:
            lib.gg_result_destroy(made)


def test_every_reader_on_every_result_returns_the_code_of_the_rule(graph):
    gg, csr, results = graph
    make_results(gg, csr, results)
    assert len(CODE_TABLE) == 30 and all(len(row) == len(KINDS) for row in CODE_TABLE.values())
    wrong = []
    for name, row in CODE_TABLE.items():
        for kind, want in zip(KINDS, row):
            rc = call_reader(gg, csr, name, results[kind])
            print(f"{name}({kind}) = {rc}, the rule says {CODES[want]}")
            if rc != CODES[want]:
                wrong.append((name, kind, rc, CODES[want]))
    assert not wrong, wrong
    # the context still serves: the walk table is what it was
    n = C.c_uint64()
    assert gg.lib.gg_result_rows(results["walk"], HOPS, C.byref(n)) == GG_OK and n.value > 3


# ---- slices -----------------------------------------------------------------------------------------------------------
# a fetcher: name, the result it reads, its columns as (dtype, nullable), how its row count is read, and the call given
# (result, offset, max_rows, column pointers, n_out)
I64, I32, U64 = np.int64, np.int32, np.uint64
_PT = {I64: i64p, I32: i32p, U64: u64p}


def _array_call(fn, hops=None):
    def call(lib, res, offset, max_rows, ptrs, n_out):
        arr = (i64p * len(ptrs))(*ptrs)
        if hops is None:
            return getattr(lib, fn)(res, offset, max_rows, arr, n_out)
        return getattr(lib, fn)(res, hops, offset, max_rows, arr, n_out)
    return call


def _plain_call(fn, *lead):
    def call(lib, res, offset, max_rows, ptrs, n_out):
        return getattr(lib, fn)(res, *lead, offset, max_rows, *ptrs, n_out)
    return call


def _rows(fn, *lead):
    def total(lib, res):
        n = C.c_uint64()
        assert getattr(lib, fn)(res, *lead, C.byref(n)) == GG_OK
        return n.value
    return total


def _levels(fn):
    def total(lib, res):
        nl, per = C.c_int(), np.zeros(8, np.uint64)
        assert getattr(lib, fn)(res, _p(per, u64p), 8, C.byref(nl)) == GG_OK
        assert 2 <= nl.value <= 8 and np.all(per[:nl.value] > 0) and not per[nl.value:].any()
        one = np.zeros(1, np.uint64)  # a smaller capacity: the count is the same, the array is filled to its capacity
        nl1 = C.c_int()
        assert getattr(lib, fn)(res, _p(one, u64p), 1, C.byref(nl1)) == GG_OK and nl1.value == nl.value and one[0] == per[0]
        assert getattr(lib, fn)(res, None, 0, C.byref(nl1)) == GG_OK and nl1.value == nl.value
        return int(per.sum()), per[:nl.value].astype(np.int64)
    return total


FETCHERS = [
    ("gg_result_fetch", "walk", [(I64, False)] * 3, _rows("gg_result_rows", HOPS), _array_call("gg_result_fetch", HOPS)),
    ("gg_result_fetch/1", "walk", [(I64, False)] * 2, _rows("gg_result_rows", 1), _array_call("gg_result_fetch", 1)),
    ("gg_result_fetch/tri", "tri_edges", [(I64, False)] * 3, _rows("gg_result_rows", 2), _array_call("gg_result_fetch", 2)),
    ("gg_result_fetch_edges", "walk_edges", [(I64, False)] * 2, _rows("gg_result_rows", HOPS),
     _array_call("gg_result_fetch_edges", HOPS)),
    ("gg_triangles_fetch_edges", "tri_edges", [(I64, False)] * 3, _rows("gg_result_rows", 2),
     _array_call("gg_triangles_fetch_edges")),
    ("gg_walk_closure_fetch", "closure", [(I64, False), (I64, False), (I32, True)], _levels("gg_walk_closure_levels"),
     _plain_call("gg_walk_closure_fetch")),
    ("gg_reach_closure_fetch", "reach", [(I64, False), (I64, False), (I32, True)], _levels("gg_reach_closure_levels"),
     _plain_call("gg_reach_closure_fetch")),
    ("gg_level_sets_fetch", "levels", [(I64, False), (I64, False), (I32, True)], _levels("gg_level_sets_levels"),
     _plain_call("gg_level_sets_fetch")),
    ("gg_bfs64_paths_fetch", "paths", [(I64, False), (I32, False), (I64, False), (I64, True)], _rows("gg_bfs64_paths_rows"),
     _plain_call("gg_bfs64_paths_fetch")),
    ("gg_khop_aggregate_fetch", "agg", [(I64, False), (U64, False), (U64, True), (I64, True)],
     _rows("gg_khop_aggregate_rows", HOPS), _plain_call("gg_khop_aggregate_fetch", HOPS)),
    ("gg_khop_aggregate_fetch/1", "agg", [(I64, False), (U64, False), (U64, True), (I64, True)],
     _rows("gg_khop_aggregate_rows", 1), _plain_call("gg_khop_aggregate_fetch", 1)),
    ("gg_khop_aggregate_fetch/top", "top", [(I64, False), (U64, False), (U64, True), (I64, True)],
     _rows("gg_khop_aggregate_rows", HOPS), _plain_call("gg_khop_aggregate_fetch", HOPS)),
    ("gg_khop_pair_counts_fetch", "pairs", [(I64, True), (I64, True), (U64, True)], _rows("gg_khop_pair_counts_rows", HOPS),
     _plain_call("gg_khop_pair_counts_fetch", HOPS)),
    ("gg_khop_pair_counts_fetch/1", "pairs", [(I64, True), (I64, True), (U64, True)], _rows("gg_khop_pair_counts_rows", 1),
     _plain_call("gg_khop_pair_counts_fetch", 1)),
    ("gg_components_fetch", "comps", [(I64, True), (I64, True), (U64, True)], _rows("gg_components_rows", 0),
     _plain_call("gg_components_fetch")),
    ("gg_components_fetch_sizes", "comps", [(I64, True), (U64, True)], _rows("gg_components_rows", 1),
     _plain_call("gg_components_fetch_sizes")),
    ("gg_bfs64_all_paths_fetch_pairs", "all_paths", [(I64, True), (I32, True), (U64, True), (U64, True)],
     _rows("gg_bfs64_all_paths_rows", 0), _plain_call("gg_bfs64_all_paths_fetch_pairs")),
    ("gg_bfs64_all_paths_fetch", "all_paths", [(I64, False), (I64, False), (I32, False), (I64, False), (I64, True)],
     _rows("gg_bfs64_all_paths_rows", 1), _plain_call("gg_bfs64_all_paths_fetch")),
]
FILL = 0x5A  # the byte a destination holds before a fetch: rows past *n_out must keep it


def fetch(lib, call, res, cols, offset, max_rows, absent=()):
    """one call: (*n_out, the fetched rows per column — None for a column whose pointer was NULL)"""
    bufs = [None if c in absent else np.full(max(max_rows, 1) * np.dtype(t).itemsize, FILL, np.uint8).view(t)
            for c, (t, _) in enumerate(cols)]
    ptrs = [None if b is None else _p(b, _PT[cols[c][0]]) for c, b in enumerate(bufs)]
    n_out = C.c_uint32(0xDEAD)
    assert call(lib, res, offset, max_rows, ptrs, C.byref(n_out)) == GG_OK
    n = n_out.value
    assert n <= max_rows
    for b in bufs:
        if b is not None:
            assert np.all(b[n:].view(np.uint8) == FILL)  # nothing is written past the rows handed out
    return n, [None if b is None else b[:n].copy() for b in bufs]


def check_slices(lib, name, call, res, cols, total, absent=()):
    n, whole = fetch(lib, call, res, cols, 0, total + 10, absent)
    assert n == total >= 3, (name, n, total)
    for (offset, max_rows), expect in [((0, 1), 1), ((total - 1, 1), 1), ((total - 1, 9), 1), ((total, 9), 0),
                                       ((total + 7, 9), 0), ((1, total + 10), total - 1), ((2, 1), 1),
                                       ((1, total - 2), total - 2)]:
        n, part = fetch(lib, call, res, cols, offset, max_rows, absent)
        assert n == expect == min(max_rows, max(total - offset, 0)), (name, offset, max_rows, n)
        for w, p in zip(whole, part):
            assert (w is None) == (p is None)
            if w is not None:
                assert p.dtype == w.dtype and np.array_equal(p, w[offset:offset + n]), (name, offset, max_rows)
    # the whole table again from slices: one row, then what is left with room to spare
    _, head = fetch(lib, call, res, cols, 0, 1, absent)
    _, tail = fetch(lib, call, res, cols, 1, total + 10, absent)
    for w, a, b in zip(whole, head, tail):
        if w is not None:
            assert np.array_equal(np.concatenate([a, b]), w), name
    return whole


def test_every_fetcher_hands_out_exact_slices_of_its_own_kind(graph):
    gg, csr, results = graph
    lib = gg.lib
    make_results(gg, csr, results)
    wholes = {}
    for name, kind, cols, total_of, call in FETCHERS:
        total = total_of(lib, results[kind])
        per_level = None
        if isinstance(total, tuple):
            total, per_level = total
        whole = wholes[name] = check_slices(lib, name, call, results[kind], cols, total)
        if per_level is not None:  # the level column is the per-level row counts spelled out
            assert np.array_equal(whole[2], np.repeat(np.arange(1, per_level.size + 1, dtype=np.int32), per_level)), name
        for c, (_, nullable) in enumerate(cols):
            if not nullable:
                continue
            part = check_slices(lib, name, call, results[kind], cols, total, absent=(c,))
            for k, (w, p) in enumerate(zip(whole, part)):  # the remaining columns are unchanged
                assert (p is None) == (k == c) and (p is None or np.array_equal(p, w)), (name, c, k)
        nullable = [c for c, (_, nl) in enumerate(cols) if nl]
        if len(nullable) > 1:  # all of them NULL at once: the count alone
            part = check_slices(lib, name, call, results[kind], cols, total, absent=tuple(nullable))
            assert all((p is None) == (k in nullable) for k, p in enumerate(part))
    # explicit rowids come back as staged, and the id columns of the two triangle fetches belong to the same rows
    assert set(wholes["gg_result_fetch_edges"][0]) <= set(ROWID) and set(wholes["gg_walk_closure_fetch"][1]) <= set(ROWID)
    a, b, c = wholes["gg_result_fetch/tri"]
    e1, e2, e3 = wholes["gg_triangles_fetch_edges"]
    where = {int(r): i for i, r in enumerate(ROWID)}
    for col_from, col_to, e in ((a, b, e1), (b, c, e2), (c, a, e3)):
        at = np.array([where[int(r)] for r in e])
        assert np.array_equal(SRC[at], col_from) and np.array_equal(DST[at], col_to)
    assert a.size == 18  # 7 -> {11, 20, 21} -> 41 -> 7 in three rotations each, the closing rows 41 -> 7 twice

    # searched without edges: the same rows, and -1 for every rowid
    make_results(gg, csr, results, edges=False)
    for name, kind in (("gg_bfs64_paths_fetch", "paths"), ("gg_bfs64_all_paths_fetch", "all_paths")):
        _, _, cols, total_of, call = next(f for f in FETCHERS if f[0] == name)
        total = total_of(lib, results[kind + "_plain"])
        whole = check_slices(lib, name, call, results[kind + "_plain"], cols, total)
        assert total == wholes[name][0].size and np.all(whole[-1] == -1) and (wholes[name][-1] != -1).any()
        for w, p in zip(wholes[name][:-1], whole[:-1]):
            assert np.array_equal(w, p)
        check_slices(lib, name, call, results[kind + "_plain"], cols, total, absent=(len(cols) - 1,))
