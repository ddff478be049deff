"""GG.components (gg_components) against the restatement (tests/components_ref.py): both tables row for row, in order, and
every stats field.  Each case runs under both values of the init_mode knob (0 and 1) and with the flatten's changed word
read after every launch and at the default pace, twice each: the eight answers are identical arrays.  On every case
hooks == vertices - components, sum(sizes) == V, max(sizes) == largest and jump_launches stays inside the doubling bound
ceil(log2(max(V, 2))) + jumps_per_check.

The shapes are the smallest at which each mechanism can go wrong: no vertex, one vertex, direction, a path of 2^17 vertices
in three vertex-table orders (depth: a flatten that walks is quadratic there), stars whose hub is the first and the last
vertex (every CAS on one root, or on roots that keep changing), disjoint pairs and a component whose members straddle the
waves (size counting), two long paths joined by the last row, parallel rows and self-loops, V around the tile edges, the
two goldens, every build form, and the errors.

Not covered here: GG_ERR_OOM needs more vertices than the device holds labels for."""
import ctypes as C
import math
import time

import numpy as np
import pytest

from duckdb_pgq_amd import GGError
from duckdb_pgq_amd.gg import CcStats
from tests import components_ref as K
from tests import trainbenchmark as tb
from tests import triangles_ref as T

pytestmark = pytest.mark.gpu

GG_ERR_INVALID_ARG, GG_ERR_STATE = -1, -6
DEFAULT_JUMPS = 4
TABLES = ("vertex", "component", "size", "components", "sizes")


def build(gg, vid, src, dst):
    gg.staging_clear()
    gg.append_vertices(np.asarray(vid, np.int64))
    gg.append_edges(np.asarray(src, np.int64), np.asarray(dst, np.int64))
    return gg.build_csr()


def check(gg, csr, want):
    """the eight calls of one case against the restatement's answer; returns the last one"""
    V = want["stats"]["vertices"]
    got = None
    for init_mode in (0, 1):
        for jumps in (1, 0):
            gg.debug_components(init_mode, jumps)
            for _ in range(2):
                got = gg.components(csr)
                st = dict(got["stats"])
                launches = st.pop("jump_launches")
                print("init", init_mode, "jumps", jumps, st, "launches", launches)
                for key in TABLES:
                    assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), key
                assert st == want["stats"]
                assert st["hooks"] == st["vertices"] - st["components"]
                assert int(got["sizes"].sum()) == V and (int(got["sizes"].max()) if V else 0) == st["largest"]
                per_check = jumps or DEFAULT_JUMPS
                assert launches <= math.ceil(math.log2(max(V, 2))) + per_check
                assert launches % per_check == 0 and (launches > 0) == (V > 0)
            only = gg.components(csr, fetch=False)  # out_result NULL: the stats alone
            assert set(only) == {"stats"}  # (jump_launches depends on the forest the hooks left, that on the schedule)
            assert {k: v for k, v in only["stats"].items() if k != "jump_launches"} == want["stats"]
    gg.debug_components(0, 0)
    return got


def run(gg, vid, src, dst, want=None):
    want = want or K.components(vid, src, dst)
    csr = build(gg, vid, src, dst)
    try:
        assert csr.V == want["stats"]["vertices"] and csr.E == want["stats"]["entries_read"]
        return check(gg, csr, want)
    finally:
        csr.close()


def test_degenerate_graphs(gg):
    none = np.empty(0, np.int64)
    got = run(gg, none, none, none)  # V = 0: two empty tables
    assert got["vertex"].size == got["components"].size == 0 and got["stats"]["jump_launches"] == 0
    one = np.array([42], np.int64)
    assert run(gg, one, none, none)["component"].tolist() == [42]
    got = run(gg, one, one, one)  # one vertex with a self-loop
    assert got["size"].tolist() == [1] and got["stats"]["singletons"] == 1 and got["stats"]["entries_read"] == 1
    vid = np.array([9, 4, 6, 1], np.int64)
    got = run(gg, vid, np.array([4, 1, 77]), np.array([88, 99, 9]))  # every row dangles
    assert got["stats"]["components"] == 4 and got["stats"]["entries_read"] == 0


@pytest.mark.parametrize("row", [(9, 6), (6, 9)])
def test_one_unmirrored_row_joins_its_ends_whichever_way_it_points(gg, row):
    vid = np.array([9, 4, 6, 1], np.int64)  # 9 stands before 6 in the table
    got = run(gg, vid, np.array(row[:1]), np.array(row[1:]))
    assert got["component"].tolist() == [9, 4, 9, 1] and got["size"].tolist() == [2, 1, 2, 1]
    assert got["components"].tolist() == [9, 4, 1] and got["sizes"].tolist() == [2, 1, 1]


@pytest.fixture(scope="module")
def long_paths():
    """the three vertex-table orders of the path of 2^17 vertices with the restatement's answers (computed once)"""
    out = {}
    for order in ("forward", "reverse", "shuffle"):
        shape = K.path(1 << 17, order, 9)
        out[order] = shape + (K.components(*shape),)
    return out


@pytest.mark.parametrize("order", ["forward", "reverse", "shuffle"])
def test_a_path_of_2_17_vertices_is_flattened_by_doubling(gg, long_paths, order):
    vid, src, dst, want = long_paths[order]
    assert want["stats"]["components"] == 1 and want["stats"]["largest"] == 1 << 17
    csr = build(gg, vid, src, dst)
    try:
        t0 = time.perf_counter()
        got = check(gg, csr, want)
        took = time.perf_counter() - t0
        print(order, f"{took:.3f} s for the case's calls")
        assert (got["component"] == vid[0]).all()
        assert took < 5.0  # 12 calls; a flatten that walks the path instead of doubling takes minutes
    finally:
        csr.close()


@pytest.mark.parametrize("hub_first", [True, False])
def test_a_star_of_5000_leaves_contends_on_one_root(gg, hub_first):
    vid, src, dst = K.star(5000, hub_first)
    got = run(gg, vid, src, dst)
    assert got["stats"]["components"] == 1 and got["components"].tolist() == [int(vid[0])]


def test_sizes_where_every_wave_is_mixed(gg):
    got = run(gg, *K.pairs(4096))
    assert got["stats"]["components"] == 4096 and (got["sizes"] == 2).all()
    vid, src, dst = K.straddling()
    got = run(gg, vid, src, dst)
    assert got["stats"]["largest"] == 64 * 5 + 3 and got["stats"]["singletons"] == 2 * (64 * 5 + 3)


def test_two_long_paths_joined_by_the_last_row(gg):
    got = run(gg, *K.late_merge())
    assert got["stats"]["components"] == 1 and got["stats"]["largest"] == 1 << 15


@pytest.fixture(scope="module")
def hard():
    shape = T.hard_graph(V=300, rows=3000, hub_fan=120)
    return shape + (K.components(*shape),)


def test_parallel_rows_and_self_loops_change_nothing(gg, hard):
    vid, src, dst, want = hard
    run(gg, vid, src, dst, want)
    keep = np.ones(src.size, bool)  # the same graph without its self-loops and with every row once more
    keep[src == dst] = False
    again = K.components(vid, np.concatenate([src[keep], src]), np.concatenate([dst[keep], dst]))
    for key in TABLES:
        assert np.array_equal(again[key], want[key])
    run(gg, vid, np.concatenate([src[keep], src]), np.concatenate([dst[keep], dst]), again)


@pytest.mark.parametrize("V", [65, 257, 1025])
def test_tile_edges(gg, V):
    got = run(gg, *K.ring_with_chords(V))
    assert got["stats"]["components"] >= 4 and got["stats"]["singletons"] >= 2


def test_train_benchmark_connects_to(gg):
    te = tb.load("TrackElement")[:, 0]
    ct = tb.load("connectsTo")
    got = run(gg, te, ct[:, 0], ct[:, 1])
    assert got["stats"]["vertices"] == te.size and 1 <= got["stats"]["components"] < te.size


def test_ldbc_small_golden(gg):
    import os

    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ldbc_small.npz"))
    run(gg, z["vid"], z["src"], z["dst"])


@pytest.mark.parametrize("graph", ["hard", "path"])
@pytest.mark.parametrize("form", ["bucketed", "legacy_build", "no_rowid", "legacy_no_rowid", "mirrored", "edge_only"])
def test_build_forms(gg, hard, graph, form):
    vid, src, dst = hard[:3] if graph == "hard" else K.path(3001, "shuffle", 4)
    if "legacy" in form:
        gg.force_legacy_build(True)  # (row, nbr) is the pair the build leaves; else (rrow, rnbr)
    if "no_rowid" in form:
        gg.set_edge_rowid(False)
    if form == "mirrored":
        gg.set_edge_rowid(False)
        gg.rank_mode(1)
        src, dst = np.concatenate([src, dst]), np.concatenate([dst, src])
    if form == "edge_only":  # the vertex table is the ascending endpoint set: dangling rows become vertices
        gg.staging_clear()
        gg.append_edges(np.asarray(src, np.int64), np.asarray(dst, np.int64))
        n = gg.vertices_from_edges()
        vid = np.unique(np.concatenate([src, dst]))
        assert n == vid.size
        want = K.components(vid, src, dst)
        csr = gg.build_csr()
    else:
        want = K.components(vid, src, dst)
        csr = build(gg, vid, src, dst)
    try:
        print(form, graph, "reverse_derived", csr.reverse_derived)
        check(gg, csr, want)
    finally:
        csr.close()


def test_a_fully_mirrored_table_whose_reverse_rows_are_derived(gg):
    from duckdb_pgq_amd import datagen

    vid, s, d = datagen.ldbc_knows(1200, 900, 5)  # sparse: several components
    src, dst = np.concatenate([s, d]), np.concatenate([d, s])
    gg.set_edge_rowid(False)  # the vertex-sorted form of the bucketed build is the one that derives
    gg.rank_mode(1)
    csr = build(gg, vid, src, dst)
    try:
        assert csr.reverse_derived == 1  # the COO pair the hook reads is the derived reverse
        want = K.components(vid, src, dst)
        assert want["stats"]["components"] > 1
        check(gg, csr, want)
    finally:
        csr.close()


def test_the_knob_is_restored_by_debug_reset(gg):
    one = np.array([42], np.int64)
    none = np.empty(0, np.int64)
    csr = build(gg, one, none, none)
    try:
        gg.debug_components(1, 1)
        assert gg.components(csr)["stats"]["jump_launches"] == 1
        gg.debug_components(0, 3)
        assert gg.components(csr)["stats"]["jump_launches"] == 3
        gg.debug_reset()
        assert gg.components(csr)["stats"]["jump_launches"] == DEFAULT_JUMPS
        with pytest.raises(GGError) as e:
            gg.debug_components(2, 0)
        assert e.value.code == GG_ERR_INVALID_ARG
        with pytest.raises(GGError):
            gg.debug_components(-1, 0)
        assert gg.components(csr)["stats"]["jump_launches"] == DEFAULT_JUMPS
    finally:
        csr.close()


def test_errors_leave_the_context_usable(gg):
    vid, src, dst = K.islands()  # (several components: table 1 has rows to slice)
    want = K.components(vid, src, dst)
    gg.staging_clear()
    gg.append_vertices(vid)
    gg.append_edges(src, dst)
    shard = gg.build_csr_shard(0, 2)
    csr = gg.build_csr()
    other = type(gg)(0)
    i64p, u64p = C.POINTER(C.c_int64), C.POINTER(C.c_uint64)

    def call(ctx, graph, stats=True, out=True):
        st, o = CcStats(), C.c_void_p()
        rc = gg.lib.gg_components(ctx, graph, C.byref(st) if stats else None, C.byref(o) if out else None)
        assert rc != 0 and not o.value
        return rc

    def good():
        got = gg.components(csr)
        for key in TABLES:
            assert np.array_equal(got[key], want[key])

    try:
        bad = [
            lambda: (call(None, csr.handle), GG_ERR_INVALID_ARG),
            lambda: (call(gg.ctx, None), GG_ERR_INVALID_ARG),
            lambda: (call(other.ctx, csr.handle), GG_ERR_INVALID_ARG),  # a CSR of another context
            lambda: (call(gg.ctx, csr.handle, stats=False, out=False), GG_ERR_INVALID_ARG),
            lambda: (gg.lib.gg_debug_components(gg.ctx, 2, 0), GG_ERR_INVALID_ARG),
            lambda: (gg.lib.gg_debug_components(gg.ctx, -1, 0), GG_ERR_INVALID_ARG),
            lambda: (gg.lib.gg_debug_components(None, 0, 0), GG_ERR_INVALID_ARG),
            lambda: (call(gg.ctx, shard.handle), GG_ERR_STATE),
        ]
        for i, case in enumerate(bad):
            rc, code = case()
            assert rc == code, (i, rc, code)
            good()  # a correct call still works
        # the result answers its own three calls only, and they answer no other result
        res = C.c_void_p()
        assert gg.lib.gg_components(gg.ctx, csr.handle, None, C.byref(res)) == 0  # stats NULL: the result alone
        table = gg.expand_khop_result(csr, 1, vid[:4])
        agg = gg.khop_aggregate(csr, 1, 2, "end", vid[:4])
        try:
            n, got = C.c_uint64(), C.c_uint32()
            buf = np.empty((3, 8), np.int64)
            ptrs = (i64p * 3)(*[buf[c].ctypes.data_as(i64p) for c in range(3)])
            b0, b1, b2 = buf[0].ctypes.data_as(i64p), buf[1].ctypes.data_as(i64p), buf[2].ctypes.data_as(u64p)
            assert gg.lib.gg_result_rows(res, 1, C.byref(n)) == GG_ERR_STATE
            assert gg.lib.gg_result_fetch(res, 1, 0, 8, ptrs, C.byref(got)) == GG_ERR_STATE
            assert gg.lib.gg_result_fetch_edges(res, 1, 0, 8, ptrs, C.byref(got)) == GG_ERR_STATE
            assert gg.lib.gg_khop_aggregate_rows(res, 1, C.byref(n)) == GG_ERR_STATE
            assert gg.lib.gg_khop_pair_counts_rows(res, 1, C.byref(n)) == GG_ERR_STATE
            levels = C.c_int()
            assert gg.lib.gg_walk_closure_levels(res, None, 0, C.byref(levels)) == GG_ERR_STATE
            for h in (table.handle, agg.handle):
                assert gg.lib.gg_components_rows(h, 0, C.byref(n)) == GG_ERR_STATE
                assert gg.lib.gg_components_fetch(h, 0, 8, b0, b1, b2, C.byref(got)) == GG_ERR_STATE
                assert gg.lib.gg_components_fetch_sizes(h, 0, 8, b1, b2, C.byref(got)) == GG_ERR_STATE
            for t in (-1, 2):
                assert gg.lib.gg_components_rows(res, t, C.byref(n)) == GG_ERR_INVALID_ARG  # a table outside {0, 1}
            assert gg.lib.gg_components_rows(None, 0, C.byref(n)) == GG_ERR_INVALID_ARG
            # the fetches' conventions: any output may be NULL, nothing past the end
            assert gg.lib.gg_components_rows(res, 0, C.byref(n)) == 0 and n.value == vid.size
            assert gg.lib.gg_components_fetch(res, vid.size - 3, 8, None, b1, None, C.byref(got)) == 0 and got.value == 3
            assert buf[1][:3].tolist() == want["component"][-3:].tolist()
            assert gg.lib.gg_components_fetch(res, 0, 8, None, None, None, C.byref(got)) == 0 and got.value == 8
            assert gg.lib.gg_components_fetch(res, vid.size, 8, b0, None, None, C.byref(got)) == 0 and got.value == 0
            total = want["stats"]["components"]
            assert gg.lib.gg_components_rows(res, 1, C.byref(n)) == 0 and n.value == total > 3
            assert gg.lib.gg_components_fetch_sizes(res, total - 2, 8, b1, b2, C.byref(got)) == 0 and got.value == 2
            assert buf[1][:2].tolist() == want["components"][-2:].tolist()
            assert buf[2][:2].tolist() == want["sizes"][-2:].tolist()
            assert gg.lib.gg_components_fetch_sizes(res, total, 8, b1, b2, C.byref(got)) == 0 and got.value == 0
        finally:
            agg.close()
            table.close()
            gg.lib.gg_result_destroy(res)
        good()
    finally:
        other.close()
        shard.close()
        csr.close()
