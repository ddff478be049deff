"""GG.extend_edge (gg_result_extend_edge) against the numpy restatement (tests/extend_ref.py): stats, row count, digest and —
for outputs under 200 000 rows — the rows and the joined rows' rowids in the input's order, for every from_col, with and
without edge columns, on the skew shapes a tile of output rows can get wrong (under gg_debug_extend and the default), on
split launches and both CSR builds, chained, on degenerate shapes and through every error.  The cross-check of independent
kernels: extending the k-hop table over the walk graph itself from its last column gives the (k + 1)-hop table of
gg_expand_khop_result / gg_expand_khop_edges.  The 2^32-row refusal of the materialising form cannot be reached at test
size; it was checked by reading csrc/gg_extend.hip only."""
import ctypes as C

import numpy as np
import pytest

from duckdb_pgq_amd import GGError
from duckdb_pgq_amd.gg import ExtendStats
from tests import edge_filter_ref as F
from tests import extend_ref as X
from tests import triangles_ref as T
from tests.oracle_lib import sort_rows

pytestmark = pytest.mark.gpu

GG_ERR_INVALID_ARG, GG_ERR_STATE = -1, -6
FETCH_BELOW = 200_000  # outputs of fewer rows are fetched and compared in order; larger ones by count and digest
PIECE = 65_536
SMALL_TILE, DEFAULT_TILE, STAGED_ROWS = 64, 1024, 1024  # gg_debug_extend(64); EX_TILE_ROWS and EX_WIN of csrc/gg_extend.hip


@pytest.fixture(scope="module")
def hard():
    """the walk graph, the creator -> message table, and the source list S = [hub, z, hub again, a person of a few rows,
    dense index 3] with its dense walk tables (computed once, never changed)"""
    vid, src, dst = T.hard_graph()
    g = T.TriangleGraph(vid, src, dst)
    es, ed, er, info = X.ext_table(g)
    light = int(es[(es != info["hub"]) & np.isin(es, g.vid)][0])
    S = np.array([info["hub"], info["z"], info["hub"], light, int(g.vid[3])], np.int64)
    walks = {h: F.walks(g, S, h) for h in (1, 2)}
    for a in (es, ed, er, *walks.values()):
        a.setflags(write=False)
    return vid, src, dst, g, (es, ed, er, info), S, walks


def build(gg, vid, src, dst, rowid=None):
    gg.staging_clear()
    gg.append_vertices(np.asarray(vid, np.int64))
    gg.append_edges(np.asarray(src, np.int64), np.asarray(dst, np.int64), rowid)
    return gg.build_csr()


def build_ext(gg, vid, es, ed, er=None):
    """the joined table's CSR: vertex set = the persons united with every endpoint, so no row is dropped and every id of
    an output row is a vertex.  Returns (csr, its id -> dense index dictionary)."""
    gg.staging_clear()
    gg.append_vertices(np.asarray(vid, np.int64))
    gg.append_edges(np.asarray(es, np.int64), np.asarray(ed, np.int64), er)
    gg.vertices_from_edges(keep_staged=True)
    csr = gg.build_csr()
    ids = csr.export()[3]
    assert csr.E == np.asarray(es).size
    return csr, {int(v): i for i, v in enumerate(ids.tolist())}


def fetch_all(res, hops, edges=False):
    """every row of table `hops` (edges: of its edge columns), in pieces of up to PIECE rows"""
    n = res.rows(hops)
    ncols = hops if edges else hops + 1
    out = np.empty((ncols, max(n, 1)), np.int64)
    i64p = C.POINTER(C.c_int64)
    fn = res.gg.lib.gg_result_fetch_edges if edges else res.gg.lib.gg_result_fetch
    for o in range(0, n, PIECE):
        ptrs = (i64p * ncols)(*[out[c, o:].ctypes.data_as(i64p) for c in range(ncols)])
        got = C.c_uint32()
        res.gg._chk(fn(res.handle, hops, o, min(PIECE, n - o), ptrs, C.byref(got)))
        assert got.value == min(PIECE, n - o)
    return out[:, :n].T.copy()


def check(gg, table_res, hops, ext_csr, ext_index, ext, fc, id_rows=None):
    """one from_col against the restatement, count-only, materialised and with edge columns.  id_rows: the input's rows if
    the caller knows them (else they are fetched).  Returns the stats."""
    es, ed, er = ext
    if id_rows is None:
        id_rows = fetch_all(table_res, hops)
    want_rows, want_rid, want = X.extend_rows(id_rows, es, ed, er, fc)
    count_only = gg.extend_edge(table_res, hops, ext_csr, fc, materialise=False)
    st, res = gg.extend_edge(table_res, hops, ext_csr, fc)
    print((hops, fc), "device", st, "restatement", want)
    try:
        assert st == want and count_only == st
        assert res.rows(hops + 1) == st["rows_out"]
        assert res.digest(ext_csr, hops + 1) == (st["rows_out"], F.digest_dense_rows(X.dense_rows(ext_index, want_rows)))
        if st["rows_out"] < FETCH_BELOW:
            assert np.array_equal(fetch_all(res, hops + 1), want_rows)
    finally:
        res.close()
    st_e, res = gg.extend_edge(table_res, hops, ext_csr, fc, edges=True)
    try:
        assert st_e == want and res.rows(hops + 1) == want["rows_out"]
        if st["rows_out"] < FETCH_BELOW:
            assert np.array_equal(fetch_all(res, hops + 1), want_rows)
            assert np.array_equal(fetch_all(res, hops + 1, edges=True)[:, hops], want_rid)
    finally:
        res.close()
    return st


@pytest.mark.parametrize("hops", [1, 2])
def test_every_from_col_equals_the_restatement(gg, hard, hops):
    vid, src, dst, g, (es, ed, er, info), S, walks = hard
    ext_csr, ext_index = build_ext(gg, vid, es, ed, er)
    csr = build(gg, vid, src, dst)
    table = gg.expand_khop_result(csr, hops, S)
    try:
        assert np.array_equal(fetch_all(table, hops), g.vid[walks[hops]])
        outs = [check(gg, table, hops, ext_csr, ext_index, (es, ed, er), fc, g.vid[walks[hops]]) for fc in range(hops + 1)]
        assert all(st["rows_out"] > 0 and 0 < st["rows_matched"] < st["rows_in"] for st in outs)
        assert outs[0]["rows_out"] >= 2 * X.HUB_ROWS  # the duplicate source: the hub's rows twice
    finally:
        table.close()
        csr.close()
        ext_csr.close()


def test_edge_columns_are_copied_or_minus_one_and_need_rowids(gg, hard):
    vid, src, dst, g, (es, ed, er, info), S, walks = hard
    ext_csr, _ = build_ext(gg, vid, es, ed, er)
    csr = build(gg, vid, src, dst)
    with_edges = gg.expand_khop_edges(csr, 2, S)
    without = gg.expand_khop_result(csr, 2, S)
    try:
        for table, has in ((with_edges, True), (without, False)):
            rows_in = fetch_all(table, 2)
            e_in = fetch_all(table, 2, edges=True) if has else np.full((rows_in.shape[0], 2), -1, np.int64)
            both, rid, want = X.extend_rows(np.concatenate([rows_in, e_in], axis=1), es, ed, er, 2)
            st, res = gg.extend_edge(table, 2, ext_csr, 2, edges=True)
            try:
                assert st == want and want["rows_out"] > 0
                assert np.array_equal(fetch_all(res, 3), both[:, [0, 1, 2, 5]])
                assert np.array_equal(fetch_all(res, 3, edges=True), np.concatenate([both[:, 3:5], rid.reshape(-1, 1)], axis=1))
            finally:
                res.close()
        plain, _ = build_ext(gg, vid, es, ed, None)  # no rowids given: the rowid is the append position
        try:
            rows, rid, want = X.extend_rows(fetch_all(without, 2), es, ed, None, 2)
            st, res = gg.extend_edge(without, 2, plain, 2, edges=True)
            assert st == want and np.array_equal(fetch_all(res, 3, edges=True)[:, 2], rid)
            assert np.array_equal(es[rid], rows[:, 2]) and np.array_equal(ed[rid], rows[:, 3])
            res.close()
        finally:
            plain.close()
        gg.set_edge_rowid(False)
        bare, _ = build_ext(gg, vid, es, ed, None)
        try:
            with pytest.raises(GGError) as e:
                gg.extend_edge(without, 2, bare, 2, edges=True)
            assert e.value.code == GG_ERR_STATE
            st, res = gg.extend_edge(without, 2, bare, 2)  # the rows need no rowid
            assert st == want and np.array_equal(fetch_all(res, 3), rows)
            with pytest.raises(GGError):
                res.fetch_edges(3, 0)
            res.close()
        finally:
            bare.close()
    finally:
        with_edges.close()
        without.close()
        csr.close()
        ext_csr.close()


def degrees(id_rows, es, fc):
    keys, n = np.unique(es, return_counts=True)
    at = np.clip(np.searchsorted(keys, id_rows[:, fc]), 0, keys.size - 1)
    return np.where(keys[at] == id_rows[:, fc], n[at], 0)


@pytest.mark.parametrize("shape", ["long_parent", "zero_run_then_parent"])
def test_skew_shapes_give_identical_rows_for_every_tile(gg, hard, shape):
    """long_parent: every input row has the hub's rows — a parent spans 46 small and 2.9 default tiles.
    zero_run_then_parent: the 2-hop table of [z, hub] from column 0 — more rows without an edge row than a small tile has
    rows (17 times) and than a tile stages input rows, then a parent of many tiles, so tile 0 holds both at either size."""
    vid, src, dst, g, (es, ed, er, info), S, walks = hard
    ext_csr, ext_index = build_ext(gg, vid, es, ed, er)
    csr = build(gg, vid, src, dst)
    hops, sources = (1, [info["hub"]]) if shape == "long_parent" else (2, [info["z"], info["hub"]])
    table = gg.expand_khop_result(csr, hops, np.array(sources, np.int64))
    try:
        id_rows = fetch_all(table, hops)
        deg = degrees(id_rows, es, 0)
        if shape == "long_parent":
            assert deg.min() >= 8 * SMALL_TILE and deg.min() >= 2 * DEFAULT_TILE
        else:
            run = int(np.argmax(deg > 0))  # the rows before the first one with an edge row
            assert run >= 4 * SMALL_TILE and run > STAGED_ROWS and deg[run] >= 8 * SMALL_TILE and deg[run] >= 2 * DEFAULT_TILE
        want_rows, want_rid, want = X.extend_rows(id_rows, es, ed, er, 0)
        assert 0 < want["rows_out"] < FETCH_BELOW
        for tile in (SMALL_TILE, 0, 100, 1):
            gg.debug_extend(tile)
            st, res = gg.extend_edge(table, hops, ext_csr, 0, edges=True)
            try:
                assert st == want, tile
                assert np.array_equal(fetch_all(res, hops + 1), want_rows), tile
                assert np.array_equal(fetch_all(res, hops + 1, edges=True)[:, hops], want_rid), tile
            finally:
                res.close()
        gg.debug_reset()
        st, res = gg.extend_edge(table, hops, ext_csr, 0)
        assert np.array_equal(fetch_all(res, hops + 1), want_rows)  # gg_debug_reset restores the default tile
        res.close()
    finally:
        table.close()
        csr.close()
        ext_csr.close()


@pytest.mark.parametrize("route", ["grid1", "grid1_small_tile", "legacy_build"])
def test_split_launches_and_both_builds(gg, hard, route):
    vid, src, dst, g, (es, ed, er, info), S, walks = hard
    if route == "legacy_build":
        gg.force_legacy_build(True)
    ext_csr, ext_index = build_ext(gg, vid, es, ed, er)
    csr = build(gg, vid, src, dst)
    table = gg.expand_khop_result(csr, 2, S)
    if route.startswith("grid1"):
        gg.max_grid_tiles(1)  # one workgroup a launch: 256 input rows, one output tile
    if route == "grid1_small_tile":
        gg.debug_extend(SMALL_TILE)
    try:
        check(gg, table, 2, ext_csr, ext_index, (es, ed, er), 2, g.vid[walks[2]])
        check(gg, table, 2, ext_csr, ext_index, (es, ed, er), 1, g.vid[walks[2]])
    finally:
        table.close()
        csr.close()
        ext_csr.close()


@pytest.mark.parametrize("k", [1, 2])
def test_over_the_walk_graph_it_is_the_next_hop_of_the_expansion(gg, hard, k):
    vid, src, dst, g, (es, ed, er, info), S, walks = hard
    csr = build(gg, vid, src, dst)
    table = gg.expand_khop_edges(csr, k, S)
    longer = gg.expand_khop_result(csr, k + 1, S)
    longer_e = gg.expand_khop_edges(csr, k + 1, S)
    try:
        st, res = gg.extend_edge(table, k, csr, k)
        st_e, res_e = gg.extend_edge(table, k, csr, k, edges=True)
        try:
            n = longer.rows(k + 1)
            assert st["rows_out"] == st_e["rows_out"] == res.rows(k + 1) == n == longer_e.rows(k + 1) > 0
            assert res.digest(csr, k + 1) == longer.digest(csr, k + 1) and res.digest(csr, k + 1)[0] == n
            assert np.array_equal(sort_rows(fetch_all(res, k + 1)), sort_rows(fetch_all(longer, k + 1)))
            got = np.concatenate([fetch_all(res_e, k + 1), fetch_all(res_e, k + 1, edges=True)], axis=1)
            want = np.concatenate([fetch_all(longer_e, k + 1), fetch_all(longer_e, k + 1, edges=True)], axis=1)
            assert np.array_equal(sort_rows(got), sort_rows(want))
        finally:
            res.close()
            res_e.close()
    finally:
        table.close()
        longer.close()
        longer_e.close()
        csr.close()


def test_chains_message_then_tag_and_a_filter_on_the_new_column(gg, hard):
    vid, src, dst, g, (es, ed, er, info), S, walks = hard
    ts, td, tr = X.tag_table(ed)
    ext_csr, _ = build_ext(gg, vid, es, ed, er)
    gg.staging_clear()
    gg.append_edges(ts, td, tr)
    gg.vertices_from_edges()  # messages and tags only: a person in column w matches nothing unless it is a message too
    tag_csr = gg.build_csr()
    csr = build(gg, vid, src, dst)
    table = gg.expand_khop_result(csr, 1, S)
    try:
        st1, first = gg.extend_edge(table, 1, ext_csr, 1, edges=True)
        try:
            r1, rid1, w1 = X.extend_rows(g.vid[walks[1]], es, ed, er, 1)
            assert st1 == w1 and w1["rows_out"] > 0
            # knows -> message -> tag (interactive-complex-4.sql:2-8)
            st2, second = gg.extend_edge(first, 2, tag_csr, 2, edges=True)
            try:
                both, rid2, w2 = X.extend_rows(np.concatenate([r1, rid1.reshape(-1, 1)], axis=1), ts, td, tr, 2)
                assert st2 == w2 and 0 < w2["rows_matched"] < w2["rows_in"]
                assert np.array_equal(fetch_all(second, 3), both[:, [0, 1, 2, 4]])
                e = fetch_all(second, 3, edges=True)
                assert (e[:, 0] == -1).all() and np.array_equal(e[:, 1], both[:, 3]) and np.array_equal(e[:, 2], rid2)
            finally:
                second.close()
            # and a branch: the creator's messages again, off the middle column of the longer rows
            st3, third = gg.extend_edge(first, 2, ext_csr, 1)
            try:
                r3, _, w3 = X.extend_rows(r1, es, ed, er, 1)
                assert st3 == w3 and third.rows(3) == r3.shape[0]
                if r3.shape[0] < FETCH_BELOW:
                    assert np.array_equal(fetch_all(third, 3), r3)
            finally:
                third.close()
            # the filter on the new column: messages whose id is a person who knows v0
            for mode in ("semi", "anti"):
                stf, kept = gg.filter_edge(first, 2, csr, 2, 0, mode)
                try:
                    want_rows, want = F.filter_graph(g, r1, 2, 0, mode)
                    assert stf == want and np.array_equal(fetch_all(kept, 2), want_rows)
                finally:
                    kept.close()
            out = C.c_void_p()
            gg._chk(gg.lib.gg_result_filter_common_neighbour(gg.ctx, first.handle, 2, csr.handle, C.byref(out)))
            gg.lib.gg_result_destroy(out)
        finally:
            first.close()
    finally:
        table.close()
        csr.close()
        tag_csr.close()
        ext_csr.close()


@pytest.mark.parametrize("n_rows_wanted", [1, 63, 65, 257, 1000])
def test_row_counts_that_are_no_multiple_of_the_wavefront_or_the_workgroup(gg, n_rows_wanted):
    """a star: the 1-hop table of the centre has n rows; leaf i has i % 5 rows in the joined table"""
    n = n_rows_wanted
    vid = np.arange(100, 100 + n + 1, dtype=np.int64)
    leaves = vid[1:]
    es = np.repeat(leaves, np.arange(n) % 5)
    ed = 9000 + np.arange(es.size, dtype=np.int64)
    ext_csr, ext_index = build_ext(gg, vid, es, ed, None)
    csr = build(gg, vid, np.full(n, vid[0], np.int64), leaves)
    table = gg.expand_khop_result(csr, 1, vid[:1])
    try:
        assert table.rows(1) == n
        for tile in (0, 3):
            gg.debug_extend(tile)
            check(gg, table, 1, ext_csr, ext_index, (es, ed, None), 1)
    finally:
        table.close()
        csr.close()
        ext_csr.close()


def test_degenerate_shapes(gg):
    vid = np.array([10, 20, 30], np.int64)
    csr = build(gg, vid, np.array([10, 20], np.int64), np.array([20, 10], np.int64))
    ext_csr, _ = build_ext(gg, vid, np.array([30, 30], np.int64), np.array([77, 78], np.int64))
    bare = build(gg, vid, np.empty(0, np.int64), np.empty(0, np.int64))
    zero = {"rows_in": 0, "rows_out": 0, "rows_matched": 0}
    try:
        empty = gg.expand_khop_result(csr, 2, np.empty(0, np.int64))  # an empty input table
        two = gg.expand_khop_result(csr, 1, None)                     # (10, 20), (20, 10)
        try:
            for edges in (False, True):
                st, res = gg.extend_edge(empty, 2, ext_csr, 2, edges=edges)
                assert st == zero and res.handle and res.rows(3) == 0 and fetch_all(res, 3).shape == (0, 4)
                res.close()
                for graph in (bare, ext_csr):  # a joined table without rows; one of which no row matches
                    st, res = gg.extend_edge(two, 1, graph, 1, edges=edges)
                    assert st == {"rows_in": 2, "rows_out": 0, "rows_matched": 0} and res.rows(2) == 0
                    assert fetch_all(res, 2).shape == (0, 3)
                    st2, again = gg.extend_edge(res, 2, ext_csr, 0)  # and an empty result is an input like any other
                    assert st2 == zero and again.rows(3) == 0
                    again.close()
                    res.close()
            assert gg.extend_edge(empty, 2, bare, 0, materialise=False) == zero
            st, res = gg.extend_edge(two, 1, csr, 0, edges=True)  # one edge row each: (10, 20, 20), (20, 10, 10)
            assert st == {"rows_in": 2, "rows_out": 2, "rows_matched": 2}
            assert fetch_all(res, 2).tolist() == [[10, 20, 20], [20, 10, 10]]
            assert fetch_all(res, 2, edges=True).tolist() == [[-1, 0], [-1, 1]]
            res.close()
        finally:
            empty.close()
            two.close()
    finally:
        bare.close()
        ext_csr.close()
        csr.close()


def test_errors_leave_the_context_usable(gg, hard):
    vid, src, dst, g, (es, ed, er, info), S, walks = hard
    ext_csr, _ = build_ext(gg, vid, es, ed, er)
    gg.staging_clear()
    gg.append_vertices(vid)
    gg.append_edges(src, dst)
    shard = gg.build_csr_shard(0, 2)
    csr = gg.build_csr()
    table = gg.expand_khop_result(csr, 2, S)
    full = gg.expand_khop_result(csr, 8, vid[:1] * 0 - 123456)  # GG_MAX_HOPS hops of a source that is no vertex: 0 rows
    closure = gg.walk_closure(csr, S[4:5], max_levels=2)
    other = type(gg)(0)
    other.append_vertices(vid[:4])
    other.append_edges(vid[:2], vid[2:4])
    foreign = other.build_csr()
    want = X.extend_rows(g.vid[walks[2]], es, ed, er, 2)[2]

    def call(res, hops, graph, fc, edges=0, materialise=1, out=True, ctx=None):
        st, o = ExtendStats(), C.c_void_p()
        rc = gg.lib.gg_result_extend_edge(ctx or gg.ctx, res, hops, graph, fc, edges, materialise, C.byref(st),
                                          C.byref(o) if out else None)
        assert rc != 0 and not o.value
        return rc

    try:
        bad = [
            (call(table.handle, 2, shard.handle, 2), GG_ERR_STATE),              # a shard CSR
            (call(closure.handle, 2, csr.handle, 2), GG_ERR_STATE),              # no fixed-length table
            (call(table.handle, 2, ext_csr.handle, 3), GG_ERR_INVALID_ARG),      # column hops + 1
            (call(table.handle, 2, ext_csr.handle, -1), GG_ERR_INVALID_ARG),     # column -1
            (call(table.handle, 3, ext_csr.handle, 2), GG_ERR_INVALID_ARG),      # hops outside the result
            (call(table.handle, 1, ext_csr.handle, 1), GG_ERR_INVALID_ARG),
            (call(full.handle, 8, ext_csr.handle, 0), GG_ERR_INVALID_ARG),       # hops + 1 > GG_MAX_HOPS
            (call(None, 2, ext_csr.handle, 2), GG_ERR_INVALID_ARG),
            (call(table.handle, 2, None, 2), GG_ERR_INVALID_ARG),
            (call(table.handle, 2, foreign.handle, 2), GG_ERR_INVALID_ARG),      # a CSR of another context
            (call(table.handle, 2, ext_csr.handle, 2, ctx=other.ctx), GG_ERR_INVALID_ARG),
            (call(table.handle, 2, ext_csr.handle, 2, out=False), GG_ERR_INVALID_ARG),  # materialise without out_result
        ]
        for i, (rc, code) in enumerate(bad):
            assert rc == code, (i, rc, code)
            assert gg.extend_edge(table, 2, ext_csr, 2, materialise=False) == want  # a correct call still works
        st = ExtendStats()  # count mode takes a NULL out_result
        assert gg.lib.gg_result_extend_edge(gg.ctx, table.handle, 2, ext_csr.handle, 2, 0, 0, C.byref(st), None) == 0
        assert int(st.rows_out) == want["rows_out"]
        with pytest.raises(GGError) as e:
            gg.extend_edge(table, 2, shard, 2)
        assert e.value.code == GG_ERR_STATE
    finally:
        foreign.close()
        other.close()
        closure.close()
        full.close()
        table.close()
        shard.close()
        csr.close()
        ext_csr.close()
