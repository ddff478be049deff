"""The walk-row operators (gg_result_filter_edge, gg_result_filter_common_neighbour, gg_result_extend_edge,
gg_result_group_by, gg_result_filter_value, gg_result_top_rows) on tables of 4 to 8 hops — up to 9 id columns and 8 edge
columns, the widest they accept — against the numpy restatements (tests/edge_filter_ref.py, extend_ref.py, group_by_ref.py,
value_rows_ref.py; pinned at this width by tests/test_wide_rows_ref_cpu.py).

The tables are the walks of deep_graphs.sources_of over the small shapes of tests/deep_graphs.py, made by both producers
(gg_expand_khop_edges carries edge columns, gg_expand_khop_result none), and the 8-hop table with 8 edge columns that the
extension of the 7-hop one over deep_graphs.ext_table gives.  Every check runs with default launches and under
gg_debug_max_grid_tiles(1), where the split-launch loops pass a non-zero first group or tile.  Every comparison is of
integers, in order (the same-neighbour filter's rows alone are compared sorted, as tests/test_gpu_deep_walks.py compares
them).  test_full_width_chain_and_its_kernels asserts that the write kernels ran on 8-hop tables, so that a
changed route cannot turn this file into a repeat of the narrow tests.

The 2^32-row refusals cannot be reached at test size; they remain checked by reading csrc/ only."""
import numpy as np
import pytest

from duckdb_pgq_amd import GGError
from tests import deep_graphs as D
from tests import edge_filter_ref as F
from tests import extend_ref as X
from tests import group_by_ref as G
from tests import khop_aggregate_ref as K
from tests import khop_aggregate_top_ref as TOP
from tests import triangles_ref as T
from tests import value_rows_ref as R
from tests import wide_rows_ref as W
from tests.oracle_lib import sort_rows
from tests.test_gpu_deep_walks import launched
from tests.test_gpu_extend import build, build_ext, fetch_all
from tests.test_gpu_group_by import check as check_group
from tests.test_gpu_value_rows import KNOBS, check_filter, check_top, id_values

pytestmark = pytest.mark.gpu

GG_ERR_INVALID_ARG = -1
LO, HI = R.I64_MIN, R.I64_MAX
SHAPES = D.SMALL
ALIVE = [n for n in SHAPES if n != "dying"]
HOPS = [4, 5, 6, 7, 8]
TILES = (0, 1)  # gg_debug_max_grid_tiles: the default, and one workgroup a launch


class World:
    """the device objects of one (shape, hops): the walk CSR, the second table's CSR and the `hops`-hop table of both
    producers, each checked against the CPU walk rows in order"""

    def __init__(self, gg, name, hops):
        self.gg, self.name, self.hops = gg, name, hops
        self.vid, self.src, self.dst, self.g, self.S = W.world(name)
        self.es, self.ed, self.er, self.info = D.ext_table(name)
        self.opened = []
        self.ext_csr, self.ext_index = build_ext(gg, self.vid, self.es, self.ed, self.er)
        self.own(self.ext_csr)
        self.ext_ids = self.ext_csr.export()[3]
        self.csr = self.own(build(gg, self.vid, self.src, self.dst))
        self.rows = W.walk_rows(name, hops)
        self.with_edges = self.own(gg.expand_khop_edges(self.csr, hops, self.S))
        self.plain = self.own(gg.expand_khop_result(self.csr, hops, self.S))
        for table in (self.with_edges, self.plain):
            assert table.rows(hops) == W.ROWS[name][hops - 1]
            assert np.array_equal(fetch_all(table, hops), self.rows)
        self.edges = fetch_all(self.with_edges, hops, edges=True)
        assert self.edges.shape == (self.rows.shape[0], hops) and (self.edges >= 0).all()
        # (table, its id rows, its edge columns or None)
        self.tables = [(self.with_edges, self.rows, self.edges), (self.plain, self.rows, None)]

    def own(self, obj):
        self.opened.insert(0, obj)
        return obj

    def extended(self, from_col):
        """the (hops + 1)-hop table with hops + 1 edge columns: the table with edge columns extended over the second table;
        (result, id rows, edge columns), the latter two from the restatement"""
        both, rid, want = X.extend_rows(np.concatenate([self.rows, self.edges], axis=1), self.es, self.ed, self.er, from_col)
        n = self.hops + 1
        rows = both[:, list(range(n)) + [both.shape[1] - 1]]
        edges = np.concatenate([both[:, n:2 * n - 1], rid.reshape(-1, 1)], axis=1)
        st, res = self.gg.extend_edge(self.with_edges, self.hops, self.ext_csr, from_col, edges=True)
        self.own(res)
        assert st == want
        return res, rows, edges

    def close(self):
        for o in self.opened:
            o.close()


@pytest.fixture
def world(gg, request):
    made = []

    def make(name, hops):
        made.append(World(gg, name, hops))
        return made[-1]

    yield make
    for w in made:
        w.close()


def no_edge_columns(res, hops):
    """a table with rows and without edge columns refuses gg_result_fetch_edges"""
    if res.rows(hops):
        with pytest.raises(GGError) as e:
            res.fetch_edges(hops, 0)
        assert e.value.code == GG_ERR_INVALID_ARG


# ---- gg_result_filter_edge ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", SHAPES)
@pytest.mark.parametrize("hops", HOPS)
def test_filter_edge_every_mode_and_column_pair(gg, world, name, hops):
    w = world(name, hops)
    selective = False
    for fc, tc in W.column_pairs(hops):
        for mode in F.MODES:
            want_rows, want = F.filter_graph(w.g, w.rows, fc, tc, mode)
            selective = selective or 0 < want["rows_out"] < want["rows_in"]
            for tiles in TILES:
                gg.max_grid_tiles(tiles)
                for table, _, _ in w.tables:
                    assert gg.filter_edge(table, hops, w.csr, fc, tc, mode, materialise=False) == want, (fc, tc, mode, tiles)
                    st, res = gg.filter_edge(table, hops, w.csr, fc, tc, mode)
                    try:
                        assert st == want, (fc, tc, mode, tiles)
                        assert res.rows(hops) == want["rows_out"]
                        assert np.array_equal(fetch_all(res, hops), want_rows), (fc, tc, mode, tiles)
                        no_edge_columns(res, hops)
                    finally:
                        res.close()
    assert selective == (w.rows.shape[0] > 0)


@pytest.mark.parametrize("name", ALIVE)
def test_the_hub_shape_pair_that_matches_nothing_is_one_of_the_cases(name):
    """(no device call) v_0 -> v_h keeps some rows on two shapes and none on the hub at 6 and 8 hops, where another pair
    of the cases above is the selective one"""
    g = W.world(name)[3]
    for hops in (6, 8):
        assert (0, hops) in W.column_pairs(hops)
        kept = F.filter_graph(g, W.walk_rows(name, hops), 0, hops, "semi")[1]["rows_out"]
        assert (kept == 0) == (name == "hub")


# ---- gg_result_filter_common_neighbour ---------------------------------------------------------------------------------


def sensors_of(vid):
    """tests/test_gpu_deep_walks.py's second graph: most vertices watched by sensor 0 (some twice), a few by sensor 1 as
    well or instead, some by none; (sensor ids, edge sources, edge destinations)"""
    rng = np.random.default_rng(91)
    sensors = vid.max() + 1000 + np.arange(3, dtype=np.int64)
    m_src, m_dst = [], []
    for v in vid.tolist():
        r = rng.random()
        ws = [0] if r < 0.75 else [0, 0] if r < 0.85 else [0, 1] if r < 0.93 else [1] if r < 0.97 else []
        for s in ws:
            m_src.append(v)
            m_dst.append(int(sensors[s]))
    return sensors, np.array(m_src, np.int64), np.array(m_dst, np.int64)


def same_neighbour_rows(g, paths, sensors, m_src, m_dst):
    """for every path row and every sensor w, the row (w, v0..vh) prod_c mult(v_c, w) times"""
    dense = F.dense_of(g.index, paths.reshape(-1)).reshape(paths.shape)
    out = []
    for w in sensors.tolist():
        per_vertex = np.bincount(F.dense_of(g.index, m_src[m_dst == w]), minlength=g.V)
        m = per_vertex[dense].prod(axis=1) if paths.shape[0] else np.zeros(0, np.int64)
        kept = np.repeat(paths, m, axis=0)
        out.append(np.concatenate([np.full((kept.shape[0], 1), w, np.int64), kept], axis=1))
    return np.concatenate(out, axis=0)


@pytest.mark.parametrize("name", SHAPES)
def test_same_neighbour_filter_at_four_to_seven_hops(gg, name):
    vid, src, dst, g, S = W.world(name)
    sensors, m_src, m_dst = sensors_of(vid)
    gg.staging_clear()
    gg.append_vertices(np.concatenate([vid, sensors]))
    gg.append_edges(src, dst)
    path_csr = gg.build_csr()
    gg.staging_clear_edges()
    gg.append_edges(m_src, m_dst)
    filter_csr = gg.build_csr()
    try:
        for hops in (4, 5, 6, 7):
            want = same_neighbour_rows(g, W.walk_rows(name, hops), sensors, m_src, m_dst)
            assert (want.shape[0] > 0) == (name != "dying")
            for tiles in TILES:
                gg.max_grid_tiles(tiles)
                got, names = launched(gg, lambda: gg.connected_paths_same_neighbour(path_csr, filter_csr, hops, S))
                assert got.shape[0] == want.shape[0], (hops, tiles)
                if want.shape[0]:
                    assert np.array_equal(sort_rows(got), sort_rows(want)), (hops, tiles)
                    assert "filter_fill" in names, names
    finally:
        path_csr.close()
        filter_csr.close()


# ---- gg_result_extend_edge ---------------------------------------------------------------------------------------------


def check_extend(gg, w, from_col, tag):
    hops = w.hops
    for table, rows, edges in w.tables:
        want_rows, want_rid, want = X.extend_rows(rows, w.es, w.ed, w.er, from_col)
        assert gg.extend_edge(table, hops, w.ext_csr, from_col, materialise=False) == want, (from_col, tag)
        st, res = gg.extend_edge(table, hops, w.ext_csr, from_col)
        try:
            assert st == want and res.rows(hops + 1) == want["rows_out"], (from_col, tag)
            assert np.array_equal(fetch_all(res, hops + 1), want_rows), (from_col, tag)
            no_edge_columns(res, hops + 1)
        finally:
            res.close()
        # with edge columns: the inherited ones are the producer's, repeated per parent, or -1; the new one is the rowid
        e_in = edges if edges is not None else np.full((rows.shape[0], hops), -1, np.int64)
        both, rid, want_e = X.extend_rows(np.concatenate([rows, e_in], axis=1), w.es, w.ed, w.er, from_col)
        assert want_e == want and np.array_equal(rid, want_rid)
        st, res = gg.extend_edge(table, hops, w.ext_csr, from_col, edges=True)
        try:
            assert st == want and res.rows(hops + 1) == want["rows_out"], (from_col, tag)
            assert np.array_equal(fetch_all(res, hops + 1), want_rows), (from_col, tag)
            got_e = fetch_all(res, hops + 1, edges=True)
            assert got_e.shape == (want["rows_out"], hops + 1)
            assert np.array_equal(got_e[:, :hops], both[:, hops + 1:2 * hops + 1]), (from_col, tag)
            assert np.array_equal(got_e[:, hops], want_rid), (from_col, tag)
            if edges is None:
                assert (got_e[:, :hops] == -1).all()
        finally:
            res.close()
    return want


@pytest.mark.parametrize("name", SHAPES)
@pytest.mark.parametrize("hops", [4, 5, 6, 7])
def test_extend_edge_from_every_kind_of_column(gg, world, name, hops):
    w = world(name, hops)
    for from_col in (0, 3, hops):
        for tiles in TILES:
            gg.max_grid_tiles(tiles)
            want = check_extend(gg, w, from_col, ("tiles", tiles))
        gg.max_grid_tiles(0)
        gg.debug_extend(tile_rows=64)
        check_extend(gg, w, from_col, "tile_rows 64")
        gg.debug_extend(0)
        if w.rows.shape[0]:
            assert 0 < want["rows_matched"] < want["rows_in"]
            assert from_col or want["rows_out"] > D.EXT_HUB_ROWS  # the long key stands in column 0


@pytest.mark.parametrize("name", SHAPES)
def test_extend_edge_refuses_eight_hops_with_rows_or_without(gg, world, name):
    w = world(name, 8)
    assert (w.rows.shape[0] > 0) == (name != "dying")
    for table, _, _ in w.tables:
        for edges in (False, True):
            for materialise in (False, True):
                with pytest.raises(GGError) as e:
                    gg.extend_edge(table, 8, w.ext_csr, 0, edges=edges, materialise=materialise)
                assert e.value.code == GG_ERR_INVALID_ARG
    st = gg.filter_edge(w.plain, 8, w.csr, 0, 8, "anti", materialise=False)  # the context still serves
    assert st["rows_in"] == w.rows.shape[0]


# ---- gg_result_group_by ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", SHAPES)
@pytest.mark.parametrize("hops", HOPS)
def test_group_by_every_kind_of_key_and_weight_column(gg, world, name, hops):
    w = world(name, hops)
    heavy = int(np.bincount(F.dense_of(w.g.index, w.rows[:, 4])).argmax()) if w.rows.shape[0] else 0
    weights = G.hub_weights(w.vid, int(w.vid[heavy]))  # -2^63 on the most frequent cell of column 4: the sum carries
    carried = False
    for kc in (0, 4, hops):
        for wc in [None] + sorted({0, hops, kc}):
            for route in (1, 2):
                for tiles in TILES:
                    gg.debug_group(route)
                    gg.max_grid_tiles(tiles)
                    for table, rows, _ in w.tables:
                        st, level = check_group(gg, table, hops, rows, kc, w.csr, w.vid, wc, None, None,
                                                None if wc is None else weights, route=route)
                        carried = carried or any(abs(int(t)) >= 1 << 64 for t in level[2])
    assert carried == (w.rows.shape[0] > 0)


@pytest.mark.parametrize("name", SHAPES)
def test_group_by_the_new_column_of_the_eight_hop_extension(gg, world, name):
    w = world(name, 7)
    res, rows, _ = w.extended(0)
    weights = np.arange(w.ext_ids.size, dtype=np.int64) * 1_000_003 - (1 << 62)
    person_weights = G.hub_weights(w.vid, w.info["hub"])
    for route in (1, 2):
        for tiles in TILES:
            gg.debug_group(route)
            gg.max_grid_tiles(tiles)
            st, level = check_group(gg, res, 8, rows, 8, w.ext_csr, w.ext_ids)  # count(*) per next id
            assert (st["groups"] > 1) == (rows.shape[0] > 0) and st["rows_grouped"] == rows.shape[0]
            check_group(gg, res, 8, rows, 8, w.ext_csr, w.ext_ids, 8, None, None, weights)
            check_group(gg, res, 8, rows, 8, w.ext_csr, w.ext_ids, 0, w.csr, w.vid, person_weights)
            check_group(gg, res, 8, rows, 0, w.csr, w.vid, 8, w.ext_csr, w.ext_ids, weights)


# ---- gg_result_filter_value and gg_result_top_rows ---------------------------------------------------------------------


def bounds_of(x_valued):
    """test_gpu_value_rows.bounds_of's selective, everything, nothing and lo_above_hi; fixed bounds for a table without a
    valued row"""
    s = np.sort(np.asarray(x_valued, np.int64))
    if s.size == 0:
        return {"selective": (-5, 5), "everything": (LO, HI), "nothing": (7, 7), "lo_above_hi": (5, -5)}
    absent = int(s[s.size // 2]) + 1
    while absent in set(s.tolist()):
        absent += 1
    return {"selective": (int(s[s.size // 4]), int(s[s.size // 2])), "everything": (LO, HI), "nothing": (absent, absent),
            "lo_above_hi": (int(s[s.size // 2]), int(s[s.size // 4]) - 1)}


def value_tables(w):
    """(table, hops, id rows, edge columns or None, the value CSR and ids of every value column) of the producers' tables
    and, from the 7-hop world, of the 8-hop extension with 8 edge columns"""
    walk = (w.csr, w.vid)
    out = [(table, w.hops, rows, edges, {c: walk for c in (0, 4, w.hops)}) for table, rows, edges in w.tables]
    if w.hops == 7:
        res, rows, edges = w.extended(0)
        assert edges.shape[1] == 8 and (edges != -1).all()
        out.append((res, 8, rows, edges, {0: walk, 4: walk, 8: (w.ext_csr, w.ext_ids)}))
    return out


@pytest.mark.parametrize("name", SHAPES)
@pytest.mark.parametrize("hops", HOPS)
def test_filter_value_every_kind_of_column_mode_bound_and_bitmap(gg, world, name, hops):
    w = world(name, hops)
    for table, h, rows, edges, graphs in value_tables(w):
        seen = {}
        for col, (csr, ids) in graphs.items():
            values = id_values(ids, "full")
            for valid in (None, R.pack_valid(np.arange(ids.size) % 5 != 2)):
                has, x = R.row_values(rows, col, ids, values, valid)
                for bname, (lo, hi) in bounds_of(x[has]).items():
                    for mode in ("in", "not_in"):
                        for tiles in TILES:
                            gg.max_grid_tiles(tiles)
                            st = check_filter(gg, table, h, rows, edges, col, csr, ids, values, valid, lo, hi, mode)
                            if edges is None:
                                _, out = gg.filter_value(table, h, col, csr, values, valid, lo, hi, mode)
                                try:
                                    no_edge_columns(out, h)
                                finally:
                                    out.close()
                        seen[(col, valid is None, bname, mode)] = st
        n = rows.shape[0]
        for col in graphs:
            assert seen[(col, True, "everything", "in")]["rows_out"] == seen[(col, True, "lo_above_hi", "not_in")]["rows_out"]
            assert seen[(col, True, "nothing", "in")]["rows_out"] == 0 == seen[(col, True, "lo_above_hi", "in")]["rows_out"]
            if n:
                assert 0 < seen[(col, True, "selective", "in")]["rows_out"] < n
                assert seen[(col, False, "everything", "in")]["rows_valued"] < n  # the bitmap takes some values away
        if n:
            assert seen[(0, True, "everything", "in")]["rows_out"] == n


@pytest.mark.parametrize("name", SHAPES)
@pytest.mark.parametrize("hops", HOPS)
@pytest.mark.parametrize("desc", [True, False])
def test_top_rows_with_ties_under_every_route(gg, world, name, hops, desc):
    w = world(name, hops)
    for table, h, rows, edges, graphs in value_tables(w):
        csr, ids = graphs[h]
        values = id_values(ids, "seven")
        n_rows = rows.shape[0]
        if n_rows:
            assert np.unique(R.row_values(rows, h, ids, values)[1]).size == 7
        for tie in (None, 0, h):
            for tiles in TILES:
                gg.max_grid_tiles(tiles)
                cand = check_top(gg, table, h, rows, edges, h, csr, ids, values, None, LO, HI, "in", desc, tie,
                                 lambda cand: sorted({0, 1, 100, n_rows, n_rows + 1}), knobs=KNOBS)
                assert cand == n_rows
                if edges is None and n_rows:
                    _, out = gg.top_rows(table, h, h, csr, values, 1, None, LO, HI, "in", desc, tie)
                    try:
                        no_edge_columns(out, h)
                    finally:
                        out.close()


# ---- one chain at full width, and the kernels it must launch -------------------------------------------------------------


@pytest.mark.parametrize("name", SHAPES)
def test_full_width_chain_and_its_kernels(gg, world, name):
    """expand_khop_edges(7) -> extend_edge(edges) -> filter_value -> filter_edge(semi, 0 -> 8) -> group_by(key_col 8) ->
    khop_aggregate_top, and top_rows of the 8-hop table: every stage against its restatement, the digests of the 8-hop
    tables against the row digest, and — where the tables have rows — the full-width write kernels among the launches"""
    w = world(name, 7)
    alive = name != "dying"
    dense = lambda rows: X.dense_rows(w.ext_index, rows)
    digest = lambda rows: (rows.shape[0], F.digest_dense_rows(dense(rows)))
    # the extension, from the walks' last column
    both, rid, want1 = X.extend_rows(np.concatenate([w.rows, w.edges], axis=1), w.es, w.ed, w.er, 7)
    rows1 = both[:, list(range(8)) + [15]]
    edges1 = np.concatenate([both[:, 8:15], rid.reshape(-1, 1)], axis=1)
    (st1, t1), names = launched(gg, lambda: gg.extend_edge(w.with_edges, 7, w.ext_csr, 7, edges=True))
    w.own(t1)
    assert st1 == want1 and (want1["rows_out"] > 0) == alive
    assert np.array_equal(fetch_all(t1, 8), rows1) and np.array_equal(fetch_all(t1, 8, edges=True), edges1)
    assert t1.digest(w.ext_csr, 8) == digest(rows1)
    assert not alive or "k_extend_write_edges" in names, names
    # rows whose next id has a value between the first and the seventh octile
    values = id_values(w.ext_ids, "full")
    has, x = R.row_values(rows1, 8, w.ext_ids, values)
    s = np.sort(x[has])
    lo, hi = (int(s[s.size // 8]), int(s[(7 * s.size) // 8])) if alive else (-5, 5)
    rows2, edges2, want2 = R.filter_rows(rows1, edges1, 8, w.ext_ids, values, None, lo, hi, "in")
    (st2, t2), names = launched(gg, lambda: gg.filter_value(t1, 8, 8, w.ext_csr, values, None, lo, hi))
    w.own(t2)
    assert st2 == want2 and (0 < want2["rows_out"] < want2["rows_in"]) == alive
    assert np.array_equal(fetch_all(t2, 8), rows2) and np.array_equal(fetch_all(t2, 8, edges=True), edges2)
    assert t2.digest(w.ext_csr, 8) == digest(rows2)
    assert not alive or "k_value_write" in names, names
    # a condition graph over the second table's vertices: every other distinct (v0, v8) pair, every fourth one twice
    pairs = np.unique(rows2[:, [0, 8]], axis=0)[::2]
    pairs = np.concatenate([pairs, pairs[::2]], axis=0)
    cond = T.TriangleGraph(w.ext_ids, pairs[:, 0], pairs[:, 1])
    cond_csr = w.own(build(gg, w.ext_ids, pairs[:, 0], pairs[:, 1]))
    rows3, want3 = F.filter_graph(cond, rows2, 0, 8, "semi")
    (st3, t3), names = launched(gg, lambda: gg.filter_edge(t2, 8, cond_csr, 0, 8, "semi"))
    w.own(t3)
    assert st3 == want3 and (0 < want3["rows_out"] < want3["rows_in"]) == alive
    assert not alive or want3["matches"] > want3["rows_out"]
    assert np.array_equal(fetch_all(t3, 8), rows3)
    no_edge_columns(t3, 8)
    assert t3.digest(w.ext_csr, 8) == digest(rows3)
    assert not alive or "k_edge_filter_write" in names, names
    # count(*) per next id, ordered
    level, want4 = G.group_by(rows3, 8, w.ext_ids)
    agg, names = launched(gg, lambda: gg.group_by(t3, 8, 8, w.ext_csr))
    w.own(agg)
    st4 = dict(agg.stats)
    st4.pop("route")
    assert st4 == want4 and (want4["groups"] > 1) == alive
    assert K.same(agg.fetch(8), level)
    assert not alive or any(k.startswith("k_group_accum") for k in names), names
    for n in (1, 10, len(level[0]) + 1):
        top = gg.khop_aggregate_top(agg, 8, "walks", True, n)
        try:
            assert K.same(top.fetch(8), TOP.top(level, n, "walks", True))
        finally:
            top.close()
    # the best 100 rows of the 8-hop table by a seven-valued column, ties by the next id
    seven = id_values(w.ext_ids, "seven")
    rows5, edges5, want5 = R.top_rows(rows1, edges1, 8, w.ext_ids, seven, None, LO, HI, "in", True, 8, 100)
    (st5, t5), names = launched(gg, lambda: gg.top_rows(t1, 8, 8, w.ext_csr, seven, 100, None, LO, HI, "in", True, 8))
    w.own(t5)
    assert {k: st5[k] for k in want5} == want5 and (want5["rows_out"] == 100) == alive
    assert np.array_equal(fetch_all(t5, 8), rows5) and np.array_equal(fetch_all(t5, 8, edges=True), edges5)
    assert not alive or "k_value_gather" in names, names


# ---- tables without rows -------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("hops", HOPS)
def test_every_operator_on_an_empty_deep_table(gg, world, hops):
    """the dying shape has no walk of 4 hops or more: every operator answers zero rows and zeroed stats, and its result is
    fetched and closed like any other"""
    w = world("dying", hops)
    values = id_values(w.vid, "seven")
    for tiles in TILES:
        gg.max_grid_tiles(tiles)
        for table, rows, _ in w.tables:
            assert rows.shape == (0, hops + 1) and table.rows(hops) == 0
            for mode in F.MODES:
                st, res = gg.filter_edge(table, hops, w.csr, 0, hops, mode)
                assert st == {"rows_in": 0, "rows_out": 0, "matches": 0} and res.rows(hops) == 0
                assert fetch_all(res, hops).shape == (0, hops + 1)
                res.close()
            if hops < 8:
                for edges in (False, True):
                    st, res = gg.extend_edge(table, hops, w.ext_csr, hops, edges=edges)
                    assert st == {"rows_in": 0, "rows_out": 0, "rows_matched": 0} and res.rows(hops + 1) == 0
                    assert fetch_all(res, hops + 1).shape == (0, hops + 2)
                    res.close()
            agg = gg.group_by(table, hops, hops, w.csr, 0, None, values)
            assert agg.stats == {"rows_in": 0, "rows_grouped": 0, "groups": 0, "route": 0} and agg.rows(hops) == 0
            assert len(agg.fetch(hops)[0]) == 0
            agg.close()
            st, res = gg.filter_value(table, hops, hops, w.csr, values)
            assert st == {"rows_in": 0, "rows_valued": 0, "rows_out": 0} and fetch_all(res, hops).shape == (0, hops + 1)
            res.close()
            st, res = gg.top_rows(table, hops, hops, w.csr, values, 5, tie_col=0)
            assert not any(st.values()) and res.rows(hops) == 0 and fetch_all(res, hops).shape == (0, hops + 1)
            res.close()
