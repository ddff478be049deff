"""GG.filter_value (gg_result_filter_value) and GG.top_rows (gg_result_top_rows) against the numpy restatement
(tests/value_rows_ref.py): stats, rows in input or rank order and edge columns, for every value column, both modes, the
bounds' edge cases, valid bitmaps, both directions and every kind of tie column, under the default and the forced selection
and sort routes, on split launches, on row counts around the wavefront, the workgroup and the select tile, on edge-case ids
under every id dictionary, chained with the other device operators, on degenerate shapes and through every error.

The tables are tests/test_gpu_extend.py's: the walks of its source list over triangles_ref.hard_graph(), extended over
extend_ref.ext_table.  Some next ids of that table are person ids by design, so with the walk CSR as value_csr a few
message cells do have a value; the CSR of which truly no cell is a vertex is STRANGERS below.  The stranger key of
ext_table is a vertex of the extension's CSR that no row holds: it carries INT64_MAX / INT64_MIN, so a lookup that went
astray would put it first.

The 2^32-row refusals (materialising 2^32 rows, a top over a table of 2^32 rows) cannot be reached at test size; they were
checked by reading csrc/gg_value.hip only."""
import ctypes as C

import numpy as np
import pytest

from duckdb_pgq_amd import GGError
from duckdb_pgq_amd.gg import ValueFilterStats, ValueTopStats
from tests import edge_filter_ref as F
from tests import edge_ids as E
from tests import extend_ref as X
from tests import group_by_ref as G
from tests import khop_aggregate_ref as K
from tests import khop_aggregate_top_ref as TOP
from tests import triangles_ref as T
from tests import value_rows_ref as R
from tests.test_gpu_extend import build, build_ext, fetch_all

pytestmark = pytest.mark.gpu

GG_ERR_INVALID_ARG, GG_ERR_STATE = -1, -6
LO, HI = R.I64_MIN, R.I64_MAX
FETCH_BELOW = 200_000  # outputs of fewer rows are fetched and compared in order; larger ones by count and digest
LDS_ROWS, DEFAULT_FLOOR, TILE = 1024, 65_536, 4096  # GG_CHUNK_ROWS, TOP_CANDIDATE_FLOOR, TOP_TILE of csrc/gg_top.h
KNOBS = [(0, 0), (1, 256), (2, 256)]  # (sort_route, candidate_floor) of gg_debug_value_top
STRANGERS = np.array([-7, -8, -9], np.int64)  # vertices of a CSR that no cell of any table holds


def id_values(ids, kind: str, seed: int = 0x5EED) -> np.ndarray:
    """one int64 per id, a function of the id alone.  full: random over the whole signed range; seven: 7 distinct values"""
    ids = np.asarray(ids, np.int64)
    h = ids.view(np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(seed)
    h ^= h >> np.uint64(29)
    h *= np.uint64(0xBF58476D1CE4E5B9)
    h ^= h >> np.uint64(32)
    if kind == "seven":
        return (h % np.uint64(7)).astype(np.int64) - 3
    return h.view(np.int64).copy()


@pytest.fixture(scope="module")
def hard():
    """test_gpu_extend.py's graph, joined table and source list; the extended tables (CPU, from the restatement of the
    extension) and the value columns, keyed by id.  Computed once, never changed."""
    vid, src, dst = T.hard_graph()
    g = T.TriangleGraph(vid, src, dst)
    es, ed, er, info = X.ext_table(g)
    light = int(es[(es != info["hub"]) & np.isin(es, g.vid)][0])
    S = np.array([info["hub"], info["z"], info["hub"], light, int(g.vid[3])], np.int64)
    walks = {h: g.vid[F.walks(g, S, h)] for h in (1, 2)}
    ext = {"big": (2, 0), "mid": (2, 2), "small": (1, 1)}  # name -> (hops of the walk table, from_col)
    rows = {name: X.extend_rows(walks[h], es, ed, er, fc)[0] for name, (h, fc) in ext.items()}
    assert [rows[k].shape[0] for k in ("big", "mid", "small")] == [172_475, 25_146, 10]
    msgs, per_msg = np.unique(rows["big"][:, 3], return_counts=True)
    assert msgs.size == 2937 and per_msg.max() == 839
    assert rows["big"].shape[0] > DEFAULT_FLOOR and (rows["big"].shape[0] + TILE - 1) // TILE == 43
    universe = np.unique(np.concatenate([vid, es, ed]))
    full, seven = id_values(universe, "full"), id_values(universe, "seven")
    # the extremes on four messages of every table, and on the stranger key that no table holds
    planted = set()
    for name in ("small", "mid", "big"):
        fresh = [m for m in np.unique(rows[name][:, -1]).tolist() if m not in planted][:4]
        assert len(fresh) == 4
        for m, x in zip(fresh, (LO, -1, 0, HI)):
            full[np.searchsorted(universe, m)] = x
        planted.update(fresh)
    full[np.searchsorted(universe, info["stranger"])] = HI
    seven[np.searchsorted(universe, info["stranger"])] = LO
    assert np.unique(seven[np.isin(universe, rows["big"][:, 3])]).size == 7
    rng = np.random.RandomState(0x7A11D)
    some_valid = rng.rand(universe.size) >= 1 / 8
    for a in (es, ed, er, full, seven, some_valid, universe, *walks.values(), *rows.values()):
        a.setflags(write=False)
    return {"vid": vid, "src": src, "dst": dst, "g": g, "ext": (es, ed, er, info), "S": S, "walks": walks, "shape": ext,
            "rows": rows, "universe": universe, "full": full, "seven": seven, "some_valid": some_valid}


def column(hard, ids, kind):
    """the value column `kind` in the order of `ids` (a vertex table)"""
    return hard[kind][np.searchsorted(hard["universe"], ids)]


def valid_words(hard, ids, which):
    if which == "all":
        return None
    if which == "none":
        return R.pack_valid(np.zeros(len(ids), bool))
    return R.pack_valid(hard["some_valid"][np.searchsorted(hard["universe"], ids)])


class World:
    """the device objects of one test: the walk CSR, the extension's CSR and one extended table with edge columns"""

    def __init__(self, gg, hard, name):
        es, ed, er, _ = hard["ext"]
        self.gg, self.hops = gg, hard["shape"][name][0] + 1
        self.ext_csr, _ = build_ext(gg, hard["vid"], es, ed, er)
        self.ext_ids = self.ext_csr.export()[3]
        self.csr = build(gg, hard["vid"], hard["src"], hard["dst"])
        h, fc = hard["shape"][name]
        self.walk = gg.expand_khop_edges(self.csr, h, hard["S"])
        assert np.array_equal(fetch_all(self.walk, h), hard["walks"][h])
        st, self.table = gg.extend_edge(self.walk, h, self.ext_csr, fc, edges=True)
        self.rows = hard["rows"][name]
        assert st["rows_out"] == self.rows.shape[0]
        self.edges = fetch_all(self.table, self.hops, edges=True)
        assert (self.edges[:, :h] != -1).all()
        self.opened = [self.table, self.walk, self.csr, self.ext_csr]

    def own(self, obj):
        self.opened.insert(0, obj)
        return obj

    def close(self):
        for o in self.opened:
            o.close()


def check_filter(gg, res, hops, rows, edges, col, csr, ids, values, valid, lo, hi, mode, digest_index=None):
    """one predicate against the restatement, count-only and materialised; returns the stats"""
    want_rows, want_edges, want = R.filter_rows(rows, edges, col, ids, values, valid, lo, hi, mode)
    only = gg.filter_value(res, hops, col, csr, values, valid, lo, hi, mode, materialise=False)
    st, out = gg.filter_value(res, hops, col, csr, values, valid, lo, hi, mode)
    print((hops, col, mode, lo, hi), "device", st, "restatement", want)
    try:
        assert st == want and only == want
        assert out.rows(hops) == want["rows_out"]
        if want["rows_out"] < FETCH_BELOW:
            assert np.array_equal(fetch_all(out, hops), want_rows)
            if edges is not None and hops:
                assert np.array_equal(fetch_all(out, hops, edges=True), want_edges)
        elif digest_index is not None:
            assert out.digest(csr, hops) == (want["rows_out"], F.digest_dense_rows(X.dense_rows(digest_index, want_rows)))
    finally:
        out.close()
    return st


def bounds_of(x_valued):
    """name -> (lo, hi) for the values some rows have: selective, everything, nothing, lo > hi, lo == hi, the extremes"""
    s = np.sort(np.asarray(x_valued, np.int64))
    absent = int(s[s.size // 2]) + 1
    while absent in set(s.tolist()):
        absent += 1
    return {"selective": (int(s[s.size // 4]), int(s[s.size // 2])), "everything": (LO, HI), "nothing": (absent, absent),
            "lo_above_hi": (int(s[s.size // 2]), int(s[s.size // 4]) - 1), "one_value": (int(s[s.size // 3]),) * 2,
            "min_only": (LO, LO), "max_only": (HI, HI), "below_max": (LO, HI - 1), "above_min": (LO + 1, HI)}


@pytest.mark.parametrize("name", ["big", "mid", "small"])
def test_filter_every_value_column_mode_and_bound(gg, hard, name):
    w = World(gg, hard, name)
    try:
        hops, rows, edges = w.hops, w.rows, w.edges
        person_vals, msg_vals = column(hard, hard["vid"], "full"), column(hard, w.ext_ids, "full")
        seen = {}
        for col in range(hops + 1):
            # a person column over the walk CSR, the message column over the extension's; every column over the latter too
            for csr, ids, values in ((w.csr, hard["vid"], person_vals), (w.ext_csr, w.ext_ids, msg_vals)):
                if col == hops and csr is w.csr and name == "big":
                    continue  # (covered by test_value_csr_that_holds_no_cell_or_few)
                has, x = R.row_values(rows, col, ids, values)
                for bname, (lo, hi) in bounds_of(x[has]).items():
                    for mode in ("in", "not_in"):
                        if name == "big" and bname not in ("selective", "lo_above_hi") and csr is w.csr:
                            continue  # (the large table: every bound on the message column, two on the others)
                        st = check_filter(gg, w.table, hops, rows, edges, col, csr, ids, values, None, lo, hi, mode)
                        seen[(col, bname, mode)] = st
        # the facts the cases rest on
        assert any(0 < st["rows_out"] < st["rows_in"] for st in seen.values())
        assert seen[(hops, "everything", "in")]["rows_out"] == rows.shape[0] == seen[(hops, "lo_above_hi", "not_in")]["rows_out"]
        assert seen[(hops, "nothing", "in")]["rows_out"] == 0 == seen[(hops, "lo_above_hi", "in")]["rows_out"]
        assert seen[(hops, "min_only", "in")]["rows_out"] > 0 and seen[(hops, "max_only", "in")]["rows_out"] > 0
        assert 0 < seen[(hops, "one_value", "not_in")]["rows_out"] < rows.shape[0]
    finally:
        w.close()


@pytest.mark.parametrize("which", ["some", "none"])
def test_filter_with_a_valid_bitmap(gg, hard, which):
    w = World(gg, hard, "mid")
    try:
        for kind in ("full", "seven"):
            values, valid = column(hard, w.ext_ids, kind), valid_words(hard, w.ext_ids, which)
            has, x = R.row_values(w.rows, w.hops, w.ext_ids, values, valid)
            assert (which == "none") == (not has.any()) and not has.all()
            for col in (0, w.hops):
                for lo, hi in ((LO, HI), (-1, 1), (1, -1), (0, 0)):
                    for mode in ("in", "not_in"):
                        st = check_filter(gg, w.table, w.hops, w.rows, w.edges, col, w.ext_csr, w.ext_ids, values, valid, lo, hi, mode)
                        assert st["rows_valued"] < st["rows_in"]
    finally:
        w.close()


def test_value_csr_that_holds_no_cell_or_few(gg, hard):
    w = World(gg, hard, "big")
    try:
        none = w.own(build(gg, STRANGERS, STRANGERS[:2], STRANGERS[1:]))
        for csr, ids in ((none, STRANGERS), (w.csr, hard["vid"])):
            values = id_values(ids, "full")
            for mode, (lo, hi) in (("in", (LO, HI)), ("not_in", (1, 0))):
                st = check_filter(gg, w.table, w.hops, w.rows, w.edges, w.hops, csr, ids, values, None, lo, hi, mode)
                assert st["rows_out"] == st["rows_valued"] and (st["rows_valued"] == 0) == (csr is none)
                assert st["rows_valued"] < st["rows_in"] // 2
                ts, top = gg.top_rows(w.table, w.hops, w.hops, csr, values, 20, None, lo, hi, mode, True, 0)
                want = R.top_rows(w.rows, w.edges, w.hops, ids, values, None, lo, hi, mode, True, 0, 20)
                assert ts["candidates"] == want[2]["candidates"] and np.array_equal(fetch_all(top, w.hops), want[0])
                top.close()
    finally:
        w.close()


def test_filter_rows_are_identical_on_split_launches_and_large_outputs_by_digest(gg, hard):
    w = World(gg, hard, "big")
    try:
        values = column(hard, w.ext_ids, "full")
        index = {int(v): i for i, v in enumerate(w.ext_ids.tolist())}
        s = np.sort(R.row_values(w.rows, w.hops, w.ext_ids, values)[1])
        args = (gg, w.table, w.hops, w.rows, w.edges, w.hops, w.ext_csr, w.ext_ids, values, None)
        first = check_filter(*args, int(s[s.size // 4]), int(s[s.size // 2]), "in")
        gg.max_grid_tiles(3)  # three workgroups a launch: the probe strides, the write pass takes 225 launches
        assert check_filter(*args, int(s[s.size // 4]), int(s[s.size // 2]), "in") == first
        assert 256 * 3 < first["rows_out"] < first["rows_in"]
        gg.debug_reset()
        global FETCH_BELOW
        keep, FETCH_BELOW = FETCH_BELOW, 1000  # the route of outputs too large to fetch: count and digest
        try:
            check_filter(*args, int(s[s.size // 4]), int(s[s.size // 2]), "not_in", digest_index=index)
        finally:
            FETCH_BELOW = keep
    finally:
        w.close()


# ---- the top
def expected_route(knob_route, n, rows_in, rows_out):
    bound = min(n, rows_in)
    return 0 if rows_out < 2 else (1 if knob_route != 2 and bound <= LDS_ROWS else 2)


def check_top(gg, res, hops, rows, edges, col, csr, ids, values, valid, lo, hi, mode, desc, tie, ns, knobs=KNOBS):
    """every n under every knob against one run of the restatement (its answer for n is the first n rows of its answer
    for every candidate); returns the number of candidates"""
    all_rows, all_edges, all_st = R.top_rows(rows, edges, col, ids, values, valid, lo, hi, mode, desc, tie, 1 << 62)
    cand = all_st["candidates"]
    key_bytes = 8 + (8 if tie is not None else 0) + (max(1, (rows.shape[0] - 1).bit_length()) + 7) // 8
    for n in ns(cand):
        m = min(n, cand)
        for route, floor in knobs:
            gg.debug_value_top(route, floor)
            st, out = gg.top_rows(res, hops, col, csr, values, n, valid, lo, hi, mode, desc, tie)
            try:
                print((col, mode, desc, tie, n, route, floor), st)
                assert {k: st[k] for k in all_st} == dict(all_st, rows_out=m)
                assert out.rows(hops) == m
                assert np.array_equal(fetch_all(out, hops), all_rows[:m])
                if edges is not None:
                    assert np.array_equal(fetch_all(out, hops, edges=True), all_edges[:m])
                assert st["sort_route"] == expected_route(route, n, rows.shape[0], m)
                if m == 0:
                    assert st["select_passes"] == 0
                elif n >= cand:
                    assert st["select_passes"] == 1  # every candidate is in: decided by the first pass
                else:
                    assert 1 <= st["select_passes"] <= key_bytes
            finally:
                out.close()
    gg.debug_value_top(0, 0)
    return cand


def all_ns(cand):
    return sorted({0, 1, 20, 1024, 1025, max(cand - 1, 0), cand, cand + 5, 1 << 40})


def few_large_ns(cand):  # the 172 475-row table: one answer of every candidate per knob
    return [0, 1, 20, 1024, 1025, cand - 1, 1 << 40]


def tie_straddles(rows, x, has, tie, n, desc):
    """the n-th and the (n + 1)-th row of the order share their value (tie None) or their value and tie id"""
    cand = np.nonzero(has)[0]
    t = rows[cand, tie] if tie is not None else np.zeros(cand.size, np.int64)
    o = np.lexsort((cand, t, R.order_key(x[cand], desc)))
    a, b = cand[o[n - 1]], cand[o[n]]
    return x[a] == x[b] and (tie is None or rows[a, tie] == rows[b, tie])


@pytest.mark.parametrize("desc", [True, False])
@pytest.mark.parametrize("tie", [None, 1, "last"])
def test_top_of_the_seven_valued_column_on_the_mid_table(gg, hard, desc, tie):
    w = World(gg, hard, "mid")
    try:
        tie = w.hops if tie == "last" else tie
        values = column(hard, w.ext_ids, "seven")
        has, x = R.row_values(w.rows, w.hops, w.ext_ids, values)
        assert has.all() and np.unique(x).size == 7
        # ties by row number straddle these n (7 values over 25 146 rows; the same message many times)
        for n in (20, 1024, 1025):
            assert tie_straddles(w.rows, x, has, tie, n, desc)
        cand = check_top(gg, w.table, w.hops, w.rows, w.edges, w.hops, w.ext_csr, w.ext_ids, values, None, LO, HI, "in", desc, tie, all_ns)
        assert cand == w.rows.shape[0] > LDS_ROWS
    finally:
        w.close()


@pytest.mark.parametrize("desc", [True, False])
def test_top_of_the_large_table_above_the_default_floor(gg, hard, desc):
    w = World(gg, hard, "big")
    try:
        for kind, tie in (("seven", w.hops), ("full", None), ("seven", 1)):
            values = column(hard, w.ext_ids, kind)
            cand = check_top(gg, w.table, w.hops, w.rows, w.edges, w.hops, w.ext_csr, w.ext_ids, values, None, LO, HI, "in", desc, tie,
                             few_large_ns, knobs=KNOBS if kind == "seven" and tie == w.hops else KNOBS[:1])
            assert cand == w.rows.shape[0] > DEFAULT_FLOOR
    finally:
        w.close()


@pytest.mark.parametrize("mode", ["in", "not_in"])
def test_top_with_a_predicate_and_a_valid_bitmap(gg, hard, mode):
    w = World(gg, hard, "mid")
    try:
        values, valid = column(hard, w.ext_ids, "full"), valid_words(hard, w.ext_ids, "some")
        has, x = R.row_values(w.rows, w.hops, w.ext_ids, values, valid)
        s = np.sort(x[has])
        few = (int(s[0]), int(s[600])) if mode == "in" else (int(s[600]) + 1, HI)   # at most 1 023 candidates ...
        many = (int(s[0]), int(s[5000])) if mode == "in" else (int(s[5000]) + 1, HI)  # ... and 1 025 or more
        counts = []
        for lo, hi in (few, many):
            for desc, tie in ((True, w.hops), (False, None), (True, 0)):
                counts.append(check_top(gg, w.table, w.hops, w.rows, w.edges, w.hops, w.ext_csr, w.ext_ids, values, valid, lo, hi, mode,
                                        desc, tie, all_ns))
        assert 0 < counts[0] < LDS_ROWS and LDS_ROWS + 1 <= counts[-1] < has.sum()
        # a person's value over the walk CSR, ordered by the message id
        pv = column(hard, hard["vid"], "seven")
        check_top(gg, w.table, w.hops, w.rows, w.edges, 1, w.csr, hard["vid"], pv, None, -1, 1, mode, True, w.hops, all_ns, knobs=KNOBS[:2])
    finally:
        w.close()


@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097])
def test_row_counts_around_the_wavefront_the_workgroup_and_the_select_tile(gg, n_rows):
    """a star: the 1-hop table of the centre has n rows; the value is per leaf"""
    n = n_rows
    vid = np.arange(100, 100 + n + 1, dtype=np.int64)
    csr = build(gg, vid, np.full(n, vid[0], np.int64), vid[1:])
    table = gg.expand_khop_edges(csr, 1, vid[:1])
    try:
        rows, edges = fetch_all(table, 1), fetch_all(table, 1, edges=True)
        assert rows.shape[0] == n
        values = id_values(vid, "seven")
        valid = R.pack_valid(np.arange(vid.size) % 5 != 2)
        for lo, hi in ((LO, HI), (-1, 2), (0, 0)):
            for mode in ("in", "not_in"):
                check_filter(gg, table, 1, rows, edges, 1, csr, vid, values, valid, lo, hi, mode)
        for desc in (True, False):
            for tie in (None, 1):
                check_top(gg, table, 1, rows, edges, 1, csr, vid, values, valid, -2, 3, "in", desc, tie,
                          lambda cand: sorted({0, 1, cand // 2, max(cand - 1, 0), cand, n + 1}))
    finally:
        table.close()
        csr.close()


@pytest.mark.parametrize("kind", E.PLACEMENTS)
def test_edge_case_ids_as_cells_and_as_tie_ids_under_every_dictionary(gg, kind):
    eg = E.edge_graph(kind)
    ref = E.references(eg)
    rows = ref["table"]
    csr = build(gg, eg.vid, eg.src, eg.dst)
    table = gg.expand_khop_result(csr, E.TABLE_HOPS, ref["table_sources"])
    try:
        assert np.array_equal(fetch_all(table, E.TABLE_HOPS), rows)
        assert all(np.isin(eg.named, rows[:, c]).any() for c in (0, 2))  # the columns hold the edge-case ids
        full, seven = E.weights_of(eg), id_values(eg.vid, "seven")
        for col in range(E.TABLE_HOPS + 1):
            for lo, hi, mode in ((LO, HI, "in"), (-1, -1, "not_in"), (LO + 1, HI - 1, "not_in"), (0, HI, "in")):
                check_filter(gg, table, E.TABLE_HOPS, rows, None, col, csr, eg.vid, full, None, lo, hi, mode)
        for desc in (True, False):
            for tie in (0, 2):  # signed tie order over INT64_MIN, -1, 2^32 - 1 and INT64_MAX
                check_top(gg, table, E.TABLE_HOPS, rows, None, 1, csr, eg.vid, seven, None, LO, HI, "in", desc, tie,
                          lambda cand: sorted({20, cand // 3, cand}))
            check_top(gg, table, E.TABLE_HOPS, rows, None, 2, csr, eg.vid, full, None, LO, HI, "in", desc, 0,
                      lambda cand: [5, cand], knobs=KNOBS[:1])
    finally:
        table.close()
        csr.close()


# ---- chains
def test_chain_filter_group_and_aggregate_top(gg, hard):
    """expand -> extend -> filter_value -> group_by -> khop_aggregate_top: count(*) per message of a value range, ordered"""
    w = World(gg, hard, "mid")
    try:
        values = column(hard, w.ext_ids, "full")
        s = np.sort(values)
        lo, hi = int(s[s.size // 5]), int(s[s.size // 2])
        kept_rows, _, want_st = R.filter_rows(w.rows, None, w.hops, w.ext_ids, values, None, lo, hi, "in")
        st, kept = gg.filter_value(w.table, w.hops, w.hops, w.ext_csr, values, None, lo, hi)
        w.own(kept)
        assert st == want_st and 0 < st["rows_out"] < st["rows_in"]
        level, _ = G.group_by(kept_rows, w.hops, w.ext_ids)
        agg = w.own(gg.group_by(kept, w.hops, w.hops, w.ext_csr))
        assert K.same(agg.fetch(w.hops), level)
        for n in (1, 10, len(level[0])):
            top = gg.khop_aggregate_top(agg, w.hops, "walks", True, n)
            assert K.same(top.fetch(w.hops), TOP.top(level, n, "walks", True))
            top.close()
    finally:
        w.close()


def test_chain_top_rows_extended_again_and_filter_then_top(gg, hard):
    w = World(gg, hard, "mid")
    try:
        es, ed, er, _ = hard["ext"]
        ts, td, tr = X.tag_table(ed)
        gg.staging_clear()
        gg.append_edges(ts, td, tr)
        gg.vertices_from_edges()
        tag_csr = w.own(gg.build_csr())
        values = column(hard, w.ext_ids, "seven")
        top_rows, top_edges, want = R.top_rows(w.rows, w.edges, w.hops, w.ext_ids, values, None, -2, 2, "in", True, w.hops, 300)
        st, top = gg.top_rows(w.table, w.hops, w.hops, w.ext_csr, values, 300, None, -2, 2, "in", True, w.hops)
        w.own(top)
        assert np.array_equal(fetch_all(top, w.hops), top_rows) and np.array_equal(fetch_all(top, w.hops, edges=True), top_edges)
        # the top is an ordinary walk table: its messages' tags
        both, rid, want_ext = X.extend_rows(np.concatenate([top_rows, top_edges], axis=1), ts, td, tr, w.hops)
        st2, longer = gg.extend_edge(top, w.hops, tag_csr, w.hops, edges=True)
        w.own(longer)
        assert st2 == want_ext and want_ext["rows_out"] > 0
        ncol = w.hops + 1
        assert np.array_equal(fetch_all(longer, ncol), both[:, list(range(ncol)) + [both.shape[1] - 1]])
        assert np.array_equal(fetch_all(longer, ncol, edges=True), np.concatenate([both[:, ncol:2 * ncol - 1], rid.reshape(-1, 1)], axis=1))
        # a filter followed by a top of everything equals the top with the predicate; so does every other reader's view
        _, kept = gg.filter_value(w.table, w.hops, w.hops, w.ext_csr, values, None, -2, 2)
        w.own(kept)
        st3, again = gg.top_rows(kept, w.hops, w.hops, w.ext_csr, values, 300, descending=True, tie_col=w.hops)
        w.own(again)
        assert st3["rows_in"] == st3["candidates"] == st["candidates"]
        assert np.array_equal(fetch_all(again, w.hops), top_rows) and np.array_equal(fetch_all(again, w.hops, edges=True), top_edges)
        assert top.digest(w.ext_csr, w.hops) == again.digest(w.ext_csr, w.hops)
        fst, f2 = gg.filter_value(top, w.hops, 0, w.csr, column(hard, hard["vid"], "seven"), None, 0, 3)  # this call again
        w.own(f2)
        sst, semi = gg.filter_edge(top, w.hops, w.csr, 1, 0, "semi")  # and the edge filter
        w.own(semi)
        assert fst["rows_in"] == sst["rows_in"] == 300
    finally:
        w.close()


def test_degenerate_shapes(gg):
    vid = np.array([10, 20, 30], np.int64)
    csr = build(gg, vid, np.array([10, 20], np.int64), np.array([20, 10], np.int64))
    gg.staging_clear()
    no_vertices = gg.build_csr()
    values = np.array([5, 6, 7], np.int64)
    none = np.empty(0, np.int64)
    empty = gg.expand_khop_result(csr, 2, none)  # an empty input table
    two = gg.expand_khop_edges(csr, 1, None)     # (10, 20), (20, 10)
    try:
        assert no_vertices.V == 0
        cases = [(empty, 2, csr, values, LO, HI, 5, 0, 0),          # an empty table
                 (two, 1, no_vertices, none, LO, HI, 5, 2, 0),      # a value_csr without vertices
                 (two, 1, csr, values, LO, HI, 0, 2, 2),            # n == 0
                 (two, 1, csr, values, 100, 200, 5, 2, 2)]          # no candidate
        for res, hops, graph, vals, lo, hi, n, rows_in, valued in cases:
            st, out = gg.top_rows(res, hops, 0, graph, vals, n, None, lo, hi)
            assert (st["rows_in"], st["rows_valued"], st["rows_out"], st["select_passes"], st["sort_route"]) == (rows_in, valued, 0, 0, 0)
            assert out.handle and out.rows(hops) == 0 and fetch_all(out, hops).shape == (0, hops + 1)
            st2, again = gg.filter_value(out, hops, 0, csr, values)  # an empty result is an input like any other
            assert st2 == {"rows_in": 0, "rows_valued": 0, "rows_out": 0} and again.rows(hops) == 0
            again.close()
            out.close()
            if n:
                fs, kept = gg.filter_value(res, hops, 0, graph, vals, None, lo, hi)
                assert fs == {"rows_in": rows_in, "rows_valued": valued, "rows_out": 0} and kept.rows(hops) == 0
                assert fetch_all(kept, hops).shape == (0, hops + 1)
                kept.close()
        st, out = gg.top_rows(two, 1, 1, csr, values, 5, descending=False, tie_col=0)  # and a table of two rows
        assert fetch_all(out, 1).tolist() == [[20, 10], [10, 20]] and st["sort_route"] == 1 and st["candidates"] == 2
        assert np.array_equal(fetch_all(out, 1, edges=True), fetch_all(two, 1, edges=True)[::-1])
        out.close()
    finally:
        empty.close()
        two.close()
        no_vertices.close()
        csr.close()


def test_errors_leave_the_context_usable(gg, hard):
    from tests import test_gpu_result_kinds as RK

    vid, src, dst, S = hard["vid"], hard["src"], hard["dst"], hard["S"]
    gg.staging_clear()
    gg.append_vertices(vid)
    gg.append_edges(src, dst)
    shard = gg.build_csr_shard(0, 2)
    csr = gg.build_csr()
    table = gg.expand_khop_result(csr, 2, S)
    other = type(gg)(0)
    other.append_vertices(vid[:4])
    other.append_edges(vid[:2], vid[2:4])
    foreign = other.build_csr()
    foreign_table = other.expand_khop_result(foreign, 1, None)
    values = column(hard, vid, "seven")
    vp = values.ctypes.data_as(C.POINTER(C.c_int64))
    rows = hard["walks"][2]
    want = R.filter_rows(rows, None, 1, vid, values, None, -1, 1, "in")[2]
    want_top = R.top_rows(rows, None, 1, vid, values, None, -1, 1, "in", True, 2, 7)[0]

    def filt(res, hops, col, graph, vals=vp, mode=0, materialise=1, out=True, ctx=None):
        st, o = ValueFilterStats(), C.c_void_p(1)
        rc = gg.lib.gg_result_filter_value(ctx or gg.ctx, res, hops, col, graph, vals, None, -1, 1, mode, materialise, C.byref(st),
                                           C.byref(o) if out else None)
        assert rc != 0 and (not out or not o.value)
        return rc

    def top(res, hops, col, graph, vals=vp, mode=0, tie=-1, out=True, ctx=None):
        st, o = ValueTopStats(), C.c_void_p(1)
        rc = gg.lib.gg_result_top_rows(ctx or gg.ctx, res, hops, col, graph, vals, None, -1, 1, mode, 1, tie, 7, C.byref(st),
                                       C.byref(o) if out else None)
        assert rc != 0 and (not out or not o.value)
        return rc

    kinds_csr = build(gg, RK.VID, RK.SRC, RK.DST, RK.ROWID)
    kinds = {}
    try:
        RK.make_results(gg, kinds_csr, kinds)
        kv = np.zeros(RK.VID.size, np.int64).ctypes.data_as(C.POINTER(C.c_int64))
        bad = []
        for f in (filt, top):
            bad += [
                (f(None, 2, 1, csr.handle), GG_ERR_INVALID_ARG),
                (f(table.handle, 2, 1, None), GG_ERR_INVALID_ARG),
                (f(table.handle, 2, 1, csr.handle, ctx=other.ctx), GG_ERR_INVALID_ARG),
                (f(table.handle, 2, 1, foreign.handle), GG_ERR_INVALID_ARG),          # a CSR of another context
                (f(foreign_table.handle, 1, 1, csr.handle), GG_ERR_INVALID_ARG),      # a result of another context
                (f(table.handle, 3, 1, csr.handle), GG_ERR_INVALID_ARG),              # hops outside the result's levels
                (f(table.handle, 1, 1, csr.handle), GG_ERR_INVALID_ARG),
                (f(table.handle, 2, 3, csr.handle), GG_ERR_INVALID_ARG),              # value column hops + 1
                (f(table.handle, 2, -1, csr.handle), GG_ERR_INVALID_ARG),
                (f(table.handle, 2, 1, csr.handle, mode=2), GG_ERR_INVALID_ARG),
                (f(table.handle, 2, 1, csr.handle, mode=-1), GG_ERR_INVALID_ARG),
                (f(table.handle, 2, 1, csr.handle, vals=None), GG_ERR_INVALID_ARG),   # NULL values
                (f(table.handle, 2, 1, csr.handle, out=False), GG_ERR_INVALID_ARG),   # materialise / top without out_result
                (f(table.handle, 2, 1, shard.handle), GG_ERR_STATE),                  # a shard CSR
            ]
            for name in ("closure", "reach", "levels", "paths", "agg", "top", "pairs", "comps", "all_paths"):
                bad.append((f(kinds[name], RK.HOPS, 0, kinds_csr.handle, vals=kv), GG_ERR_STATE))  # no fixed-length table
        bad += [(top(table.handle, 2, 1, csr.handle, tie=3), GG_ERR_INVALID_ARG),      # tie column hops + 1
                (top(table.handle, 2, 1, csr.handle, tie=-2), GG_ERR_INVALID_ARG)]
        for i, (rc, code) in enumerate(bad):
            assert rc == code, (i, rc, code)
            assert gg.filter_value(table, 2, 1, csr, values, None, -1, 1, materialise=False) == want  # a correct call still works
        _, out = gg.top_rows(table, 2, 1, csr, values, 7, None, -1, 1, "in", True, 2)
        assert np.array_equal(fetch_all(out, 2), want_top)
        out.close()
        # the walk tables of every origin are answered, a triangle table without its triangle edge columns
        for name in ("walk", "walk_edges", "tri", "tri_edges"):
            st, out = gg.filter_value(_Handle(gg, kinds[name]), RK.HOPS, 0, kinds_csr, np.zeros(RK.VID.size, np.int64))
            assert st["rows_out"] == st["rows_in"] > 0
            if name == "walk_edges":
                assert fetch_all(out, RK.HOPS, edges=True).shape == (st["rows_in"], RK.HOPS)
            else:
                with pytest.raises(GGError):
                    out.fetch_edges(RK.HOPS, 0)
            bufs = (C.POINTER(C.c_int64) * 3)(*[np.zeros(8, np.int64).ctypes.data_as(C.POINTER(C.c_int64)) for _ in range(3)])
            assert gg.lib.gg_triangles_fetch_edges(out.handle, 0, 8, bufs, C.byref(C.c_uint32())) == GG_ERR_STATE
            out.close()
        st = ValueFilterStats()  # count mode takes a NULL out_result
        assert gg.lib.gg_result_filter_value(gg.ctx, table.handle, 2, 1, csr.handle, vp, None, -1, 1, 0, 0, C.byref(st), None) == 0
        assert int(st.rows_out) == want["rows_out"]
        with pytest.raises(ValueError):
            gg.filter_value(table, 2, 1, csr, values[:-1])
        with pytest.raises(ValueError):
            gg.top_rows(table, 2, 1, csr, values, 5, valid=np.zeros(1, np.uint64))
    finally:
        for res in kinds.values():
            gg.lib.gg_result_destroy(res)
        kinds_csr.close()
        foreign_table.close()
        foreign.close()
        other.close()
        table.close()
        shard.close()
        csr.close()


class _Handle:
    """a result owned elsewhere, for the calls that take a KhopResult"""

    def __init__(self, gg, handle):
        self.gg, self.handle = gg, handle
