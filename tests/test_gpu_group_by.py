"""GG.group_by (gg_result_group_by) against the numpy restatement (tests/group_by_ref.py): the stats and every row in order
with both halves of the total, for every key and weight column of plain, extended and chained tables, at the row counts
and run shapes a wavefront, a workgroup or a tile can get wrong, on both routes and under every knob (identical rows), on
both CSR builds, against gg_khop_aggregate (independent kernels), under gg_khop_aggregate_top, and through every error.
Tables of 2^32 rows or more cannot be reached at test size; that the kernels stride with 64-bit row numbers was checked
by reading csrc/gg_group.hip only."""
import ctypes as C

import numpy as np
import pytest

from duckdb_pgq_amd import GGError
from duckdb_pgq_amd.gg import GroupStats
from tests import edge_filter_ref as F
from tests import extend_ref as X
from tests import group_by_ref as R
from tests import khop_aggregate_ref as K
from tests import khop_aggregate_top_ref as TOP
from tests import triangles_ref as T
from tests.test_gpu_extend import build, build_ext, fetch_all

pytestmark = pytest.mark.gpu

GG_ERR_INVALID_ARG, GG_ERR_STATE = -1, -6
LDS_KEYS = {False: 6144, True: 2048}  # the default capacities of csrc/gg_group.hip: 48 KiB of 8-byte / 24-byte keys
TILE_ROWS = 1024                      # GRP_TILE_ROWS


@pytest.fixture(scope="module")
def hard():
    """tests/test_gpu_extend.py's fixture: the walk graph, the creator -> message table, the source list S (a duplicate,
    the hub) and its dense walk tables; plus person weights with the extremes and -2^63 on the hub"""
    vid, src, dst = T.hard_graph()
    g = T.TriangleGraph(vid, src, dst)
    es, ed, er, info = X.ext_table(g)
    light = int(es[(es != info["hub"]) & np.isin(es, g.vid)][0])
    S = np.array([info["hub"], info["z"], info["hub"], light, int(g.vid[3])], np.int64)
    walks = {h: F.walks(g, S, h) for h in (1, 2, 3)}
    w = R.hub_weights(g.vid, info["hub"])
    for a in (es, ed, er, w, *walks.values()):
        a.setflags(write=False)
    return vid, src, dst, g, (es, ed, er, info), S, walks, w


def route_for(V, weighted, route=0, lds_keys=0):
    cap = min(LDS_KEYS[weighted], lds_keys) if lds_keys else LDS_KEYS[weighted]
    return 1 if route != 2 and V <= cap else 2


def check(gg, res, hops, rows, kc, key_csr, key_ids, wc=None, wcsr=None, wids=None, weights=None, route=None):
    """one (key, weight) choice against the restatement; returns (stats, (ids, walks, totals))"""
    want, want_st = R.group_by(rows, kc, key_ids, wc, wids, weights)
    agg = gg.group_by(res, hops, kc, key_csr, wc, wcsr, weights)
    try:
        st = dict(agg.stats)
        got_route = st.pop("route")
        got = agg.fetch(hops)
        print((hops, kc, wc), "device", st, "route", got_route, "restatement", want_st)
        assert st == want_st
        assert agg.rows(hops) == want_st["groups"]
        assert K.same(got, want)
        if route is not None:
            assert got_route == (route if want_st["rows_in"] and key_csr.V else 0)
        only = gg.group_by(res, hops, kc, key_csr, wc, wcsr, weights, fetch=False)
        assert only.handle is None and only.stats == agg.stats
    finally:
        agg.close()
    return agg.stats, got


@pytest.mark.parametrize("hops", [1, 2])
def test_every_key_and_weight_column_of_plain_extended_and_chained_tables(gg, hard, hops):
    vid, src, dst, g, (es, ed, er, info), S, walks, w = hard
    ts, td, tr = X.tag_table(ed)
    ext_csr, _ = build_ext(gg, vid, es, ed, er)
    ext_ids = ext_csr.export()[3]
    gg.staging_clear()
    gg.append_edges(ts, td, tr)
    gg.vertices_from_edges()
    tag_csr = gg.build_csr()
    tag_ids = tag_csr.export()[3]
    csr = build(gg, vid, src, dst)
    table = gg.expand_khop_result(csr, hops, S)
    try:
        rows0 = g.vid[walks[hops]]
        for kc in range(hops + 1):  # plain walks: keys and weights are persons
            for wc in [None] + list(range(hops + 1)):
                check(gg, table, hops, rows0, kc, csr, g.vid, wc, None, None, None if wc is None else w)
        _, ext = gg.extend_edge(table, hops, ext_csr, hops)
        try:
            rows1 = X.extend_rows(rows0, es, ed, er, hops)[0]
            assert 0 < rows1.shape[0] and np.array_equal(fetch_all(ext, hops + 1), rows1)
            for kc in range(hops + 2):
                # the key's table holds every id of the rows; the weights are the persons': a message weighs 0
                for wc in [None] + list(range(hops + 2)):
                    check(gg, ext, hops + 1, rows1, kc, ext_csr, ext_ids, wc, None if wc is None else csr,
                          None if wc is None else g.vid, None if wc is None else w)
                # and by the persons alone: w is a person in one row of seven
                st, _ = check(gg, ext, hops + 1, rows1, kc, csr, g.vid)
                assert (st["rows_grouped"] < st["rows_in"]) == (kc == hops + 1)
            _, tags = gg.extend_edge(ext, hops + 1, tag_csr, hops + 1)  # knows -> message -> tag
            try:
                rows2 = X.extend_rows(rows1, ts, td, tr, hops + 1)[0]
                assert 0 < rows2.shape[0] and np.array_equal(fetch_all(tags, hops + 2), rows2)
                st, level = check(gg, tags, hops + 2, rows2, hops + 2, tag_csr, tag_ids)  # count(*) GROUP BY tag
                assert 1 < st["groups"] <= 50 and (level[0] >= 5_000_000).all()
                check(gg, tags, hops + 2, rows2, hops + 2, tag_csr, tag_ids, hops, csr, g.vid, w)  # sum(person weight) per tag
                check(gg, tags, hops + 2, rows2, 0, csr, g.vid, hops + 2, tag_csr, tag_ids,
                      np.arange(tag_ids.size, dtype=np.int64) - 7)  # sum(a tag weight) per start
            finally:
                tags.close()
        finally:
            ext.close()
    finally:
        table.close()
        csr.close()
        tag_csr.close()
        ext_csr.close()


def star(gg, runs):
    """a centre with len(runs) leaves, leaf i wired runs[i] times: the 1-hop table of the centre has sum(runs) rows, column
    0 one key for every row, column 1 runs of equal keys of those lengths.  (csr, table, id rows)"""
    runs = np.asarray(runs, np.int64)
    vid = 100 + 3 * np.arange(runs.size + 1, dtype=np.int64)
    dst = np.repeat(vid[1:], runs)
    csr = build(gg, vid, np.full(dst.size, vid[0], np.int64), dst)
    table = gg.expand_khop_result(csr, 1, vid[:1])
    rows = np.stack([np.full(dst.size, vid[0], np.int64), dst], axis=1)
    assert table.rows(1) == dst.size
    return csr, vid, table, rows


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, TILE_ROWS + 1])
def test_row_counts_around_the_wavefront_the_workgroup_and_the_tile(gg, n):
    """every row its own key (column 1) and one key for every row (column 0), with weights at the extremes, on both routes"""
    csr, vid, table, rows = star(gg, np.ones(max(n, 1), np.int64))
    if n == 0:
        table.close()
        table, rows = gg.expand_khop_result(csr, 1, np.empty(0, np.int64)), rows[:0]
    w = np.array([np.iinfo(np.int64).max, np.iinfo(np.int64).min, -np.iinfo(np.int64).max, 3], np.int64)[np.arange(vid.size) % 4]
    try:
        for route in (1, 2):
            gg.debug_group(route)
            for kc in (0, 1):
                st, level = check(gg, table, 1, rows, kc, csr, vid, route=route_for(csr.V, False, route))
                assert st["groups"] == (n if kc else min(n, 1)) and st["rows_grouped"] == n
                check(gg, table, 1, rows, kc, csr, vid, 1, None, None, w, route=route_for(csr.V, True, route))
    finally:
        table.close()
        csr.close()


def test_runs_of_equal_keys_cross_wavefronts_workgroups_and_tiles(gg):
    runs = [50, 30, 1, 1, 200, 3, 700, 2 * TILE_ROWS + 100, 1, 63, 64, 65, 5]
    edges = np.cumsum(runs)
    assert any(a // 64 != b // 64 for a, b in zip(edges - np.array(runs), edges - 1))        # a run over a wavefront's end
    assert any((b - 1) // 256 - a // 256 >= 1 for a, b in zip(edges - np.array(runs), edges))  # over a workgroup pass's end
    assert any((b - 1) // TILE_ROWS - a // TILE_ROWS >= 2 for a, b in zip(edges - np.array(runs), edges))  # over whole tiles
    csr, vid, table, rows = star(gg, runs)
    w = -(1 << 62) - np.arange(vid.size, dtype=np.int64)
    try:
        levels = []
        for route, tiles in ((1, 0), (2, 0), (1, 1), (2, 1), (0, 3)):
            gg.debug_group(route)
            gg.max_grid_tiles(tiles)
            levels.append(check(gg, table, 1, rows, 1, csr, vid, 1, None, None, w)[1])
            levels.append(check(gg, table, 1, rows, 1, csr, vid, 0, None, None, w)[1])
            assert [int(x) for x in levels[-2][1]] == runs
        assert all(K.same(levels[i], levels[i % 2]) for i in range(len(levels)))
    finally:
        table.close()
        csr.close()


def test_the_hub_carries_many_times_and_every_route_and_knob_gives_identical_rows(gg, hard):
    """1-hop walks of S extended from column 0: the hub's rows arrive as one run of 4 * HUB_ROWS rows or more, each weighing
    -2^63 — the low half carries thousands of times, the high half goes negative"""
    vid, src, dst, g, (es, ed, er, info), S, walks, w = hard
    ext_csr, _ = build_ext(gg, vid, es, ed, er)
    ext_ids = ext_csr.export()[3]
    csr = build(gg, vid, src, dst)
    table = gg.expand_khop_result(csr, 1, S)
    _, ext = gg.extend_edge(table, 1, ext_csr, 0)
    try:
        rows = X.extend_rows(g.vid[walks[1]], es, ed, er, 0)[0]
        assert rows.shape[0] >= 4 * X.HUB_ROWS
        Vp, Vx = csr.V, ext_csr.V
        assert Vp < LDS_KEYS[True] < Vx < LDS_KEYS[False]  # the ext table's keys fit the count form only
        base_st, base = check(gg, ext, 2, rows, 0, csr, g.vid, 0, None, None, w, route=1)
        hub_total = [t for i, t in zip(base[0].tolist(), base[2]) if i == info["hub"]][0]
        assert hub_total <= -(1 << 63) * 4 * X.HUB_ROWS and hub_total < -(1 << 64)
        by_w_st, by_w = check(gg, ext, 2, rows, 2, ext_csr, ext_ids, 0, csr, g.vid, w, route=2)  # scattered keys, does not fit
        cnt_st, cnt = check(gg, ext, 2, rows, 2, ext_csr, ext_ids, route=1)                        # the count form fits
        knobs = [(0, 0, 0), (1, 0, 0), (2, 0, 0), (0, Vp - 1, 0), (0, Vp, 0), (0, Vp + 1, 0), (1, Vp - 1, 0),
                 (0, Vx - 1, 0), (0, Vx, 0), (0, Vx + 1, 0), (1, Vx - 1, 0), (0, 0, 1), (1, 0, 1), (2, 0, 1), (0, 1, 0)]
        seen = set()
        for route, lds_keys, tiles in knobs:
            gg.debug_group(route, lds_keys)
            gg.max_grid_tiles(tiles)
            a = check(gg, ext, 2, rows, 0, csr, g.vid, 0, None, None, w, route=route_for(Vp, True, route, lds_keys))
            b = check(gg, ext, 2, rows, 2, ext_csr, ext_ids, 0, csr, g.vid, w, route=route_for(Vx, True, route, lds_keys))
            c = check(gg, ext, 2, rows, 2, ext_csr, ext_ids, route=route_for(Vx, False, route, lds_keys))
            assert K.same(a[1], base) and K.same(b[1], by_w) and K.same(c[1], cnt)
            seen |= {a[0]["route"], b[0]["route"], c[0]["route"]}
            assert route != 2 or {a[0]["route"], b[0]["route"], c[0]["route"]} == {2}
        assert seen == {1, 2}
        gg.debug_reset()  # restores the knob
        assert gg.group_by(ext, 2, 0, csr, fetch=False).stats["route"] == 1
        with pytest.raises(GGError) as e:
            gg.debug_group(3)
        assert e.value.code == GG_ERR_INVALID_ARG
    finally:
        ext.close()
        table.close()
        csr.close()
        ext_csr.close()


def test_both_csr_builds(gg, hard):
    vid, src, dst, g, (es, ed, er, info), S, walks, w = hard
    levels = []
    for legacy in (False, True):
        gg.force_legacy_build(legacy)
        ext_csr, _ = build_ext(gg, vid, es, ed, er)
        ext_ids = ext_csr.export()[3]
        csr = build(gg, vid, src, dst)
        table = gg.expand_khop_result(csr, 2, S)
        _, ext = gg.extend_edge(table, 2, ext_csr, 2)
        try:
            rows = X.extend_rows(g.vid[walks[2]], es, ed, er, 2)[0]
            for route in (1, 2):
                gg.debug_group(route)
                levels.append(check(gg, ext, 3, rows, 3, ext_csr, ext_ids, 1, csr, g.vid, w)[1])
                levels.append(check(gg, ext, 3, rows, 1, csr, g.vid, 3, ext_csr, ext_ids,
                                    np.arange(ext_ids.size, dtype=np.int64) * 1_000_003 - 5)[1])
        finally:
            ext.close()
            table.close()
            csr.close()
            ext_csr.close()
    assert all(K.same(levels[i], levels[i % 2]) for i in range(len(levels)))


@pytest.mark.parametrize("h", [1, 2, 3])
def test_grouping_the_walk_table_equals_gg_khop_aggregate(gg, hard, h):
    vid, src, dst, g, (es, ed, er, info), S, walks, w = hard
    csr = build(gg, vid, src, dst)
    table = gg.expand_khop_result(csr, h, S)
    try:
        for group, kc, wc in (("start", 0, h), ("end", h, 0)):
            for weights in (w, None):
                want = gg.khop_aggregate(csr, h, h, group, sources=S, weights=weights)
                got = gg.group_by(table, h, kc, csr, None if weights is None else wc, None, weights)
                try:
                    a, b = got.fetch(h), want.fetch(h)
                    assert len(a[0]) > 0 and K.same(a, b)
                    assert got.stats["groups"] == want.stats["groups"][h]
                    assert got.stats["rows_grouped"] == want.stats["walks"][h] == table.rows(h)
                    if weights is not None:
                        assert K.same(a, R.group_by(g.vid[walks[h]], kc, g.vid, wc, None, w)[0])
                finally:
                    got.close()
                    want.close()
    finally:
        table.close()
        csr.close()


def test_khop_aggregate_top_orders_the_groups(gg, hard):
    vid, src, dst, g, (es, ed, er, info), S, walks, w = hard
    ext_csr, _ = build_ext(gg, vid, es, ed, er)
    ext_ids = ext_csr.export()[3]
    csr = build(gg, vid, src, dst)
    table = gg.expand_khop_result(csr, 2, S)
    _, ext = gg.extend_edge(table, 2, ext_csr, 2)
    try:
        rows = X.extend_rows(g.vid[walks[2]], es, ed, er, 2)[0]
        level, _ = R.group_by(rows, 3, ext_ids, 1, g.vid, w)
        bias = (np.arange(ext_ids.size, dtype=np.int64) * 7919) % 100_003 - 50_000
        bias_of = {int(v): int(b) for v, b in zip(ext_ids.tolist(), bias.tolist())}
        agg = gg.group_by(ext, 3, 3, ext_csr, 1, csr, w)
        try:
            for n in (0, 1, 10, len(level[0]), len(level[0]) + 5):
                for desc in (True, False):
                    top = gg.khop_aggregate_top(agg, 3, "walks", desc, n)
                    assert K.same(top.fetch(3), TOP.top(level, n, "walks", desc))
                    top.close()
                    top = gg.khop_aggregate_top(agg, 3, "total", desc, n, csr=ext_csr, bias=bias)
                    assert K.same(top.fetch(3), TOP.top(level, n, "total", desc, bias_of))
                    top.close()
        finally:
            agg.close()
    finally:
        ext.close()
        table.close()
        csr.close()
        ext_csr.close()


def test_kinds_and_errors_leave_the_context_usable(gg, hard):
    vid, src, dst, g, (es, ed, er, info), S, walks, w = hard
    gg.staging_clear()
    gg.append_vertices(vid)
    gg.append_edges(src, dst)
    shard = gg.build_csr_shard(0, 2)
    csr = gg.build_csr()
    table = gg.expand_khop_result(csr, 2, S)
    closure = gg.walk_closure(csr, S[4:5], max_levels=2)
    other = type(gg)(0)
    other.append_vertices(vid[:4])
    other.append_edges(vid[:2], vid[2:4])
    foreign = other.build_csr()
    foreign_table = other.expand_khop_result(foreign, 1, None)
    want, want_st = R.group_by(g.vid[walks[2]], 1, g.vid, 2, None, w)
    wp = w.ctypes.data_as(C.POINTER(C.c_int64))

    def call(res, hops, kc, key, wc=-1, wcsr=None, weights=None, stats=True, out=True, ctx=None):
        st, o = GroupStats(), C.c_void_p()
        rc = gg.lib.gg_result_group_by(ctx or gg.ctx, res, hops, kc, key, wc, wcsr, weights, C.byref(st) if stats else None,
                                       C.byref(o) if out else None)
        assert rc != 0 and not o.value
        return rc

    agg = gg.group_by(table, 2, 1, csr, 2, None, w)
    try:
        # the three aggregate readers answer it; every other reader, this function included, refuses it
        assert agg.rows(2) == want_st["groups"] and K.same(agg.fetch(2), want)
        top = gg.khop_aggregate_top(agg, 2, "walks", True, 3)
        assert K.same(top.fetch(2), TOP.top(want, 3, "walks", True))
        top.close()
        n = C.c_uint64()
        assert gg.lib.gg_result_rows(agg.handle, 2, C.byref(n)) == GG_ERR_STATE
        assert call(agg.handle, 2, 0, csr.handle) == GG_ERR_STATE
        with pytest.raises(GGError):
            agg.rows(1)  # one level only
        bad = [
            (call(None, 2, 1, csr.handle), GG_ERR_INVALID_ARG),
            (call(table.handle, 2, 1, None), GG_ERR_INVALID_ARG),
            (call(table.handle, 2, 1, csr.handle, ctx=other.ctx), GG_ERR_INVALID_ARG),
            (call(table.handle, 2, 1, foreign.handle), GG_ERR_INVALID_ARG),                  # a key CSR of another context
            (call(table.handle, 2, 1, csr.handle, 2, foreign.handle, wp), GG_ERR_INVALID_ARG),  # a weight CSR of another
            (call(foreign_table.handle, 1, 1, csr.handle), GG_ERR_INVALID_ARG),              # a result of another context
            (call(table.handle, 3, 1, csr.handle), GG_ERR_INVALID_ARG),                      # hops outside the result
            (call(table.handle, 1, 1, csr.handle), GG_ERR_INVALID_ARG),
            (call(table.handle, 2, 3, csr.handle), GG_ERR_INVALID_ARG),                      # key column hops + 1
            (call(table.handle, 2, -1, csr.handle), GG_ERR_INVALID_ARG),
            (call(table.handle, 2, 1, csr.handle, 3, None, wp), GG_ERR_INVALID_ARG),         # weight column hops + 1
            (call(table.handle, 2, 1, csr.handle, -2, None, None), GG_ERR_INVALID_ARG),
            (call(table.handle, 2, 1, csr.handle, 2, None, None), GG_ERR_INVALID_ARG),       # a weight column without weights
            (call(table.handle, 2, 1, csr.handle, -1, None, wp), GG_ERR_INVALID_ARG),        # weights without a column
            (call(table.handle, 2, 1, csr.handle, stats=False, out=False), GG_ERR_INVALID_ARG),
            (call(table.handle, 2, 1, shard.handle), GG_ERR_STATE),                          # a shard as the key's table
            (call(table.handle, 2, 1, csr.handle, 2, shard.handle, wp), GG_ERR_STATE),       # ... as the weight's
            (call(closure.handle, 2, 1, csr.handle), GG_ERR_STATE),                          # no fixed-length table
        ]
        for i, (rc, code) in enumerate(bad):
            assert rc == code, (i, rc, code)
            again = gg.group_by(table, 2, 1, csr, 2, None, w)  # a correct call still works
            assert K.same(again.fetch(2), want)
            again.close()
        with pytest.raises(ValueError):
            gg.group_by(table, 2, 1, csr, 2, None, w[:-1])
    finally:
        agg.close()
        foreign_table.close()
        foreign.close()
        other.close()
        closure.close()
        table.close()
        shard.close()
        csr.close()
