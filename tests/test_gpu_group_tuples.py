"""GG.group_tuples (gg_result_group_tuples) against the restatement (tests/group_tuples_ref.py): the keys in order, all
six aggregates and the stats, for the column sets of plain and extended tables in the count form and the valued form, at the
row counts and run shapes a wavefront or a workgroup can get wrong, on both routes and at the capacity boundary, under
gg_debug_distinct's knobs and split launches (identical output), on sums that carry and wrap, min / max at the extremes,
groups without a value, tuples that differ in one place only, edge-case ids, against gg_result_group_by and
gg_result_distinct, on filtered, top, distinct and triangle tables, through the readers' slices and every error.

The 2^32-row refusal and the probe bound's GG_ERR_STATE cannot be reached at test size — the tuple table always has an
empty slot, and no test tries to fill it; both were checked by reading csrc/gg_tuples.h and csrc/gg_group_tuples.hip only."""
import ctypes as C

import numpy as np
import pytest

from duckdb_pgq_amd import GGError
from duckdb_pgq_amd.gg import GroupTuplesStats, KhopResult
from tests import distinct_ref as D
from tests import edge_filter_ref as F
from tests import edge_ids as E
from tests import group_by_ref as G
from tests import group_tuples_ref as T
from tests import value_rows_ref as R
from tests.distinct_tables import hard_tables
from tests.test_gpu_distinct import column_sets, default_slots
from tests.test_gpu_extend import build, fetch_all
from tests.test_gpu_value_rows import World, id_values

pytestmark = pytest.mark.gpu

GG_OK, GG_ERR_INVALID_ARG, GG_ERR_STATE = 0, -1, -6
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
LDS_GROUPS = {False: 6144, True: 1024}  # the default capacities of csrc/gg_group_tuples.hip: 48 KiB of 8 B / 48 B cells
i64p, u64p = C.POINTER(C.c_int64), C.POINTER(C.c_uint64)


@pytest.fixture(scope="module")
def hard():
    return hard_tables()


def route_for(groups, valued, route=0, lds_groups=0):
    cap = min(LDS_GROUPS[valued], lds_groups) if lds_groups else LDS_GROUPS[valued]
    return 0 if groups == 0 else 1 if route != 2 and groups <= cap else 2


def extreme_values(ids) -> np.ndarray:
    """one int64 per id: random over the whole signed range, with the extremes, -1 and 0 mixed in"""
    v = id_values(ids, "full")
    v[::5], v[1::7], v[2::11], v[3::13] = I64_MAX, I64_MIN, -1, 0
    return v


def check(gg, res, hops, rows, cols, vc=None, csr=None, ids=None, values=None, valid=None, slots=None, knob=(0, 0)):
    """one call against the restatement, with rows and stats-only; knob: what gg_debug_group_tuples was given.  Returns
    (stats, the fetched answer)"""
    want, want_st = T.group_tuples(rows, cols, vc, ids, values, valid)
    tg = gg.group_tuples(res, hops, cols, vc, csr, values, valid)
    try:
        st = tg.stats
        got = tg.fetch()
        print((hops, cols, vc), "device", st, "restatement", want_st)
        assert {k: st[k] for k in want_st} == want_st
        assert st["slots"] == (default_slots(rows.shape[0]) if slots is None else slots)
        assert st["route"] == route_for(want_st["groups"], vc is not None, *knob)
        assert want_st["groups"] <= st["probe_steps"]
        assert tg.shape() == (want_st["groups"], len(cols))
        assert got["keys"].shape == want["keys"].shape and T.same(got, want)
        only = gg.group_tuples(res, hops, cols, vc, csr, values, valid, fetch=False)
        assert only.handle is None
        assert {k: v for k, v in only.stats.items() if k != "probe_steps"} == {k: v for k, v in st.items() if k != "probe_steps"}
    finally:
        tg.close()
    return st, got


def check_forms(gg, res, hops, rows, cols, csr, ids, values, valid=None, value_cols=None, **kw):
    """the count form and the valued form over value_cols (default: one column inside cols, one outside where there is one)"""
    check(gg, res, hops, rows, cols, **kw)
    if value_cols is None:
        outside = [c for c in range(hops + 1) if c not in cols]
        value_cols = [cols[-1]] + outside[-1:]
    for vc in value_cols:
        check(gg, res, hops, rows, cols, vc, csr, ids, values, valid, **kw)


@pytest.mark.parametrize("hops", [1, 2])
def test_plain_walk_tables_with_edge_columns(gg, hard, hops):
    csr = build(gg, hard["vid"], hard["src"], hard["dst"])
    table = gg.expand_khop_edges(csr, hops, hard["S"])
    w = G.hub_weights(hard["vid"], hard["ext"][3]["hub"])  # tests/test_gpu_group_by.py's weights: the extremes, -2^63 on the hub
    try:
        rows = hard["walks"][hops]
        assert np.array_equal(fetch_all(table, hops), rows)
        for cols in column_sets(hops):
            check_forms(gg, table, hops, rows, cols, csr, hard["vid"], w)
    finally:
        table.close()
        csr.close()


@pytest.mark.parametrize("name", ["small", "mid", "big"])
def test_extended_tables(gg, hard, name):
    w = World(gg, hard, name)
    try:
        values = extreme_values(w.ext_ids)
        sets = column_sets(w.hops) if name != "big" else [[3], [0, 3], [0, 1, 2, 3]]
        for cols in sets:
            check_forms(gg, w.table, w.hops, w.rows, cols, w.ext_csr, w.ext_ids, values)
        # the persons' table as the values' table: only a message whose id is a person's as well has a value
        pv = extreme_values(hard["vid"])
        st, got = check(gg, w.table, w.hops, w.rows, [0], w.hops, w.csr, hard["vid"], pv)
        assert st["rows_valued"] == int(np.isin(w.rows[:, w.hops], hard["vid"]).sum()) < st["rows_in"]
    finally:
        w.close()


def star(gg, dst_of_row):
    """the 1-hop table of a star's centre, whose leaves are wired in the order of dst_of_row (leaf numbers): n rows
    (centre, leaf).  (csr, vertex ids, table, rows)"""
    dst_of_row = np.asarray(dst_of_row, np.int64)
    leaves = int(dst_of_row.max()) + 1 if dst_of_row.size else 1
    vid = 100 + 3 * np.arange(leaves + 1, dtype=np.int64)
    dst = vid[1 + dst_of_row]
    csr = build(gg, vid, np.full(dst.size, vid[0], np.int64), dst)
    table = gg.expand_khop_result(csr, 1, vid[:1] if dst.size else np.empty(0, np.int64))
    rows = fetch_all(table, 1)
    assert rows.shape == (dst.size, 2) and np.array_equal(rows[:, 1], dst)
    return csr, vid, table, rows


@pytest.mark.parametrize("n_rows", [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097])
def test_row_counts_around_the_wavefront_the_workgroup_and_the_lds_capacity(gg, n_rows):
    """every row its own tuple (1 024 groups are the valued form's LDS capacity), a third of the rows repeating, and one
    tuple for every row; both routes forced"""
    for leaves in sorted({max(n_rows, 1), max(2 * n_rows // 3, 1)}):
        csr, vid, table, rows = star(gg, np.arange(n_rows) % leaves)
        values = np.array([I64_MAX, I64_MIN, -I64_MAX, 3, -1], np.int64)[np.arange(vid.size) % 5]
        try:
            for route in (0, 1, 2):
                gg.debug_group_tuples(route)
                for cols in ([0], [1], [1, 0]):
                    st, got = check(gg, table, 1, rows, cols, knob=(route, 0))
                    if n_rows == 0:
                        assert st == {"rows_in": 0, "rows_valued": 0, "groups": 0, "slots": 0, "probe_steps": 0, "route": 0}
                    else:
                        assert st["groups"] == (1 if cols == [0] else min(n_rows, leaves))
                    st, got = check(gg, table, 1, rows, cols, 1, csr, vid, values, knob=(route, 0))
                    assert st["rows_valued"] == n_rows
        finally:
            gg.debug_reset()
            table.close()
            csr.close()


def test_equal_tuples_adjacent_apart_and_across_wavefront_and_workgroup_borders(gg):
    n, copies = 40, 30
    sorted_list = np.repeat(np.arange(n), copies)
    shuffled = np.tile(np.random.RandomState(5).permutation(n), copies)
    crossing = np.arange(600)
    crossing[60:71] = 60    # one tuple in rows 60..70: over the end of the first wavefront
    crossing[250:261] = 250  # and in rows 250..260: over the end of the first workgroup's rows
    for name, dst in (("adjacent", sorted_list), ("apart", shuffled), ("crossing", crossing)):
        csr, vid, table, rows = star(gg, dst)
        values = -(1 << 62) - 7 * np.arange(vid.size, dtype=np.int64)
        if name == "crossing":
            values[1 + 60], values[1 + 250] = I64_MIN, I64_MAX
        try:
            same_as_above = int((rows[1:, 1] == rows[:-1, 1]).sum())
            assert same_as_above == {"adjacent": n * (copies - 1), "apart": 0, "crossing": 20}[name]
            answers = []
            for route in (1, 2):
                for combine in (0, 1):
                    gg.debug_group_tuples(route)
                    gg.debug_distinct(0, combine)
                    for cols in ([1], [1, 0], [0]):
                        answers.append(check(gg, table, 1, rows, cols, 1, csr, vid, values, knob=(route, 0))[1])
                        check(gg, table, 1, rows, cols, knob=(route, 0))
            assert all(T.same(a, answers[i % 3]) for i, a in enumerate(answers))
            if name == "crossing":
                by_leaf = dict(zip(answers[0]["keys"][:, 0].tolist(), answers[0]["rows"].tolist()))
                assert by_leaf[int(vid[1 + 60])] == 11 and by_leaf[int(vid[1 + 250])] == 11
        finally:
            gg.debug_reset()
            table.close()
            csr.close()


@pytest.mark.parametrize("groups", [3, 4, 5])
def test_both_routes_and_the_capacity_boundary(gg, groups):
    """lds_groups = 4: capacity - 1, capacity and capacity + 1 groups"""
    csr, vid, table, rows = star(gg, np.arange(700) % groups)
    values = np.array([I64_MAX, 5, I64_MIN, -1, I64_MAX, -9], np.int64)[: vid.size]
    try:
        base = None
        seen = set()
        for route, lds in ((0, 0), (0, 4), (1, 4), (2, 4), (2, 0), (1, 0), (0, 1)):
            gg.debug_group_tuples(route, lds)
            for cols in ([1], [0, 1]):
                a = check(gg, table, 1, rows, cols, knob=(route, lds))
                b = check(gg, table, 1, rows, cols, 1, csr, vid, values, knob=(route, lds))
                seen |= {a[0]["route"], b[0]["route"]}
                assert a[0]["groups"] == b[0]["groups"] == groups
                if cols == [1]:
                    base = base or b[1]
                    assert T.same(b[1], base)
            if lds == 4:
                assert b[0]["route"] == (1 if route != 2 and groups <= 4 else 2)
        assert seen == {1, 2}
        gg.debug_reset()  # restores the knob
        assert gg.group_tuples(table, 1, [1], fetch=False).stats["route"] == 1
        with pytest.raises(GGError) as e:
            gg.debug_group_tuples(3)
        assert e.value.code == GG_ERR_INVALID_ARG
    finally:
        gg.debug_reset()
        table.close()
        csr.close()


def test_knobs_slot_counts_and_split_launches_give_identical_output(gg, hard):
    w = World(gg, hard, "mid")
    try:
        values = extreme_values(w.ext_ids)
        n = w.rows.shape[0]
        base = default_slots(n)
        assert base // 2 > n
        for cols, vc in (([3], 3), ([0, 3], 1), ([3, 2, 1, 0], None)):
            args = (vc, w.ext_csr, w.ext_ids, values) if vc is not None else ()
            first, want = check(gg, w.table, w.hops, w.rows, cols, *args)
            settings = [(slots, combine, 0, route) for slots in (2 * base, base // 2) for combine in (0, 1) for route in (1, 2)]
            settings += [(0, 0, 1, 1), (0, 1, 1, 2), (base // 2, 1, 1, 0), (0, 1, 0, 0)]
            for slots, combine, tiles, route in settings:
                gg.debug_distinct(slots, combine)
                gg.max_grid_tiles(tiles)  # 1: one workgroup a launch
                gg.debug_group_tuples(route)
                st, got = check(gg, w.table, w.hops, w.rows, cols, *args, slots=slots or base, knob=(route, 0))
                assert T.same(got, want) and st["groups"] == first["groups"]
                gg.debug_reset()
    finally:
        gg.debug_reset()
        w.close()


def test_sums_carry_and_wrap_min_and_max_at_the_extremes_and_groups_without_a_value(gg):
    """a star whose rows are (centre, leaf); the value of a row is the leaf's.  Grouped by the centre every value meets in
    one sum; grouped by the leaf's residue (a 2-hop table is not needed: the leaf column itself, with repeated leaves)"""
    cases = {
        "three_max": [I64_MAX] * 3,
        "min_next_to_minus_one": [I64_MIN, -1],
        "mixed_signs": [I64_MAX, I64_MIN, I64_MAX, -1, 1, I64_MIN, I64_MIN, 7],
        "hub": G.hub_weights(np.arange(300), 7).tolist(),
    }
    for name, vals in cases.items():
        dst = np.arange(len(vals))
        if name == "hub":
            dst = np.repeat(dst, 9)  # every leaf nine times: -2^63 nine times over carries out of the low word
        csr, vid, table, rows = star(gg, dst)
        values = np.zeros(vid.size, np.int64)
        values[1:] = vals
        try:
            for route in (1, 2):
                gg.debug_group_tuples(route)
                st, got = check(gg, table, 1, rows, [0], 1, csr, vid, values, knob=(route, 0))
                assert int(got["sum"][0]) == sum(int(v) for v in values[1:][dst].tolist())
                if name == "three_max":
                    assert int(got["sum"][0]) == 3 * I64_MAX > 1 << 64  # the low word carried
                if name == "min_next_to_minus_one":
                    assert int(got["sum"][0]) == I64_MIN - 1 < I64_MIN  # the high word went negative
                assert got["min"][0] == min(vals) and got["max"][0] == max(vals)
                check(gg, table, 1, rows, [1], 1, csr, vid, values, knob=(route, 0))
                # valid clears every other leaf, and the centre: grouped by the leaf, half the groups have no value
                bits = np.arange(vid.size) % 2 == 1
                valid = R.pack_valid(bits)
                st, got = check(gg, table, 1, rows, [1], 1, csr, vid, values, valid, knob=(route, 0))
                none = got["valued"] == 0
                assert none.any() and (len(vals) == 1 or (~none).any())
                assert not got["min"][none].any() and not got["max"][none].any() and not any(got["sum"][none])
                assert (got["rows"][none] > 0).all()
                st, got = check(gg, table, 1, rows, [0], 0, csr, vid, values, valid, knob=(route, 0))  # the centre: no value
                assert st["rows_valued"] == 0 and got["valued"].tolist() == [0] and got["rows"].tolist() == [dst.size]
        finally:
            gg.debug_reset()
            table.close()
            csr.close()


def test_a_value_cell_that_is_no_vertex_of_the_value_csr(gg, hard):
    """the values' table holds every third person only: the other cells have no value"""
    csr = build(gg, hard["vid"], hard["src"], hard["dst"])
    table = gg.expand_khop_result(csr, 2, hard["S"])
    try:
        rows = hard["walks"][2]
        # (a CSR of the same context, over a subset of the ids)
        sub = np.ascontiguousarray(hard["vid"][::3])
        gg.staging_clear()
        gg.append_vertices(sub)
        gg.append_edges(sub[:1], sub[1:2])
        sub_csr = gg.build_csr()
        try:
            values = extreme_values(sub)
            for cols in ([2], [0, 2], [1]):
                st, got = check(gg, table, 2, rows, cols, 2, sub_csr, sub, values)
                assert 0 < st["rows_valued"] < st["rows_in"]
                # grouped by the value cell itself, a group has a value in every row or in none
                assert 2 not in cols or ((got["valued"] == 0) | (got["valued"] == got["rows"])).all() and (got["valued"] == 0).any()
        finally:
            sub_csr.close()
    finally:
        table.close()
        csr.close()


def test_tuples_that_differ_in_one_place_only(gg):
    x = 5
    y, z = x + (1 << 32), x - (1 << 63)  # differ from x only above bit 32 / only in bit 63
    a, b, s = 11, 12, 20
    vid = np.array([a, b, x, y, z, s, I64_MIN, I64_MAX, -1, 0], np.int64)
    src = np.array([a, b, s, s, s, s, x, y, z, x, I64_MIN, I64_MAX, -1, 0, s, s], np.int64)
    dst = np.array([b, a, x, y, z, x, s, s, s, a, I64_MAX, -1, 0, I64_MIN, -1, I64_MIN], np.int64)
    csr = build(gg, vid, src, dst)
    S = np.array([a, b, s, x, y, z, s, I64_MIN, -1, 0, I64_MAX], np.int64)
    values = np.array([1, 2, I64_MAX, I64_MIN, -1, 0, 5, -5, I64_MAX, I64_MIN], np.int64)
    try:
        for hops in (1, 2):
            table = gg.expand_khop_edges(csr, hops, S)
            try:
                rows = fetch_all(table, hops)
                as_set = {tuple(r) for r in rows.tolist()}
                if hops == 1:
                    assert (a, b) in as_set and (b, a) in as_set and {(s, x), (s, y), (s, z)} <= as_set
                for cols in column_sets(hops) + ([[2, 1, 0], [2, 0], [1, 0]] if hops == 2 else []):
                    check_forms(gg, table, hops, rows, cols, csr, vid, values)
                got = check(gg, table, hops, rows, list(range(hops + 1)))[1]
                assert {tuple(r) for r in got["keys"].tolist()} == as_set  # (a, b) and (b, a), x, y and z are tuples of their own
                ones = check(gg, table, hops, rows, [1])[1]["keys"][:, 0].tolist()
                assert len(set(ones)) == len(ones) and {x, y, z} <= set(ones)
            finally:
                table.close()
    finally:
        csr.close()


@pytest.mark.parametrize("kind", ["wide", "dense_zero", "dense_max", "dense_min", "sparse"])
def test_edge_case_ids(gg, kind):
    eg = E.edge_graph(kind)
    sources = np.concatenate([eg.named[:4], eg.wired[[3, 3]], E.LISTED]).astype(np.int64)
    rows = eg.tri.vid[F.walks(eg.tri, sources, E.TABLE_HOPS)]
    csr = build(gg, eg.vid, eg.src, eg.dst)
    table = gg.expand_khop_result(csr, E.TABLE_HOPS, sources)
    try:
        assert np.array_equal(fetch_all(table, E.TABLE_HOPS), rows)
        w = E.weights_of(eg)
        for cols in column_sets(E.TABLE_HOPS) + [[2, 1, 0]]:
            check_forms(gg, table, E.TABLE_HOPS, rows, cols, csr, eg.vid, w)
    finally:
        table.close()
        csr.close()


def test_one_column_equals_group_by_and_the_keys_equal_distinct(gg, hard):
    w = World(gg, hard, "mid")
    try:
        values = extreme_values(w.ext_ids)
        for col in range(w.hops + 1):  # every cell is a vertex of ext_csr: gg_result_group_by's groups are the same
            tg = w.own(gg.group_tuples(w.table, w.hops, [col], col, w.ext_csr, values))
            got = tg.fetch()
            assert (got["valued"] == got["rows"]).all()
            agg = w.own(gg.group_by(w.table, w.hops, col, w.ext_csr, col, None, values))
            ids, walks, totals = agg.fetch(w.hops)
            mine = {(int(k), int(r), int(s) & ((1 << 128) - 1))
                    for k, r, s in zip(got["keys"][:, 0].tolist(), got["rows"].tolist(), got["sum"])}
            theirs = {(int(k), int(r), int(s) & ((1 << 128) - 1)) for k, r, s in zip(ids.tolist(), walks.tolist(), totals)}
            assert mine == theirs and len(mine) == tg.rows()
        for cols in column_sets(w.hops):
            tg = w.own(gg.group_tuples(w.table, w.hops, cols))
            _, out = gg.distinct(w.table, w.hops, cols)
            w.own(out)
            assert np.array_equal(tg.fetch()["keys"], fetch_all(out, len(cols) - 1))
    finally:
        w.close()


def test_filtered_top_distinct_and_triangle_tables_are_inputs_like_any_other(gg, hard):
    w = World(gg, hard, "mid")
    try:
        values = id_values(w.ext_ids, "seven")
        kept_rows, _, _ = R.filter_rows(w.rows, None, w.hops, w.ext_ids, values, None, -1, 1, "in")
        _, kept = gg.filter_value(w.table, w.hops, w.hops, w.ext_csr, values, None, -1, 1)
        w.own(kept)
        top_rows, _, _ = R.top_rows(w.rows, None, w.hops, w.ext_ids, values, None, -2, 2, "in", True, w.hops, 3000)
        _, top = gg.top_rows(w.table, w.hops, w.hops, w.ext_csr, values, 3000, None, -2, 2, "in", True, w.hops)
        w.own(top)
        _, semi = gg.filter_edge(w.table, w.hops, w.csr, 1, 0, "semi")
        w.own(semi)
        semi_rows = F.filter_rows(w.rows, hard["g"].A, hard["g"].index, 1, 0, "semi")[0]
        for res, rows in ((kept, kept_rows), (top, top_rows), (semi, semi_rows)):
            assert rows.shape[0] > 256
            for cols in ([3], [0, 3], [3, 0, 1, 2]):
                check_forms(gg, res, w.hops, rows, cols, w.ext_csr, w.ext_ids, values, value_cols=[3, 1])
        pairs, _, _ = D.distinct_rows(w.rows, [0, 3])
        _, dis = gg.distinct(w.table, w.hops, [0, 3])
        w.own(dis)
        check_forms(gg, dis, 1, pairs, [0], w.ext_csr, w.ext_ids, values, value_cols=[1])  # count(DISTINCT message) per source
        _, tri = gg.triangles_edges(w.csr, hard["S"])
        w.own(tri)
        tri_rows = fetch_all(tri, 2)
        assert tri_rows.shape[0] > 0
        for cols in ([0, 1, 2], [2, 0]):
            check_forms(gg, tri, 2, tri_rows, cols, w.ext_csr, w.ext_ids, values)
    finally:
        w.close()


def test_fetch_in_slices_and_with_every_pointer_null_but_one(gg, hard):
    w = World(gg, hard, "mid")
    try:
        values = extreme_values(w.ext_ids)
        want, st = T.group_tuples(w.rows, [0, 3], 3, w.ext_ids, values)
        tg = w.own(gg.group_tuples(w.table, w.hops, [0, 3], 3, w.ext_csr, values))
        n = st["groups"]
        assert n > 1000
        for offset, m in ((0, 1), (1, 255), (n - 3, 3), (n - 3, 100), (n, 5), (n + 7, 5), (500, None)):
            got = tg.fetch(offset, m)
            hi = n if m is None else min(n, offset + m)
            part = {k: v[offset:hi] for k, v in want.items()}
            assert got["keys"].shape[0] == max(0, hi - offset) and T.same(got, part)
        # one destination at a time: slot 0 / 1 are the key columns, 2..7 rows, valued, sum lo, sum hi, min, max
        columns = [want["keys"][:, 0], want["keys"][:, 1], want["rows"], want["valued"], want["lo"], want["hi"], want["min"],
                   want["max"]]
        for slot, column in enumerate(columns):
            buf = np.full(64, 0x5A, column.dtype)
            ptr = buf.view(np.int64).ctypes.data_as(i64p) if slot not in (2, 3) else buf.ctypes.data_as(u64p)
            keys = (i64p * 2)(ptr if slot == 0 else None, ptr if slot == 1 else None)
            args = [ptr if slot == s else None for s in range(2, 8)]
            got = C.c_uint32()
            rc = gg.lib.gg_tuple_groups_fetch(tg.handle, 10, 64, keys if slot < 2 else None, *args, C.byref(got))
            assert rc == GG_OK and got.value == 64 and np.array_equal(buf, column[10:74]), slot
        got = C.c_uint32(9)
        assert gg.lib.gg_tuple_groups_fetch(tg.handle, 0, 64, None, None, None, None, None, None, None, C.byref(got)) == GG_OK
        assert got.value == 64
        assert gg.lib.gg_tuple_groups_fetch(tg.handle, 0, 64, None, None, None, None, None, None, None, None) == GG_ERR_INVALID_ARG
        k = C.c_int()
        assert gg.lib.gg_tuple_groups_rows(tg.handle, None, C.byref(k)) == GG_OK and k.value == 2
        assert gg.lib.gg_tuple_groups_rows(tg.handle, None, None) == GG_ERR_INVALID_ARG
        # the count form: the value columns read as zeros
        cnt = w.own(gg.group_tuples(w.table, w.hops, [0, 3]))
        for slot in range(3, 8):
            buf = np.full(64, 0x5A, np.int64)
            args = [buf.ctypes.data_as(u64p if s == 3 else i64p) if slot == s else None for s in range(2, 8)]
            assert gg.lib.gg_tuple_groups_fetch(cnt.handle, n - 10, 64, None, *args, C.byref(got)) == GG_OK
            assert got.value == 10 and not buf[:10].any() and (buf[10:] == 0x5A).all()
    finally:
        w.close()


def test_degenerate_shapes(gg):
    vid = np.array([10, 20, 30], np.int64)
    csr = build(gg, vid, np.array([10, 20], np.int64), np.array([20, 10], np.int64))
    empty = gg.expand_khop_result(csr, 2, np.empty(0, np.int64))
    values = np.array([1, 2, 3], np.int64)
    try:
        for cols in ([0], [2, 0], [0, 1, 2]):
            for args in ((), (1, csr, vid, values)):
                st, got = check(gg, empty, 2, np.empty((0, 3), np.int64), cols, *args)
                assert st == {"rows_in": 0, "rows_valued": 0, "groups": 0, "slots": 0, "probe_steps": 0, "route": 0}
        made = C.c_void_p()  # stats may be NULL when rows are asked for
        cols = (C.c_int * 1)(1)
        two = gg.expand_khop_result(csr, 1, None)
        assert gg.lib.gg_result_group_tuples(gg.ctx, two.handle, 1, cols, 1, -1, None, None, None, None, C.byref(made)) == 0
        n = C.c_uint64()
        assert gg.lib.gg_tuple_groups_rows(made, C.byref(n), None) == GG_OK and n.value == 2
        gg.lib.gg_result_destroy(made)
        two.close()
    finally:
        empty.close()
        csr.close()


def test_kinds_and_errors_leave_the_context_usable(gg, hard):
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
    values = extreme_values(vid)
    vp = values.ctypes.data_as(i64p)
    bits = R.pack_valid(np.ones(vid.size, bool))
    bp = bits.ctypes.data_as(u64p)
    want, _ = T.group_tuples(hard["walks"][2], [2, 0], 1, vid, values)

    def call(res, hops, cols, n=None, vc=-1, graph=None, vals=None, valid=None, stats=True, out=True, ctx=None):
        st, o = GroupTuplesStats(), C.c_void_p(1)
        arr = None if cols is None else (C.c_int * max(len(cols), 1))(*cols)
        rc = gg.lib.gg_result_group_tuples(ctx or gg.ctx, res, hops, arr, len(cols or []) if n is None else n, vc, graph, vals,
                                           valid, C.byref(st) if stats else None, C.byref(o) if out else None)
        assert rc != 0 and (not out or not o.value)
        return rc

    kinds_csr = build(gg, RK.VID, RK.SRC, RK.DST, RK.ROWID)
    kinds = {}
    mine = None
    try:
        RK.make_results(gg, kinds_csr, kinds)
        t, h = table.handle, csr.handle
        bad = [
            (call(None, 2, [0]), GG_ERR_INVALID_ARG),
            (call(t, 2, None, n=1), GG_ERR_INVALID_ARG),                            # NULL cols
            (call(t, 2, [0], ctx=other.ctx), GG_ERR_INVALID_ARG),                   # a result of another context
            (call(foreign_table.handle, 1, [0]), GG_ERR_INVALID_ARG),
            (call(t, 3, [0]), GG_ERR_INVALID_ARG),                                  # hops outside the result's levels
            (call(t, 1, [0]), GG_ERR_INVALID_ARG),
            (call(t, -1, [0]), GG_ERR_INVALID_ARG),
            (call(t, 2, [0], n=0), GG_ERR_INVALID_ARG),                             # n_cols outside 1..hops + 1
            (call(t, 2, [0, 1, 2, 0], n=4), GG_ERR_INVALID_ARG),
            (call(t, 2, [3]), GG_ERR_INVALID_ARG),                                  # a column outside 0..hops
            (call(t, 2, [0, -1]), GG_ERR_INVALID_ARG),
            (call(t, 2, [1, 1]), GG_ERR_INVALID_ARG),                               # a repeated column
            (call(t, 2, [0], stats=False, out=False), GG_ERR_INVALID_ARG),          # nothing asked for
            (call(t, 2, [0], vc=3, graph=h, vals=vp), GG_ERR_INVALID_ARG),          # value_col outside -1..hops
            (call(t, 2, [0], vc=-2, graph=h, vals=vp), GG_ERR_INVALID_ARG),
            (call(t, 2, [0], vc=1, graph=None, vals=vp), GG_ERR_INVALID_ARG),       # a value column without its table
            (call(t, 2, [0], vc=1, graph=h, vals=None), GG_ERR_INVALID_ARG),        # ... without values
            (call(t, 2, [0], vc=1, graph=foreign.handle, vals=vp), GG_ERR_INVALID_ARG),  # a CSR of another context
            (call(t, 2, [0], vc=1, graph=shard.handle, vals=vp), GG_ERR_STATE),     # a shard CSR
            (call(t, 2, [0], vc=-1, graph=h), GG_ERR_INVALID_ARG),                  # the count form takes none of the three
            (call(t, 2, [0], vc=-1, vals=vp), GG_ERR_INVALID_ARG),
            (call(t, 2, [0], vc=-1, valid=bp), GG_ERR_INVALID_ARG),
        ]
        for name in ("closure", "reach", "levels", "paths"):          # the older kinds refuse one another so
            bad.append((call(kinds[name], RK.HOPS, [0]), GG_ERR_INVALID_ARG))
        for name in ("agg", "top", "pairs", "comps", "all_paths"):    # the kinds with a refusal contract
            bad.append((call(kinds[name], RK.HOPS, [0]), GG_ERR_STATE))
        mine = gg.group_tuples(table, 2, [2, 0], 1, csr, values)
        bad.append((call(mine.handle, 1, [0]), GG_ERR_STATE))          # its own output is no walk table
        for i, (rc, code) in enumerate(bad):
            assert rc == code, (i, rc, code)
        for i in range(0, len(bad), 8):  # a correct call still works, as often as an error came before it
            again = gg.group_tuples(table, 2, [2, 0], 1, csr, values)
            assert T.same(again.fetch(), want)
            again.close()
        # every other reader refuses the new kind: GG_ERR_STATE by expect_kind's rule, and GG_ERR_INVALID_ARG from the two
        # that answer every result without walk tables so (tests/test_gpu_result_kinds.py's table)
        for name, row in RK.CODE_TABLE.items():
            code = GG_ERR_INVALID_ARG if set(row[4:]) == {"I"} else GG_ERR_STATE
            assert RK.call_reader(gg, kinds_csr, name, mine.handle) == code, name
        n, k, got = C.c_uint64(), C.c_int(), C.c_uint32()
        assert gg.lib.gg_cheapest64_rows(mine.handle, C.byref(n)) == GG_ERR_STATE
        st = GroupTuplesStats()
        cols = (C.c_int * 1)(0)
        assert gg.lib.gg_result_distinct(gg.ctx, mine.handle, 1, cols, 1, 0, C.byref(gg.lib.gg_result_distinct.argtypes[6]._type_()),
                                         None) == GG_ERR_STATE
        # and the new readers refuse every other kind
        for name, res in kinds.items():
            assert gg.lib.gg_tuple_groups_rows(res, C.byref(n), C.byref(k)) == GG_ERR_STATE, name
            assert gg.lib.gg_tuple_groups_fetch(res, 0, 8, None, None, None, None, None, None, None, C.byref(got)) == GG_ERR_STATE, name
        # the walk tables of every origin are answered
        for name in ("walk", "walk_edges", "tri", "tri_edges"):
            res = KhopResult(gg, kinds[name], None)
            rows = fetch_all(res, RK.HOPS)
            check(gg, res, RK.HOPS, rows, [2, 0], 1, kinds_csr, RK.VID, np.arange(RK.VID.size, dtype=np.int64) - 4)
    finally:
        if mine is not None:
            mine.close()
        for res in kinds.values():
            gg.lib.gg_result_destroy(res)
        kinds_csr.close()
        foreign_table.close()
        foreign.close()
        other.close()
        table.close()
        shard.close()
        csr.close()
