"""gg_walk_closure, gg_reach_closure and gg_level_sets at the places tests/closure_edges.py builds inputs for: runs of
entries without children around locate_entry's window, tile borders, the wave patterns of k_reach_expand, keys that home
in the hash set's last slot, the growth rule's boundary, class counts up to 2^32 - 1, bit indices past 2^32, the level
sets' routes switching inside one call, the refusal of 2^32 children, slice fetches and the ids of tests/edge_ids.py.
Everything is compared exactly, row for row in the documented order and with the per-level counts, against the exact
references of the three operators' own test files (tests/test_closure_edges_cpu.py shows without a GPU that the inputs
reach the branches they are named for)."""
import ctypes
import dataclasses

import numpy as np
import pytest

from duckdb_pgq_amd import GGError
from tests import closure_edges as CE
from tests import edge_ids as EI
from tests.test_gpu_level_sets import COMBINATIONS, level_sets
from tests.test_gpu_reach_closure import reach

pytestmark = pytest.mark.gpu

GG_ERR_TOO_LARGE = -5
CASES = CE.all_cases()


def build(gg, case, assert_order=True):
    gg.staging_clear()
    gg.append_vertices(case.vertices)
    gg.append_edges(*(case.staged or (case.src, case.dst))[:2])
    csr = gg.build_csr()
    if assert_order:  # the cases are built on it: the dense index of a vertex is its position in the vertex table
        np.testing.assert_array_equal(csr.export()[3], case.vertices)
    return csr


def exact(case, op):
    if not hasattr(case, "_exact"):
        case._exact = {}
    if op not in case._exact:
        case._exact[op] = CE.exact_rows(case, op)
    return case._exact[op]


def assert_rows(got, per_level, expect, what):
    e0, e1, e_lev = expect
    assert got[0].size == e0.size, (what, got[0].size, e0.size)
    np.testing.assert_array_equal(got[2], e_lev, err_msg=str(what))
    np.testing.assert_array_equal(got[0], e0, err_msg=str(what))
    np.testing.assert_array_equal(got[1], e1, err_msg=str(what))
    assert per_level == [int((e_lev == L).sum()) for L in range(1, (int(e_lev.max()) if e_lev.size else 0) + 1)], what


def check_walk(gg, csr, case):
    res = gg.walk_closure(csr, case.seeds, None if case.bound < 0 else case.bound)
    try:
        got, per_level = res.fetch(), res.rows()
        assert res.levels() == len(per_level) and sum(per_level) == got[0].size
    finally:
        res.close()
    e_seed, e_rid, e_lev = exact(case, CE.WALK)
    if case.staged is not None:  # rows that were dropped keep their place in the rowids: the append positions
        e_rid = case.staged[2][e_rid]
    assert_rows(got, per_level, (e_seed, e_rid, e_lev), (case.name, CE.WALK))
    return per_level


def check_reach(gg, csr, case):
    per_level = None
    try:
        for mode, slots in case.reach_forms:
            gg.debug_reach_visited(mode, slots)
            got, levels = reach(gg, csr, case.seeds, case.classes, case.seen, case.n_classes)
            assert_rows(got, levels, exact(case, CE.REACH), (case.name, CE.REACH, mode, slots))
            assert per_level is None or levels == per_level
            per_level = levels
    finally:
        gg.debug_reach_visited(0, 0)
    return per_level


def check_levels(gg, csr, case):
    per_level = None
    try:
        for combination in case.levels_forms or COMBINATIONS:
            gg.debug_level_sets(*combination)
            got, levels = level_sets(gg, csr, case.seeds, case.classes, case.n_classes, case.bound)
            assert_rows(got, levels, exact(case, CE.LEVELS), (case.name, CE.LEVELS, combination))
            assert per_level is None or levels == per_level
            per_level = levels
    finally:
        gg.debug_level_sets(0, 0)
    return per_level


CHECKS = {CE.WALK: check_walk, CE.REACH: check_reach, CE.LEVELS: check_levels}


def check(gg, case, assert_order=True):
    """every operator the case applies to, on every form it names; returns the rows per level by operator"""
    csr = build(gg, case, assert_order)
    try:
        if not assert_order:
            case = dataclasses.replace(case, vertices=csr.export()[3])
        return {op: CHECKS[op](gg, csr, case) for op in case.ops}
    finally:
        csr.close()


@pytest.mark.parametrize("name", list(CASES))
def test_case(gg, name):
    case = CASES[name]
    per_level = check(gg, case)
    assert all(per_level.values())  # every case has rows in every operator
    totals = case.expect.get("totals")
    if totals and CE.WALK in per_level:
        assert per_level[CE.WALK][:len(totals)] == totals
    if "reach_level_1" in case.expect:
        assert per_level[CE.REACH][0] == case.expect["reach_level_1"]


def profiled(gg, call):
    """kernel name -> launches of one call"""
    gg.profile_reset()
    gg.profile_select(None)
    gg.profile(True)
    try:
        call()
    finally:
        gg.profile(False)
    return {name: count for name, (count, _) in gg.profile_get().items()}


def test_growth_rule_on_either_side_of_its_boundary(gg):
    """the bound 2 * (visited + M) before level 2 is 32: first slots of 32 and 33 stay (one reach_insert launch: the seen
    seed), 31 < 32 is rebuilt from the seen seed and level 1 (two more)"""
    case = CASES["growth_boundary"]
    csr = build(gg, case)
    launches = {}
    try:
        for slots in (CE.GROWTH_BOUND, CE.GROWTH_BOUND + 1, CE.GROWTH_BOUND - 1):
            gg.debug_reach_visited(2, slots)
            out = []
            counts = profiled(gg, lambda: out.append(reach(gg, csr, case.seeds, case.classes, case.seen)))
            assert_rows(*out[0], exact(case, CE.REACH), slots)
            launches[slots] = counts.get("reach_insert", 0)
    finally:
        gg.debug_reach_visited(0, 0)
        csr.close()
    assert launches == {CE.GROWTH_BOUND: 1, CE.GROWTH_BOUND + 1: 1, CE.GROWTH_BOUND - 1: 3}


def test_bit_indices_past_2_32(gg):
    """a bitmap of 70 001 x 70 001 bits (613 MB): classes on both sides of bit 2^32, vertices 0 and V - 1, and pairs
    whose bit indices agree modulo 2^32 — reach with the bitmap forced, level sets on both routes over it"""
    case = CE.bits_past_2_32()
    per_level = check(gg, case)
    cls, v, lev = exact(case, CE.LEVELS)
    assert set(cls.tolist()) == set(CE.BIG_SEED_CLASSES) and len(per_level[CE.LEVELS]) == 3
    assert {int(case.vertices[0]), int(case.vertices[-1])} <= set(v.tolist())
    assert max(int(c) * CE.BIG_V + 5 for c in cls.tolist()) > 1 << 32


def test_level_sets_switch_routes_inside_one_call(gg):
    """auto modes over a 50 MB bitmap: levels of 3, 45 000 and 6 children lie on both sides of the byte model's
    threshold (34 191, from gg_levels.hip's constants), so sort, compact and sort run in one call, each after
    k_levels_clear; over a 16-byte map the whole-map memset is the cheaper clearing and k_levels_clear never runs"""
    case = CE.route_switch()
    threshold = CE.levels_compact_threshold(CE.ROUTE_V, CE.ROUTE_CLASSES)
    assert [m >= threshold for m in case.expect["children"]] == [False, True, False]
    csr = build(gg, case)
    try:
        gg.debug_level_sets(0, 0)
        out = []
        counts = profiled(gg, lambda: out.append(level_sets(gg, csr, case.seeds, case.classes, case.n_classes, -1)))
        assert_rows(*out[0], exact(case, CE.LEVELS), case.name)
        assert out[0][1] == [3, 45000, 6]
    finally:
        csr.close()
    assert counts.get("levels_mark") == 1 and counts.get("reach_expand") == 2, counts
    assert counts.get("levels_clear") == 2 and counts.get("levels_rows") == 1, counts
    small = CE.memset_cheaper()
    csr = build(gg, small)
    try:
        out = []
        counts = profiled(gg, lambda: out.append(level_sets(gg, csr, small.seeds, small.classes, small.n_classes, -1)))
        assert_rows(*out[0], exact(small, CE.LEVELS), small.name)
        assert out[0][1] == [2, 2, 2]
    finally:
        csr.close()
    assert counts.get("levels_mark") == 3 and "levels_clear" not in counts and "reach_expand" not in counts, counts


def test_2_32_children_are_refused_by_every_operator_and_form(gg):
    """a hub of 65 536 children seeded 65 536 times: level 1 would have 2^32 rows.  (The accepted side just below is
    not run: it would write tens of GB.)"""
    case = CE.hub_65536()
    csr = build(gg, case)
    try:
        held = gg.pool()[1]
        calls = [(CE.WALK, None, lambda: gg.walk_closure(csr, case.seeds))]
        for form in CE.REACH_FORMS + ((0, 0),):
            calls.append((CE.REACH, form, lambda: gg.reach_closure(csr, case.seeds, case.classes, case.seen)))
        for form in COMBINATIONS:
            calls.append((CE.LEVELS, form, lambda: gg.level_sets(csr, case.seeds, case.classes)))
        for op, form, call in calls:
            if op == CE.REACH:
                gg.debug_reach_visited(*form)
            if op == CE.LEVELS:
                gg.debug_level_sets(*form)
            with pytest.raises(GGError) as err:
                call()
            assert err.value.code == GG_ERR_TOO_LARGE, (op, form, str(err.value))
            assert "2^32" in str(err.value)
            assert gg.pool()[1] == held, (op, form)
        gg.debug_reach_visited(0, 0)
        gg.debug_level_sets(0, 0)
        once = dataclasses.replace(case, seeds=case.seeds[:1], classes=case.classes[:1], seen=case.seen[:1])
        for op in CE.ALL_OPS:
            assert CHECKS[op](gg, csr, once) == [1 << 16]
        assert gg.pool()[1] == held
    finally:
        gg.debug_reach_visited(0, 0)
        gg.debug_level_sets(0, 0)
        csr.close()


FILL64, FILL32 = -0x5A5A5A5A5A5A5A5B, 0x5A5A5A5A


@pytest.mark.parametrize("op", CE.ALL_OPS)
def test_slices_of_levels_of_unequal_size(gg, op):
    """the fetch calls themselves: offsets inside a level, on a level border, one before the end, at the end and past
    it; max_rows that end inside a level and across several; with a level array and without"""
    case = CE.unequal_levels()
    sizes = case.expect["levels"]
    borders = np.cumsum(sizes).tolist()
    total = borders[-1]
    csr = build(gg, case)
    try:
        if op == CE.WALK:
            res = gg.walk_closure(csr, case.seeds)
        elif op == CE.REACH:
            res = gg.reach_closure(csr, case.seeds, case.classes, case.seen)
        else:
            res = gg.level_sets(csr, case.seeds, case.classes)
        try:
            assert res.rows() == sizes
            whole = res.fetch()
            assert_rows(whole, res.rows(), exact(case, op), op)
            assert whole[2].tolist() == [L + 1 for L, n in enumerate(sizes) for _ in range(n)]
            fetch = getattr(gg.lib, res._fetch_fn)
            i64p, i32p = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
            for offset in (0, 1, borders[0], borders[1] - 1, borders[1], borders[2] + 1, total - 1, total, total + 7):
                for max_rows in (0, 1, 2, 4, 9, total, total + 100):
                    for with_level in (True, False):
                        room = max_rows + 2
                        a, b = np.full(room, FILL64, np.int64), np.full(room, FILL64, np.int64)
                        lev = np.full(room, FILL32, np.int32)
                        n = ctypes.c_uint32(12345)
                        rc = fetch(res.handle, offset, max_rows, a.ctypes.data_as(i64p), b.ctypes.data_as(i64p),
                                   lev.ctypes.data_as(i32p) if with_level else None, ctypes.byref(n))
                        what = (offset, max_rows, with_level)
                        assert rc == 0, what
                        want = max(0, min(max_rows, total - offset))
                        assert n.value == want, what
                        np.testing.assert_array_equal(a[:want], whole[0][offset:offset + want], err_msg=str(what))
                        np.testing.assert_array_equal(b[:want], whole[1][offset:offset + want], err_msg=str(what))
                        assert (a[want:] == FILL64).all() and (b[want:] == FILL64).all(), what
                        if with_level:
                            np.testing.assert_array_equal(lev[:want], whole[2][offset:offset + want], err_msg=str(what))
                            assert (lev[want:] == FILL32).all(), what
                        else:
                            assert (lev == FILL32).all()
        finally:
            res.close()
    finally:
        csr.close()


def edge_id_case(name, vid, src, dst, seeds, walk_bound, levels_bound):
    """the table is staged whole; the references see the rows whose endpoints are both vertices, under their append
    positions"""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    keep = np.isin(src, vid) & np.isin(dst, vid)
    n = seeds.size
    case = CE.Case(name, vid, src[keep], dst[keep], seeds, np.arange(n) % 3, np.arange(n) % 2 == 0, n_classes=3,
                   staged=(src, dst, np.flatnonzero(keep)))
    return case, walk_bound, levels_bound


@pytest.mark.parametrize("kind", EI.PLACEMENTS)
def test_edge_case_ids(gg, kind):
    """the graph of tests/edge_ids.py under each placement (the three dictionaries, the 32 / 64-bit boundaries): seeds
    are the named boundary ids, wired vertices (one twice), the hub and ids that are no vertex"""
    eg = EI.edge_graph(kind)
    seeds = eg.sources()
    assert np.isin(eg.named[:4], seeds).all() and EI.NOT_A_VERTEX in seeds.tolist()
    assert (~np.isin(eg.src, eg.vid) | ~np.isin(eg.dst, eg.vid)).any()  # dangling rows: positions and rowids differ
    case, walk_bound, levels_bound = edge_id_case(f"edge_ids_{kind}", eg.vid, eg.src, eg.dst, seeds, 2, 3)
    per_level = {}
    for op, bound in ((CE.WALK, walk_bound), (CE.REACH, -1), (CE.LEVELS, levels_bound)):
        one = dataclasses.replace(case, ops=(op,), bound=bound)
        per_level.update(check(gg, one, assert_order=False))
    assert len(per_level[CE.WALK]) == 2 and len(per_level[CE.LEVELS]) == 3 and len(per_level[CE.REACH]) >= 2
    cls, v, _ = exact(dataclasses.replace(case, bound=-1), CE.REACH)
    assert np.isin(eg.named, v).all()  # the boundary ids come back as rows


@pytest.mark.parametrize("name", ["one_vertex", "two_vertices"])
def test_edge_case_ids_on_one_and_two_vertices(gg, name):
    vid, src, dst = EI.tiny_graphs()[name]
    seeds = np.array([-1, EI.I64_MAX, EI.NOT_A_VERTEX, EI.I64_MIN, -1], np.int64)
    case, _, _ = edge_id_case(name, vid, src, dst, seeds, 4, 4)
    case.bound = 4
    per_level = check(gg, case, assert_order=False)
    if name == "one_vertex":
        assert per_level == {CE.WALK: [], CE.REACH: [], CE.LEVELS: []}
    else:  # a 2-cycle: seeds -1 (twice) and INT64_MAX walk round it; reach ends after a level
        assert per_level[CE.WALK] == [3] * 4 and per_level[CE.LEVELS] == [3, 3, 3, 3]
        assert per_level[CE.REACH] == [2]  # (0, MAX) and (1, MAX); (0, -1) and (1, -1) are seen seeds
