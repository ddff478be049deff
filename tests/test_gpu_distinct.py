"""GG.distinct (gg_result_distinct) against the numpy restatement (tests/distinct_ref.py): the stats and every row in input
order, for single columns, pairs in both orders and all columns of plain, extended and filtered tables, with and without the
combining of adjacent lanes, under forced slot counts and split launches, on row counts around the wavefront, the
workgroup and the tile, on tuples that differ in one place only, on edge-case ids, chained with every other reader of a walk
table (table 0 included), on degenerate shapes and through every error.

The tables are tests/distinct_tables.py's (tests/test_gpu_value_rows.py's).  Outputs of fewer than 200 000 rows are fetched
and compared in order, larger ones by count and digest; every table here is smaller, so one test lowers that bound.

The 2^32-row refusal and the probe bound's GG_ERR_STATE cannot be reached at test size — the table always has an empty
slot, and no test tries to fill it; both were checked by reading csrc/gg_distinct.hip only."""
import ctypes as C

import numpy as np
import pytest

from duckdb_pgq_amd import GGError
from duckdb_pgq_amd.gg import DistinctStats, KhopResult
from tests import distinct_ref as D
from tests import edge_filter_ref as F
from tests import edge_ids as E
from tests import extend_ref as X
from tests import group_by_ref as G
from tests import khop_aggregate_ref as K
from tests import value_rows_ref as R
from tests.distinct_tables import hard_tables
from tests.test_gpu_extend import build, build_ext, fetch_all
from tests.test_gpu_value_rows import World, id_values

pytestmark = pytest.mark.gpu

GG_ERR_INVALID_ARG, GG_ERR_STATE = -1, -6
FETCH_BELOW = 200_000
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


@pytest.fixture(scope="module")
def hard():
    return hard_tables()


def default_slots(n: int) -> int:
    """the next power of two >= 2 n (include/gg.h); 0 for an empty table"""
    p = 1
    while p < 2 * n:
        p <<= 1
    return p if n else 0


def column_sets(hops: int):
    """every single column, the pairs [0, h], [h, 0], [1, 2], and all columns"""
    sets = [[c] for c in range(hops + 1)]
    if hops >= 1:
        sets += [[0, hops], [hops, 0]]
    if hops >= 2:
        sets.append([1, 2])
    sets.append(list(range(hops + 1)))
    return [s for i, s in enumerate(sets) if s not in sets[:i]]


def check(gg, res, hops, rows, cols, slots=None, digest=None):
    """one column list against the restatement, count-only and materialised; digest: (csr, id -> dense index) of a graph
    every cell is a vertex of.  Returns (stats, the output's rows)"""
    want_rows, _, want = D.distinct_rows(rows, cols)
    only = gg.distinct(res, hops, cols, materialise=False)
    st, out = gg.distinct(res, hops, cols)
    oh = len(cols) - 1
    print((hops, cols), "device", st, "restatement", want)
    try:
        assert {k: st[k] for k in want} == want and {k: only[k] for k in want} == want
        assert st["slots"] == only["slots"] == (default_slots(rows.shape[0]) if slots is None else slots)
        assert st["slots"] == 0 or (st["slots"] > rows.shape[0] and st["slots"] & (st["slots"] - 1) == 0)
        # every probing row looks at one slot at least, and adjacent equal rows of a wavefront at none
        assert want["rows_out"] <= st["probe_steps"] and want["rows_out"] <= only["probe_steps"]
        assert out.rows(oh) == want["rows_out"]
        got = None
        if want["rows_out"] < FETCH_BELOW:
            got = fetch_all(out, oh)
            assert np.array_equal(got, want_rows)
        else:
            assert digest is not None
            assert out.digest(digest[0], oh) == (want["rows_out"], F.digest_dense_rows(X.dense_rows(digest[1], want_rows)))
        if oh and want["rows_out"]:  # the output never carries edge columns (an empty table is asked for none)
            with pytest.raises(GGError):
                out.fetch_edges(oh, 0)
    finally:
        out.close()
    return st, got


def check_both_ways(gg, res, hops, rows, cols, **kw):
    """combine 0 and 1 give identical rows (both equal the restatement's)"""
    first, _ = check(gg, res, hops, rows, cols, **kw)
    gg.debug_distinct(0 if "slots" not in kw else kw["slots"], 1)
    second, _ = check(gg, res, hops, rows, cols, **kw)
    gg.debug_distinct(0 if "slots" not in kw else kw["slots"], 0)
    assert second["probe_steps"] >= rows.shape[0]  # without combining every row probes
    return first, second


@pytest.mark.parametrize("hops", [1, 2])
def test_plain_walk_tables_with_edge_columns(gg, hard, hops):
    csr = build(gg, hard["vid"], hard["src"], hard["dst"])
    table = gg.expand_khop_edges(csr, hops, hard["S"])
    try:
        rows = hard["walks"][hops]
        assert np.array_equal(fetch_all(table, hops), rows)
        assert fetch_all(table, hops, edges=True).shape == (rows.shape[0], hops)  # the input has edge columns
        for cols in column_sets(hops):
            a, b = check_both_ways(gg, table, hops, rows, cols)
            if cols == [0]:
                # the rows of a listed source are adjacent: five runs, so at most a lane per run and wavefront probes, and
                # a probe passes over slots of other tuples only, of which there are at most three
                assert a["rows_out"] <= 4 and a["probe_steps"] <= 4 * ((rows.shape[0] + 63) // 64 + 5)
    finally:
        table.close()
        csr.close()


@pytest.mark.parametrize("name", ["small", "mid", "big"])
def test_extended_tables(gg, hard, name):
    w = World(gg, hard, name)
    try:
        for cols in column_sets(w.hops):
            check_both_ways(gg, w.table, w.hops, w.rows, cols)
        if name == "big":
            st, _ = check(gg, w.table, w.hops, w.rows, [3])
            assert st["rows_out"] == 2937 and st["rows_in"] == 172_475
    finally:
        w.close()


def test_large_outputs_by_count_and_digest(gg, hard):
    w = World(gg, hard, "mid")
    global FETCH_BELOW
    keep, FETCH_BELOW = FETCH_BELOW, 1000
    try:
        index = {int(v): i for i, v in enumerate(w.ext_ids.tolist())}
        for cols in ([0, 3], [3, 2, 1, 0], [3]):
            st, got = check(gg, w.table, w.hops, w.rows, cols, digest=(w.ext_csr, index))
            assert got is None and st["rows_out"] >= 1000
    finally:
        FETCH_BELOW = keep
        w.close()


def star(gg, n_rows: int, leaves: int):
    """the 1-hop table of a star's centre: n rows (centre, leaf i % leaves)"""
    vid = np.arange(100, 100 + leaves + 1, dtype=np.int64)
    dst = vid[1 + np.arange(n_rows) % leaves]
    csr = build(gg, vid, np.full(n_rows, vid[0], np.int64), dst)
    table = gg.expand_khop_result(csr, 1, vid[:1] if n_rows else np.empty(0, np.int64))
    rows = fetch_all(table, 1)
    assert rows.shape == (n_rows, 2) and (n_rows == 0 or np.array_equal(rows[:, 1], dst))
    return csr, table, rows


@pytest.mark.parametrize("n_rows", [0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097])
def test_row_counts_around_the_wavefront_the_workgroup_and_the_tile(gg, n_rows):
    for leaves in sorted({max(n_rows, 1), max(2 * n_rows // 3, 1)}):  # pairwise different rows; a third of them repeats
        csr, table, rows = star(gg, n_rows, leaves)
        try:
            for cols in ([0], [1], [1, 0]):
                a, _ = check_both_ways(gg, table, 1, rows, cols)
                if n_rows == 0:
                    assert a == {"rows_in": 0, "rows_out": 0, "slots": 0, "probe_steps": 0}
                elif cols != [0]:
                    assert a["rows_out"] == min(n_rows, leaves)
        finally:
            table.close()
            csr.close()


def test_equal_rows_all_adjacent_and_never_adjacent(gg):
    """a star with parallel edge rows: the 1-hop table of the centre holds (centre, leaf) in the rows' append order, so a
    sorted and a shuffled list of the same multiset of leaves are the two tables"""
    for n, copies in ((50, 40), (5, 400)):
        adjacency_case(gg, n, copies)


def adjacency_case(gg, n, copies):
    vid = np.arange(1000, 1000 + n + 1, dtype=np.int64)
    leaves = vid[1:]
    sorted_list = np.repeat(leaves, copies)
    shuffled = np.tile(leaves[np.random.RandomState(5).permutation(n)], copies)
    assert np.array_equal(np.sort(shuffled), sorted_list)
    found = {}
    for name, dst in (("adjacent", sorted_list), ("apart", shuffled)):
        csr = build(gg, vid, np.full(dst.size, vid[0], np.int64), dst)
        table = gg.expand_khop_result(csr, 1, vid[:1])
        try:
            rows = fetch_all(table, 1)
            assert np.array_equal(rows[:, 1], dst) and (rows[:, 0] == vid[0]).all()
            same_as_above = (rows[1:] == rows[:-1]).all(axis=1)
            assert same_as_above.sum() == (n * (copies - 1) if name == "adjacent" else 0)
            for cols in ([1], [1, 0]):
                a, b = check_both_ways(gg, table, 1, rows, cols)
                found[(name, tuple(cols))] = a
                assert a["rows_out"] == n
        finally:
            table.close()
            csr.close()
    # only the first lane of a run probes: n runs, cut by the wavefronts' borders, and a probe passes over slots of
    # other tuples only; where no equal rows are adjacent every row probes
    bound = (n + (n * copies + 63) // 64) * n
    assert found[("adjacent", (1,))]["probe_steps"] <= bound
    assert found[("apart", (1,))]["probe_steps"] >= n * copies
    if n == 5:
        assert bound < n * copies


def test_slots_forced_to_the_minimum_and_around_the_default(gg):
    for n_rows, least in ((4095, 4096), (4096, 8192)):
        csr, table, rows = star(gg, n_rows, n_rows)  # pairwise different rows
        try:
            gg.debug_distinct(1, 0)
            st, got = check(gg, table, 1, rows, [1], slots=least)
            assert st["slots"] == least and st["rows_out"] == n_rows and np.array_equal(got, rows[:, 1:])
            st, got = check(gg, table, 1, rows, [0, 1], slots=least)
            assert st["rows_out"] == n_rows
            gg.debug_distinct(least - 1, 1)  # rounded up to a power of two
            assert check(gg, table, 1, rows, [1, 0], slots=least)[0]["rows_out"] == n_rows
            gg.debug_reset()
            assert check(gg, table, 1, rows, [1])[0]["slots"] == 8192  # gg_debug_reset clears the knob
        finally:
            gg.debug_reset()
            table.close()
            csr.close()


def test_a_single_tuple_repeated(gg):
    vid = np.array([7, 8], np.int64)
    csr = build(gg, vid, np.full(1000, 7, np.int64), np.full(1000, 8, np.int64))
    table = gg.expand_khop_edges(csr, 1, vid[:1])
    try:
        rows = fetch_all(table, 1)
        assert rows.shape == (1000, 2) and (rows == [7, 8]).all()
        for slots in (0, 1):
            gg.debug_distinct(slots, 0)
            for cols in ([0], [1], [0, 1], [1, 0]):
                a, b = check_both_ways(gg, table, 1, rows, cols, slots=1024 if slots else 2048)
                assert a["rows_out"] == 1 and b["probe_steps"] == 1000  # every row finds its tuple in its home slot
    finally:
        table.close()
        csr.close()


def test_slot_counts_and_split_launches_give_identical_rows(gg, hard):
    w = World(gg, hard, "mid")
    try:
        n = w.rows.shape[0]
        base = default_slots(n)
        assert base == 65_536 and base // 2 > n
        for cols in ([3], [0, 3], [3, 2, 1, 0]):
            first, rows_default = check(gg, w.table, w.hops, w.rows, cols)
            for slots in (2 * base, base // 2):
                for combine in (0, 1):
                    gg.debug_distinct(slots, combine)
                    st, got = check(gg, w.table, w.hops, w.rows, cols, slots=slots)
                    assert np.array_equal(got, rows_default) and st["rows_out"] == first["rows_out"]
            gg.debug_reset()
            gg.max_grid_tiles(1)  # one workgroup a launch: both passes stride over 99 groups, the write pass takes 99 launches
            st, got = check(gg, w.table, w.hops, w.rows, cols)
            assert np.array_equal(got, rows_default)
            gg.debug_distinct(base // 2, 1)
            st, got = check(gg, w.table, w.hops, w.rows, cols, slots=base // 2)
            assert np.array_equal(got, rows_default)
            gg.debug_reset()
    finally:
        w.close()


def test_tuples_that_differ_in_one_place_only(gg):
    x = 5
    y, z = x + (1 << 32), x - (1 << 63)  # differ from x only above bit 32 / only in bit 63
    a, b, s = 11, 12, 20
    vid = np.array([a, b, x, y, z, s, I64_MIN, I64_MAX, -1, 0], np.int64)
    src = np.array([a, b, s, s, s, s, x, y, z, x, I64_MIN, I64_MAX, -1, 0, s, s], np.int64)
    dst = np.array([b, a, x, y, z, x, s, s, s, a, I64_MAX, -1, 0, I64_MIN, -1, I64_MIN], np.int64)
    csr = build(gg, vid, src, dst)
    S = np.array([a, b, s, x, y, z, s, I64_MIN, -1, 0, I64_MAX], np.int64)
    try:
        for hops in (1, 2):
            table = gg.expand_khop_edges(csr, hops, S)
            try:
                rows = fetch_all(table, hops)
                as_set = {tuple(r) for r in rows.tolist()}
                if hops == 1:
                    assert (a, b) in as_set and (b, a) in as_set
                    assert {(s, x), (s, y), (s, z)} <= as_set
                else:
                    assert (s, x, s) in as_set and (s, x, a) in as_set  # equal in all but the last chosen column
                    assert {(s, x, s), (s, y, s), (s, z, s)} <= as_set  # equal but for the middle one
                for cell in (I64_MIN, I64_MAX, -1, 0):
                    assert (rows == cell).any()
                for cols in column_sets(hops) + ([[2, 1, 0], [2, 0], [1, 0]] if hops == 2 else []):
                    check_both_ways(gg, table, hops, rows, cols)
                # (a, b) and (b, a) are two tuples, and so are ids that share their low or their other 63 bits
                out_rows = check(gg, table, hops, rows, list(range(hops + 1)))[1]
                assert {tuple(r) for r in out_rows.tolist()} == as_set
                ones = check(gg, table, hops, rows, [1])[1][:, 0].tolist()
                assert len(set(ones)) == len(ones) and {x, y, z} <= set(ones)
            finally:
                table.close()
    finally:
        csr.close()


@pytest.mark.parametrize("kind,legacy", [("wide", False), ("wide", True), ("dense_zero", False), ("dense_max", False),
                                         ("dense_min", False), ("sparse", False)])
def test_edge_case_ids_under_both_csr_builds(gg, kind, legacy):
    eg = E.edge_graph(kind)
    sources = np.concatenate([eg.named[:4], eg.wired[[3, 3]], E.LISTED]).astype(np.int64)
    rows = eg.tri.vid[F.walks(eg.tri, sources, E.TABLE_HOPS)]
    gg.force_legacy_build(legacy)
    csr = build(gg, eg.vid, eg.src, eg.dst)
    table = gg.expand_khop_result(csr, E.TABLE_HOPS, sources)
    try:
        assert np.array_equal(fetch_all(table, E.TABLE_HOPS), rows)
        assert all(np.isin(eg.named, rows[:, c]).any() for c in (0, 2))  # the columns hold the edge-case ids
        for cols in column_sets(E.TABLE_HOPS) + [[2, 1, 0]]:
            check_both_ways(gg, table, E.TABLE_HOPS, rows, cols)
    finally:
        table.close()
        csr.close()


# ---- chains
def test_chain_distinct_extend_group_closes_the_friends_of_friends_gap(gg, hard):
    """2-hop -> distinct([2]) -> extend_edge from column 0 of the one-column table -> group_by by the message: every
    message of a friend of a friend once, whatever the number of walks that reach that person"""
    es, ed, er, _ = hard["ext"]
    csr = build(gg, hard["vid"], hard["src"], hard["dst"])
    ext_csr, _ = build_ext(gg, hard["vid"], es, ed, er)
    ext_ids = ext_csr.export()[3]
    walk = gg.expand_khop_edges(csr, 2, hard["S"])
    opened = [walk]
    try:
        two = hard["walks"][2]
        persons, _, _ = D.distinct_rows(two, [2])
        joined, _, want_ext = X.extend_rows(persons, es, ed, er, 0)
        want, _ = G.group_by(joined, 1, ext_ids)
        st, ends = gg.distinct(walk, 2, [2])
        opened.append(ends)
        assert st["rows_out"] == persons.shape[0] < two.shape[0] and np.array_equal(fetch_all(ends, 0), persons)
        xst, msgs = gg.extend_edge(ends, 0, ext_csr, 0)
        opened.append(msgs)
        assert xst == want_ext and np.array_equal(fetch_all(msgs, 1), joined)
        agg = gg.group_by(msgs, 1, 1, ext_csr)
        opened.append(agg)
        assert K.same(agg.fetch(1), want)
        # the same chain without the distinct counts a message once per walk that reaches its creator: the gap
        xst2, msgs_all = gg.extend_edge(walk, 2, ext_csr, 2)
        opened.append(msgs_all)
        agg_all = gg.group_by(msgs_all, 3, 3, ext_csr)
        opened.append(agg_all)
        per_walk, _ = G.group_by(X.extend_rows(two, es, ed, er, 2)[0], 3, ext_ids)
        assert K.same(agg_all.fetch(3), per_walk)
        assert np.array_equal(per_walk[0], want[0]) and per_walk[1] != want[1] and sum(per_walk[1]) > sum(want[1])
    finally:
        for o in reversed(opened):
            o.close()
        ext_csr.close()
        csr.close()


def test_chain_count_distinct_messages_per_source(gg, hard):
    """extended table -> distinct([0, 3]) -> group_by column 0: count(DISTINCT message) per source"""
    w = World(gg, hard, "mid")
    try:
        pairs, _, _ = D.distinct_rows(w.rows, [0, 3])
        st, out = gg.distinct(w.table, w.hops, [0, 3])
        w.own(out)
        assert np.array_equal(fetch_all(out, 1), pairs)
        agg = w.own(gg.group_by(out, 1, 0, w.csr))
        ids, walks, _ = agg.fetch(1)
        want = {int(s): len(set(w.rows[w.rows[:, 0] == s, 3].tolist())) for s in np.unique(w.rows[:, 0]).tolist()}
        assert dict(zip(ids.tolist(), [int(x) for x in walks.tolist()])) == want
        per_row = {int(s): int((w.rows[:, 0] == s).sum()) for s in want}
        assert any(per_row[s] > want[s] for s in want)  # count(*) would have said more
        # distinct of a distinct: the identity, in either column order
        st2, again = gg.distinct(out, 1, [0, 1])
        w.own(again)
        assert st2["rows_in"] == st2["rows_out"] == pairs.shape[0] and np.array_equal(fetch_all(again, 1), pairs)
        st3, swapped = gg.distinct(out, 1, [1, 0])
        w.own(swapped)
        assert np.array_equal(fetch_all(swapped, 1), pairs[:, ::-1])
    finally:
        w.close()


def test_distinct_pairs_equal_the_pair_counts_of_an_independent_kernel(gg, hard):
    csr = build(gg, hard["vid"], hard["src"], hard["dst"])
    S = hard["S"]
    walk = gg.expand_khop_result(csr, 2, S)
    pc = gg.khop_pair_counts(csr, 2, 2, S)
    try:
        st, out = gg.distinct(walk, 2, [0, 2])
        got = {tuple(r) for r in fetch_all(out, 1).tolist()}
        out.close()
        idx, ids, walks = pc.fetch(2)
        assert (walks != 0).all()
        want = {(int(S[i]), int(v)) for i, v in zip(idx.tolist(), ids.tolist())}
        assert got == want and st["rows_out"] == len(want) < st["rows_in"]
    finally:
        pc.close()
        walk.close()
        csr.close()


def test_every_reader_answers_an_output_table_0_included(gg, hard):
    g = hard["g"]
    csr = build(gg, hard["vid"], hard["src"], hard["dst"])
    walk = gg.expand_khop_edges(csr, 2, hard["S"])
    values = id_values(hard["vid"], "seven")
    opened = [walk]
    try:
        for cols in ([2], [0, 2], [2, 1, 0]):
            oh = len(cols) - 1
            rows, _, _ = D.distinct_rows(hard["walks"][2], cols)
            _, out = gg.distinct(walk, 2, cols)
            opened.append(out)
            assert np.array_equal(fetch_all(out, oh), rows)
            assert out.digest(csr, oh) == (rows.shape[0], F.digest_dense_rows(X.dense_rows(g.index, rows)))
            for col in range(oh + 1):
                want_rows, _, want = R.filter_rows(rows, None, col, hard["vid"], values, None, -1, 1, "in")
                fst, kept = gg.filter_value(out, oh, col, csr, values, None, -1, 1)
                opened.append(kept)
                assert fst == want and np.array_equal(fetch_all(kept, oh), want_rows)
                assert cols[col] == 0 or 0 < fst["rows_out"] < fst["rows_in"]  # (v0 holds the four sources only)
                top_rows, _, twant = R.top_rows(rows, None, col, hard["vid"], values, None, -2, 3, "in", True, 0, 7)
                tst, top = gg.top_rows(out, oh, col, csr, values, 7, None, -2, 3, "in", True, 0)
                opened.append(top)
                assert tst["candidates"] == twant["candidates"] and np.array_equal(fetch_all(top, oh), top_rows)
            for mode in ("inner", "semi", "anti"):  # from column 0 to the last: a self-loop test on table 0
                want_rows, want = F.filter_rows(rows, g.A, g.index, 0, oh, mode)
                est, kept = gg.filter_edge(out, oh, csr, 0, oh, mode)
                opened.append(kept)
                assert est == want and np.array_equal(fetch_all(kept, oh), want_rows)
            assert est["rows_out"] < est["rows_in"]
            agg = gg.group_by(out, oh, oh, csr)
            opened.append(agg)
            assert K.same(agg.fetch(oh), G.group_by(rows, oh, hard["vid"])[0])
            if oh == 0:  # the common-neighbour filter of a one-column table: a row per out-neighbour
                made = C.c_void_p()
                assert gg.lib.gg_result_filter_common_neighbour(gg.ctx, out.handle, 0, csr.handle, C.byref(made)) == 0
                longer = KhopResult(gg, made, None)
                opened.append(longer)
                assert longer.rows(1) == int(np.diff(g.off)[[g.index[int(p)] for p in rows[:, 0].tolist()]].sum())
    finally:
        for o in reversed(opened):
            o.close()
        csr.close()


def test_filtered_top_and_triangle_tables_are_inputs_like_any_other(gg, hard):
    w = World(gg, hard, "mid")
    try:
        values = id_values(w.ext_ids, "seven")
        kept_rows, _, _ = R.filter_rows(w.rows, None, w.hops, w.ext_ids, values, None, -1, 1, "in")
        _, kept = gg.filter_value(w.table, w.hops, w.hops, w.ext_csr, values, None, -1, 1)
        w.own(kept)
        top_rows, _, _ = R.top_rows(w.rows, None, w.hops, w.ext_ids, values, None, -2, 2, "in", True, w.hops, 3000)
        _, top = gg.top_rows(w.table, w.hops, w.hops, w.ext_csr, values, 3000, None, -2, 2, "in", True, w.hops)
        w.own(top)
        sst, semi = gg.filter_edge(w.table, w.hops, w.csr, 1, 0, "semi")
        w.own(semi)
        semi_rows = F.filter_rows(w.rows, hard["g"].A, hard["g"].index, 1, 0, "semi")[0]
        for res, rows in ((kept, kept_rows), (top, top_rows), (semi, semi_rows)):
            assert rows.shape[0] > 256
            for cols in ([3], [0, 3], [1, 2], [3, 0, 1, 2]):
                check(gg, res, w.hops, rows, cols)
        tst, tri = gg.triangles_edges(w.csr, hard["S"])
        w.own(tri)
        tri_rows = fetch_all(tri, 2)
        assert tri_rows.shape[0] > 0 and tri.fetch_triangle_edges(0).shape[1] == 3
        for cols in ([0, 1, 2], [2, 0]):
            _, out = gg.distinct(tri, 2, cols)
            w.own(out)
            assert np.array_equal(fetch_all(out, len(cols) - 1), D.distinct_rows(tri_rows, cols)[0])
            bufs = (C.POINTER(C.c_int64) * 3)(*[np.zeros(8, np.int64).ctypes.data_as(C.POINTER(C.c_int64)) for _ in range(3)])
            assert gg.lib.gg_triangles_fetch_edges(out.handle, 0, 8, bufs, C.byref(C.c_uint32())) == GG_ERR_STATE
    finally:
        w.close()


def test_degenerate_shapes(gg):
    vid = np.array([10, 20, 30], np.int64)
    csr = build(gg, vid, np.array([10, 20], np.int64), np.array([20, 10], np.int64))
    empty = gg.expand_khop_result(csr, 2, np.empty(0, np.int64))
    try:
        for cols in ([0], [2, 0], [0, 1, 2]):
            oh = len(cols) - 1
            st, out = gg.distinct(empty, 2, cols)
            assert st == {"rows_in": 0, "rows_out": 0, "slots": 0, "probe_steps": 0}
            assert out.handle and out.rows(oh) == 0 and fetch_all(out, oh).shape == (0, oh + 1)
            st2, again = gg.distinct(out, oh, list(range(oh + 1)))  # an empty result is an input like any other
            assert st2 == st and again.rows(oh) == 0
            again.close()
            out.close()
            assert gg.distinct(empty, 2, cols, materialise=False) == st
        st = DistinctStats()  # stats may be NULL when materialising
        made = C.c_void_p()
        cols = (C.c_int * 1)(1)
        two = gg.expand_khop_result(csr, 1, None)
        assert gg.lib.gg_result_distinct(gg.ctx, two.handle, 1, cols, 1, 1, None, C.byref(made)) == 0
        assert sorted(fetch_all(KhopResult(gg, made, None), 0)[:, 0].tolist()) == [10, 20]
        gg.lib.gg_result_destroy(made)
        two.close()
    finally:
        empty.close()
        csr.close()


def test_count_only_equals_the_materialised_stats_but_for_the_probe_steps(gg, hard):
    w = World(gg, hard, "big")
    try:
        for cols in ([3], [0, 3], [0, 1, 2, 3]):
            only = gg.distinct(w.table, w.hops, cols, materialise=False)
            st, out = gg.distinct(w.table, w.hops, cols)
            out.close()
            assert {k: v for k, v in only.items() if k != "probe_steps"} == {k: v for k, v in st.items() if k != "probe_steps"}
            assert only["rows_out"] == D.distinct_rows(w.rows, cols)[2]["rows_out"]
        st = DistinctStats()  # count mode takes a NULL out_result
        cols = (C.c_int * 1)(3)
        assert gg.lib.gg_result_distinct(gg.ctx, w.table.handle, w.hops, cols, 1, 0, C.byref(st), None) == 0
        assert int(st.rows_out) == 2937
    finally:
        w.close()


def test_errors_leave_the_context_usable(gg, hard):
    from tests import test_gpu_result_kinds as RK

    vid, src, dst, S = hard["vid"], hard["src"], hard["dst"], hard["S"]
    csr = build(gg, vid, src, dst)
    table = gg.expand_khop_result(csr, 2, S)
    other = type(gg)(0)
    other.append_vertices(vid[:4])
    other.append_edges(vid[:2], vid[2:4])
    foreign = other.build_csr()
    foreign_table = other.expand_khop_result(foreign, 1, None)
    want = D.distinct_rows(hard["walks"][2], [2, 0])

    def call(res, hops, cols, n=None, materialise=1, stats=True, out=True, ctx=None):
        st, o = DistinctStats(), C.c_void_p(1)
        arr = None if cols is None else (C.c_int * max(len(cols), 1))(*cols)
        rc = gg.lib.gg_result_distinct(ctx or gg.ctx, res, hops, arr, len(cols or []) if n is None else n, materialise,
                                       C.byref(st) if stats else None, C.byref(o) if out else None)
        assert rc != 0 and (not out or not o.value)
        return rc

    kinds_csr = build(gg, RK.VID, RK.SRC, RK.DST, RK.ROWID)
    kinds = {}
    try:
        RK.make_results(gg, kinds_csr, kinds)
        bad = [
            (call(None, 2, [0]), GG_ERR_INVALID_ARG),
            (call(table.handle, 2, None, n=1), GG_ERR_INVALID_ARG),                      # NULL cols
            (call(table.handle, 2, [0], ctx=other.ctx), GG_ERR_INVALID_ARG),             # a result of another context
            (call(foreign_table.handle, 1, [0]), GG_ERR_INVALID_ARG),
            (call(table.handle, 3, [0]), GG_ERR_INVALID_ARG),                            # hops outside the result's levels
            (call(table.handle, 1, [0]), GG_ERR_INVALID_ARG),
            (call(table.handle, -1, [0]), GG_ERR_INVALID_ARG),
            (call(table.handle, 2, [0], n=0), GG_ERR_INVALID_ARG),                       # n_cols outside 1..hops + 1
            (call(table.handle, 2, [0, 1, 2, 0], n=4), GG_ERR_INVALID_ARG),
            (call(table.handle, 2, [0], n=-1), GG_ERR_INVALID_ARG),
            (call(table.handle, 2, [3]), GG_ERR_INVALID_ARG),                            # a column outside 0..hops
            (call(table.handle, 2, [0, -1]), GG_ERR_INVALID_ARG),
            (call(table.handle, 2, [1, 1]), GG_ERR_INVALID_ARG),                         # a repeated column
            (call(table.handle, 2, [2, 0, 2]), GG_ERR_INVALID_ARG),
            (call(table.handle, 2, [0], out=False), GG_ERR_INVALID_ARG),                 # materialise without out_result
            (call(table.handle, 2, [0], materialise=0, stats=False, out=False), GG_ERR_INVALID_ARG),  # nothing asked for
        ]
        for name in ("closure", "reach", "levels", "paths"):          # the older kinds refuse one another so
            bad.append((call(kinds[name], RK.HOPS, [0]), GG_ERR_INVALID_ARG))
        for name in ("agg", "top", "pairs", "comps", "all_paths"):    # the kinds with a refusal contract
            bad.append((call(kinds[name], RK.HOPS, [0]), GG_ERR_STATE))
        for i, (rc, code) in enumerate(bad):
            assert rc == code, (i, rc, code)
        for i in range(len(bad)):  # a correct call still works, as often as an error came before it
            if i % 8 == 0:
                st, out = gg.distinct(table, 2, [2, 0])
                assert np.array_equal(fetch_all(out, 1), want[0])
                out.close()
        assert gg.lib.gg_debug_distinct(gg.ctx, 0, 2) == GG_ERR_INVALID_ARG and gg.lib.gg_debug_distinct(gg.ctx, 0, -1) == GG_ERR_INVALID_ARG
        # the walk tables of every origin are answered
        for name in ("walk", "walk_edges", "tri", "tri_edges"):
            rows = fetch_all(KhopResult(gg, kinds[name], None), RK.HOPS)
            st, out = gg.distinct(KhopResult(gg, kinds[name], None), RK.HOPS, [2, 0])
            assert np.array_equal(fetch_all(out, 1), D.distinct_rows(rows, [2, 0])[0]) and st["rows_in"] > 0
            out.close()
    finally:
        for res in kinds.values():
            gg.lib.gg_result_destroy(res)
        kinds_csr.close()
        foreign_table.close()
        foreign.close()
        other.close()
        table.close()
        csr.close()
