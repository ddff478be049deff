"""The numpy restatements of the walk-row operators at full width (7- and 8-hop tables: 8 and 9 id columns), each against
a plain python-loop form, before tests/test_gpu_wide_rows.py takes them as the yardstick of the device kernels; and the
facts about the inputs that file relies on (tests/wide_rows_ref.py, deep_graphs.ext_table)."""
import numpy as np
import pytest

from tests import deep_graphs as D
from tests import edge_filter_ref as F
from tests import extend_ref as X
from tests import group_by_ref as G
from tests import khop_aggregate_ref as K
from tests import value_rows_ref as R
from tests import wide_rows_ref as W

LO, HI = R.I64_MIN, R.I64_MAX
TABLES = [("cycle_chords", 7, None), ("cycle_chords", 8, None), ("multigraph", 8, slice(1000, 1200))]


def table_of(name, hops, part):
    rows = W.walk_rows(name, hops)
    return rows if part is None else rows[part]


@pytest.mark.parametrize("name", D.SMALL)
def test_row_counts_of_the_walk_tables(name):
    vid, src, dst, g, S = W.world(name)
    assert g.V == vid.size and g.su.size == W.KEPT_EDGE_ROWS[name]
    assert np.unique(S).size < S.size and not np.isin(S[-2:], vid).any()  # repeats, and two ids that are no vertex
    assert [W.walk_rows(name, h).shape[0] for h in range(1, 9)] == W.ROWS[name]
    assert all(W.walk_rows(name, h).shape[1] == h + 1 for h in range(1, 9))


@pytest.mark.parametrize("name", ["multigraph", "cycle_chords"])
def test_the_closing_condition_is_selective_at_every_depth(name):
    """v_0 -> v_h over the walk graph: some rows match at 4, 6, 7 and 8 hops, not all, and on the multigraph a row twice"""
    vid, src, dst, g, S = W.world(name)
    want = {"multigraph": [6, 33, 85, 100], "cycle_chords": [10, 34, 73, 130]}[name]
    ms = [F.multiplicity(W.walk_rows(name, h), g.A, g.index, 0, h) for h in (4, 6, 7, 8)]
    assert [int((m > 0).sum()) for m in ms] == want
    if name == "multigraph":
        assert max(int(m.max()) for m in ms) == 2


def test_the_hub_shape_has_a_pair_that_matches_nothing_and_one_that_is_selective():
    vid, src, dst, g, S = W.world("hub")
    for h in (6, 8):
        rows = W.walk_rows("hub", h)
        assert not F.multiplicity(rows, g.A, g.index, 0, h).any()
        assert 0 < int((F.multiplicity(rows, g.A, g.index, 1, h) > 0).sum()) < rows.shape[0]


@pytest.mark.parametrize("name", D.SMALL)
def test_the_second_edge_table_is_joined_on_every_shape_with_deep_walks(name):
    """(the generator asserts the table's own facts) the long key stands in column 0 of every table of 4 to 7 hops that has
    rows, so its EXT_HUB_ROWS + 5 rows are joined there; every output stays under 20 000 rows"""
    vid, src, dst, g, S = W.world(name)
    es, ed, er, info = D.ext_table(name)
    assert np.isin(info["hub"], vid) and not np.isin(ed[ed >= info["base"]], vid).any()
    for h in (4, 5, 6, 7):
        rows = W.walk_rows(name, h)
        for fc in (0, 3, h):
            st = X.extend_rows(rows, es, ed, er, fc)[2]
            assert st["rows_out"] < 20_000
            if rows.shape[0]:
                assert 0 < st["rows_matched"] < st["rows_in"]
        if rows.shape[0]:
            assert (rows[:, 0] == info["hub"]).any()


@pytest.mark.parametrize("name,hops,part", TABLES)
def test_extend_rows_equals_the_loops(name, hops, part):
    table = table_of(name, hops, part)
    es, ed, er, _ = D.ext_table(name)
    for fc in (0, 3, hops):
        for rowid in (er, None):
            a, b = X.extend_rows(table, es, ed, rowid, fc), X.extend_rows_brute(table, es, ed, rowid, fc)
            assert a[0].shape[1] == hops + 2 and a[2]["rows_out"] > 0
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


@pytest.mark.parametrize("name,hops,part", TABLES)
def test_group_by_equals_the_loops(name, hops, part):
    table = table_of(name, hops, part)
    vid = W.world(name)[0]
    w = G.hub_weights(vid, int(table[0, 4]))
    for kc in (0, 4, hops):
        for wc in (None, 0, 4, hops):
            a = G.group_by(table, kc, vid, wc, None, None if wc is None else w)
            b = G.group_by_brute(table, kc, vid, wc, None, None if wc is None else w)
            assert K.same(a[0], b[0]) and a[1] == b[1] and a[1]["groups"] > 0


@pytest.mark.parametrize("name,hops,part", TABLES)
def test_filter_and_top_rows_equal_the_loops(name, hops, part):
    table = table_of(name, hops, part)
    vid = W.world(name)[0]
    edges = np.arange(table.shape[0] * hops, dtype=np.int64).reshape(-1, hops) * 3 - 7
    seven = (np.arange(vid.size, dtype=np.int64) * 5) % 7 - 3
    valid = R.pack_valid(np.arange(vid.size) % 5 != 2)
    for col in (0, hops):
        for bits in (None, valid):
            for lo, hi in ((LO, HI), (-1, 1), (1, -1)):
                for mode in ("in", "not_in"):
                    a = R.filter_rows(table, edges, col, vid, seven, bits, lo, hi, mode)
                    b = R.filter_rows_loop(table, edges, col, vid, seven, bits, lo, hi, mode)
                    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
                    for tie in (None, 0, hops):
                        for desc in (True, False):
                            for n in (0, 1, 100, table.shape[0] + 1):
                                a = R.top_rows(table, edges, col, vid, seven, bits, lo, hi, mode, desc, tie, n)
                                b = R.top_rows_loop(table, edges, col, vid, seven, bits, lo, hi, mode, desc, tie, n)
                                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


@pytest.mark.parametrize("name,hops,part", TABLES)
def test_edge_filter_rows_equal_a_two_loop_count(name, hops, part):
    table = table_of(name, hops, part)
    vid, src, dst, g, S = W.world(name)
    known = set(vid.tolist())
    pairs = [(a, b) for a, b in zip(src.tolist(), dst.tolist()) if a in known and b in known]
    some = False
    for fc, tc in W.column_pairs(hops):
        m = []
        for r in table.tolist():
            n = 0
            for a, b in pairs:
                n += a == r[fc] and b == r[tc]
            m.append(n)
        m = np.array(m, np.int64)
        assert np.array_equal(F.multiplicity(table, g.A, g.index, fc, tc), m)
        some = some or 0 < int((m > 0).sum()) < m.size
        want = {"inner": np.repeat(table, m, axis=0), "semi": table[m > 0], "anti": table[m == 0]}
        for mode in F.MODES:
            rows, st = F.filter_graph(g, table, fc, tc, mode)
            assert np.array_equal(rows, want[mode])
            assert st == {"rows_in": table.shape[0], "rows_out": want[mode].shape[0], "matches": int(m.sum())}
    assert some
