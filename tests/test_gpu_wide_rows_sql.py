"""The table functions over walk rows at their widest inside the compiled reference — gg_khop_extend, _count, _group,
_filter, _filter_count and _top at 7 hops (9 id columns, w among them, and ext_rowid), gg_khop_edge_filter and _count at 8
hops (v0..v8) — with the reference's own plans of the same joins over the same tables as the yardstick (no planner rule is
on).  The tables are the cycle_chords shape of tests/deep_graphs.py and deep_graphs.ext_table as message; sorted rows are
compared."""
import os

import numpy as np
import pytest

from oracle import ref_duckdb as R
from tests import deep_graphs as D
from tests import edge_filter_ref as F
from tests import extend_ref as X
from tests import group_by_ref as G
from tests import wide_rows_ref as W
from tests.oracle_lib import sort_rows
from tests.test_gpu_value_rows_sql import date_of

EXT = R.EXTENSION

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not (R.available() and os.path.exists(EXT)), reason="reference build / extension not present"),
]

GRAPH = "'person', 'p_personid', 'knows', 'k_person1id', 'k_person2id'"
MESSAGE = "'message', 'm_creatorid', 'm_messageid'"
NAME = "cycle_chords"


@pytest.fixture(scope="module")
def db():
    vid, src, dst, g, S = W.world(NAME)
    es, ed, er, info = D.ext_table(NAME)
    d = R.RefDuckDB(threads=4)
    d.load_ldbc(vid, src, dst)
    d.load_table("message", {"m_messageid": ed, "m_creatorid": es, "m_creationdate": date_of(ed)})  # rowid: append position
    d.execute(f"LOAD '{EXT}'")
    some = np.unique(S[np.isin(S, vid)])  # the statements take distinct sources
    assert info["hub"] in some.tolist()
    yield d, g, (es, ed), some
    d.close()


def in_list(ids):
    return "'SELECT p_personid FROM person WHERE p_personid IN (" + ", ".join(str(int(s)) for s in ids) + ")'"


def id_cols(hops):
    return ", ".join(f"v{c}" for c in range(hops + 1)) + ", w, ext_rowid"


def select_all(hops):
    return ", ".join(f"p{c}.p_personid" for c in range(hops + 1)) + ", m.m_messageid, m.rowid"


@pytest.mark.parametrize("from_col", [0, 3, 7])
def test_extend_and_its_count_at_seven_hops(db, from_col):
    d, g, (es, ed), some = db
    args = f"{GRAPH}, {in_list(some)}, 7, {MESSAGE}, {from_col}"
    want = d.execute(X.sql_extend(7, from_col, some))
    rows = d.execute(f"SELECT {id_cols(7)} FROM gg_khop_extend({args})")
    assert want.shape[0] > 0 and rows.shape[1] == 10 and np.array_equal(sort_rows(rows), sort_rows(want))
    assert d.execute(f"SELECT * FROM gg_khop_extend({args})").shape == rows.shape  # v0..v7, w, ext_rowid and nothing else
    assert from_col or want.shape[0] > D.EXT_HUB_ROWS
    # the rowid fetches the row: its key is the cell of from_col, its next the new column
    assert np.array_equal(es[rows[:, 9]], rows[:, from_col]) and np.array_equal(ed[rows[:, 9]], rows[:, 8])
    count = d.execute(f"SELECT rows, walks, matched FROM gg_khop_extend_count({args})")
    st = X.extend_rows(g.vid[F.walks(g, some, 7)], es, ed, None, from_col)[2]
    assert count.tolist() == [[want.shape[0], st["rows_in"], st["rows_matched"]]] and st["rows_out"] == want.shape[0]


@pytest.mark.parametrize("from_col,key_col", [(0, 8), (7, 0), (7, 7), (3, 8)])
def test_extend_group_at_seven_hops(db, from_col, key_col):
    d, g, ext, some = db
    every = d.execute(G.sql_extend_group(7, from_col, key_col, some))
    assert every.shape[0] > 1
    for n in (None, 1, 10, every.shape[0] + 7):
        want = d.execute(G.sql_extend_group(7, from_col, key_col, some, n))
        rows = d.execute(f"SELECT rank, key, rows FROM gg_khop_extend_group({GRAPH}, {in_list(some)}, 7, {MESSAGE}, {from_col}, "
                         f"{key_col}, {'NULL' if n is None else n})")
        assert np.array_equal(rows[:, 0], np.arange(rows.shape[0]))
        assert np.array_equal(rows[:, 1:], want), (from_col, key_col, n)


@pytest.mark.parametrize("from_col,value_col", [(0, 8), (7, 8), (7, 0)])
def test_extend_filter_and_its_count_at_seven_hops(db, from_col, value_col):
    d, g, ext, some = db
    base = X.sql_extend(7, from_col, some, select_all(7))
    everything = int(d.execute(X.sql_extend(7, from_col, some, "count(*)"))[0, 0])
    if value_col == 8:
        lo, hi = 200, 600
        column, cell = "'m_creationdate'", "m.m_creationdate"
    else:  # a value of the walk's own column: the person's id
        s = np.sort(d.execute(X.sql_extend(7, from_col, some, f"p{value_col}.p_personid"))[:, 0])
        lo, hi = int(s[s.size // 4]), int(s[s.size // 2])
        column, cell = "'p_personid'", f"p{value_col}.p_personid"
    args = f"{GRAPH}, {in_list(some)}, 7, {MESSAGE}, {from_col}, {column}, {value_col}, {lo}, {hi}"
    want = d.execute(base + f" AND {cell} >= {lo} AND {cell} <= {hi}")
    rows = d.execute(f"SELECT {id_cols(7)} FROM gg_khop_extend_filter({args}, false)")
    assert 0 < want.shape[0] < everything and np.array_equal(sort_rows(rows), sort_rows(want))
    count = d.execute(f"SELECT rows, walks, valued FROM gg_khop_extend_filter_count({args}, false)")
    assert count.tolist() == [[want.shape[0], everything, everything]]
    outside = d.execute(f"SELECT {id_cols(7)} FROM gg_khop_extend_filter({args}, true)")
    want_outside = d.execute(base + f" AND NOT ({cell} >= {lo} AND {cell} <= {hi})")
    assert np.array_equal(sort_rows(outside), sort_rows(want_outside)) and rows.shape[0] + outside.shape[0] == everything


@pytest.mark.parametrize("from_col", [0, 7])
@pytest.mark.parametrize("descending", [True, False])
def test_extend_top_at_seven_hops(db, from_col, descending):
    """ORDER BY m_creationdate, m_messageid: SQL leaves the rows of one (date, message) unordered, so whole rows are
    compared after a sort for n at the end of such a group, and the messages in order"""
    d, g, ext, some = db
    below = 700
    ref = d.execute(X.sql_extend(7, from_col, some, select_all(7) + ", m.m_creationdate")
                    + f" AND m.m_creationdate < {below} ORDER BY m.m_creationdate {'DESC' if descending else 'ASC'}, "
                    "m.m_messageid ASC")
    total = ref.shape[0]
    key = ref[:, [10, 8]]
    ends = np.nonzero((key[1:] != key[:-1]).any(axis=1))[0] + 1
    assert total > 20 and ends.size >= 3
    for n in (0, int(ends[0]), int(ends[ends.size // 2]), total, total + 7, "NULL"):
        args = (f"{GRAPH}, {in_list(some)}, 7, {MESSAGE}, {from_col}, 'm_creationdate', 8, NULL, {below - 1}, false, "
                f"{'true' if descending else 'false'}, 8, {n}")
        rows = d.execute(f"SELECT rank, {id_cols(7)} FROM gg_khop_extend_top({args})")
        m = total if n == "NULL" else min(n, total)
        assert rows.shape == (m, 11) and np.array_equal(rows[:, 0], np.arange(m))
        assert np.array_equal(sort_rows(rows[:, 1:]), sort_rows(ref[:m, :10])), (from_col, n)
        assert np.array_equal(rows[:, 9], ref[:m, 8]), (from_col, n)


@pytest.mark.parametrize("from_col,to_col", [(0, 8), (8, 0), (1, 7), (7, 8)])
def test_edge_filter_and_its_count_at_eight_hops(db, from_col, to_col):
    d, g, ext, some = db
    walks = F.walks(g, some, 8).shape[0]
    cols = ", ".join(f"v{c}" for c in range(9))
    seen = {}
    for mode, negate in (("semi", False), ("anti", True)):
        args = f"{GRAPH}, {in_list(some)}, 8, {from_col}, {to_col}, '{mode}'"
        want = d.execute(F.sql_exists(8, from_col, to_col, negate, some))
        rows = d.execute(f"SELECT {cols} FROM gg_khop_edge_filter({args})")
        assert rows.shape[1] == 9 and np.array_equal(sort_rows(rows), sort_rows(want)), mode
        assert d.execute(f"SELECT * FROM gg_khop_edge_filter({args})").shape == rows.shape  # v0..v8 and nothing else
        count = d.execute(f"SELECT rows, walks, matches FROM gg_khop_edge_filter_count({args})")
        assert count.shape == (1, 3) and [int(count[0, 0]), int(count[0, 1])] == [want.shape[0], walks]
        seen[mode] = want.shape[0]
    assert seen["semi"] + seen["anti"] == walks and seen["semi"] > 0
    # inner: one row per matching edge row
    args = f"{GRAPH}, {in_list(some)}, 8, {from_col}, {to_col}, 'inner'"
    rows = d.execute(f"SELECT {cols} FROM gg_khop_edge_filter({args})")
    want_rows = F.filter_graph(g, g.vid[F.walks(g, some, 8)], from_col, to_col, "inner")[0]
    assert np.array_equal(sort_rows(rows), sort_rows(want_rows)) and rows.shape[0] >= seen["semi"]
