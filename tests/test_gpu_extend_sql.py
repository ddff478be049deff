"""gg_khop_extend / gg_khop_extend_count inside the compiled reference, with the reference's own hash-join plans of the
same statements over the same tables as the yardstick (no planner rule is on: the joins run as the reference plans
them): knows joined with message on the friend (interactive-complex-2's shape), friends of friends and their messages
(interactive-complex-9's subquery), and a branch off the middle column of a 2-hop walk."""
import os

import numpy as np
import pytest

from oracle import ref_duckdb as R
from tests import edge_filter_ref as F
from tests import extend_ref as X
from tests import triangles_ref as T
from tests.oracle_lib import sort_rows

EXT = R.EXTENSION

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not (R.available() and os.path.exists(EXT)), reason="reference build / extension not present"),
]

GRAPH = "'person', 'p_personid', 'knows', 'k_person1id', 'k_person2id'"
MESSAGE = "'message', 'm_creatorid', 'm_messageid'"


@pytest.fixture(scope="module")
def db():
    vid, src, dst = T.hard_graph()
    g = T.TriangleGraph(vid, src, dst)
    es, ed, er, info = X.ext_table(g)
    d = R.RefDuckDB(threads=4)
    d.load_ldbc(vid, src, dst)
    d.load_table("message", {"m_messageid": ed, "m_creatorid": es})  # (its rowids are the append positions)
    d.execute(f"LOAD '{EXT}'")
    # a person who knows the hub (so 1-hop walks end in it), the hub, z, and a person of a few messages
    knows_hub = int(g.vid[g.su[g.dv == g.index[info["hub"]]][0]])
    light = int(es[(es != info["hub"]) & np.isin(es, g.vid)][0])
    some = np.unique(np.array([knows_hub, info["hub"], info["z"], light], np.int64))
    assert some.size == 4
    yield d, g, (es, ed), some
    d.close()


def in_list(ids):
    return "'SELECT p_personid FROM person WHERE p_personid IN (" + ", ".join(str(int(s)) for s in ids) + ")'"


def both(d, sources_sql, hops, fc):
    """(the function's rows, its count row)"""
    args = f"{GRAPH}, {sources_sql}, {hops}, {MESSAGE}, {fc}"
    cols = ", ".join(f"v{c}" for c in range(hops + 1)) + ", w, ext_rowid"
    rows = d.execute(f"SELECT {cols} FROM gg_khop_extend({args})")
    count = d.execute(f"SELECT rows, walks, matched FROM gg_khop_extend_count({args})")
    assert count.shape == (1, 3)
    assert int(d.execute(f"SELECT count(*) FROM gg_khop_extend({args})")[0, 0]) == rows.shape[0] == int(count[0, 0])
    return rows, count[0]


def check_count(count, g, ext, sources, hops, fc, want_rows):
    es, ed = ext
    st = X.extend_rows(g.vid[F.walks(g, sources, hops)], es, ed, None, fc)[2]
    assert [int(c) for c in count] == [want_rows, st["rows_in"], st["rows_matched"]] and st["rows_out"] == want_rows


def test_knows_joined_with_message_on_the_friend(db):
    """interactive-complex-2.sql:2-7"""
    d, g, ext, some = db
    ids = ", ".join(str(int(s)) for s in some)
    want = d.execute("SELECT k.k_person1id, k.k_person2id, m.m_messageid, m.rowid FROM knows k, message m "
                     f"WHERE k.k_person1id IN ({ids}) AND m.m_creatorid = k.k_person2id")
    rows, count = both(d, in_list(some), 1, 1)
    assert want.shape[0] >= X.HUB_ROWS and np.array_equal(sort_rows(rows), sort_rows(want))
    check_count(count, g, ext, some, 1, 1, want.shape[0])
    # the rowid fetches the row: its key is the friend, its next the message
    es, ed = ext
    assert np.array_equal(es[rows[:, 3]], rows[:, 1]) and np.array_equal(ed[rows[:, 3]], rows[:, 2])


def test_friends_of_friends_and_their_messages(db):
    """the 2-hop arm of interactive-complex-9.sql:13-15"""
    d, g, ext, some = db
    want = d.execute(X.sql_extend(2, 2, some))
    rows, count = both(d, in_list(some), 2, 2)
    assert want.shape[0] > 0 and np.array_equal(sort_rows(rows), sort_rows(want))
    check_count(count, g, ext, some, 2, 2, int(d.execute(X.sql_extend(2, 2, some, "count(*)"))[0, 0]))


@pytest.mark.parametrize("from_col", [1, 0])
def test_a_branch_off_an_earlier_column_of_a_two_hop_walk(db, from_col):
    """interactive-complex-5.sql:15 joins on a middle column, not the walk's end"""
    d, g, ext, some = db
    want = d.execute(X.sql_extend(2, from_col, some))
    rows, count = both(d, in_list(some), 2, from_col)
    assert want.shape[0] > 0 and np.array_equal(sort_rows(rows), sort_rows(want))
    check_count(count, g, ext, some, 2, from_col, want.shape[0])


@pytest.mark.parametrize("all_sources", ["NULL", "''"])
def test_every_vertex_is_a_source(db, all_sources):
    d, g, ext, some = db
    want = d.execute(X.sql_extend(1, 1, None))
    rows, count = both(d, all_sources, 1, 1)
    assert want.shape[0] > 0 and np.array_equal(sort_rows(rows), sort_rows(want))


def test_bad_arguments_raise_and_the_connection_stays_usable(db):
    d, g, ext, some = db
    s = in_list(some)
    bad = [
        f"{GRAPH}, {s}, 1, 'message', 'no_such_column', 'm_messageid', 1",  # a missing column
        f"{GRAPH}, {s}, 1, 'no_such_table', 'm_creatorid', 'm_messageid', 1",
        f"{GRAPH}, {s}, 1, {MESSAGE}, 2",    # a column outside 0..hops
        f"{GRAPH}, {s}, 1, {MESSAGE}, -1",
        f"{GRAPH}, {s}, 0, {MESSAGE}, 0",    # hops outside 1..GG_MAX_HOPS - 1
        f"{GRAPH}, {s}, 8, {MESSAGE}, 0",
        f"{GRAPH}, {s}, 1, {MESSAGE}, NULL",
    ]
    for args in bad:
        for fn in ("gg_khop_extend", "gg_khop_extend_count"):
            with pytest.raises(RuntimeError):
                d.execute(f"SELECT * FROM {fn}({args})")
    rows, count = both(d, s, 1, 1)
    assert rows.shape[0] == d.execute(X.sql_extend(1, 1, some)).shape[0] > 0
