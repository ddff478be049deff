"""gg_khop_extend_filter / gg_khop_extend_filter_count / gg_khop_extend_top inside the compiled reference, with the
reference's own plans of the same statements over the same tables as the yardstick (no planner rule is on): the tails of
interactive-complex-2 and -9 (`m_creationdate < X ORDER BY m_creationdate DESC, m_messageid LIMIT n` above knows -> message
and knows -> knows -> message) and interactive-complex-4's half-open date range as filter and count.

message carries m_creationdate = DATE_OF(m_messageid), so many messages share a date, and one message is reached over many
walks.  SQL leaves ties in (date, message) unordered; the function breaks them by input row.  So for n at a boundary between
tie groups whole rows are compared after a full sort, and for an n that cuts a tie group only the (date, message) columns,
in order.  The boundaries come from the reference's complete ordered output."""
import os

import numpy as np
import pytest

from oracle import ref_duckdb as R
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
DATES = 1009


def date_of(message_ids):
    """the stored date of a message: (id * 7919) mod 1009, the one negative id of ext_table set apart"""
    m = np.asarray(message_ids, np.int64)
    return np.where(m < 0, -5, (m * 7919) % DATES).astype(np.int64)


@pytest.fixture(scope="module")
def db():
    vid, src, dst = T.hard_graph()
    g = T.TriangleGraph(vid, src, dst)
    es, ed, er, info = X.ext_table(g)
    d = R.RefDuckDB(threads=4)
    d.load_ldbc(vid, src, dst)
    d.load_table("message", {"m_messageid": ed, "m_creatorid": es, "m_creationdate": date_of(ed)})
    d.execute(f"LOAD '{EXT}'")
    knows_hub = int(g.vid[g.su[g.dv == g.index[info["hub"]]][0]])
    light = int(es[(es != info["hub"]) & np.isin(es, g.vid)][0])
    some = np.unique(np.array([knows_hub, info["hub"], info["z"], light], np.int64))
    assert some.size == 4
    yield d, g, (es, ed), some
    d.close()


def in_list(ids):
    return "'SELECT p_personid FROM person WHERE p_personid IN (" + ", ".join(str(int(s)) for s in ids) + ")'"


def id_cols(hops):
    return ", ".join(f"v{c}" for c in range(hops + 1)) + ", w, ext_rowid"


def ordered_reference(d, hops, fc, some, below, descending=True):
    """the reference's complete answer in order: rows (v0..vh, m_messageid, m.rowid, m_creationdate)"""
    select = ", ".join(f"p{c}.p_personid" for c in range(hops + 1)) + ", m.m_messageid, m.rowid, m.m_creationdate"
    return d.execute(X.sql_extend(hops, fc, some, select) + f" AND m.m_creationdate < {below} ORDER BY m.m_creationdate "
                     + ("DESC" if descending else "ASC") + ", m.m_messageid ASC")


def top(d, hops, fc, some, below, n, descending=True, table=MESSAGE):
    args = (f"{GRAPH}, {in_list(some)}, {hops}, {table}, {fc}, 'm_creationdate', {hops + 1}, NULL, {below - 1}, false, "
            f"{'true' if descending else 'false'}, {hops + 1}, {n}")
    rows = d.execute(f"SELECT rank, {id_cols(hops)} FROM gg_khop_extend_top({args})")
    assert np.array_equal(rows[:, 0], np.arange(rows.shape[0]))  # rows leave in rank order
    return rows[:, 1:]


def check_tail(d, hops, fc, some, below):
    """LIMIT n for n at tie-group boundaries (whole rows) and inside a tie group (date and message only)"""
    ref = ordered_reference(d, hops, fc, some, below)
    total = ref.shape[0]
    key = ref[:, [hops + 3, hops + 1]]  # (date, message)
    assert np.array_equal(date_of(ref[:, hops + 1]), ref[:, hops + 3])
    change = np.nonzero((key[1:] != key[:-1]).any(axis=1))[0] + 1  # n at which a tie group ends
    inside = np.setdiff1d(np.arange(1, total), change)
    assert total > 1024 and change.size >= 3 and inside.size >= 1
    boundaries = [int(change[0]), int(change[change.size // 2]), int(change[np.searchsorted(change, 20)]), total, total + 7]
    for n in boundaries:
        got = top(d, hops, fc, some, below, n)
        m = min(n, total)
        assert got.shape[0] == m
        assert np.array_equal(sort_rows(got), sort_rows(ref[:m, : hops + 3]))
        assert np.array_equal(got[:, hops + 1], ref[:m, hops + 1])  # and the messages stand in the reference's order
    cut = int(inside[inside.size // 2])
    got = top(d, hops, fc, some, below, cut)
    assert got.shape[0] == cut
    assert np.array_equal(got[:, hops + 1], ref[:cut, hops + 1])
    assert np.array_equal(date_of(got[:, hops + 1]), ref[:cut, hops + 3])
    # what the cut leaves open is which of the tied rows: all of them are rows of the tie group
    group = ref[(key == key[cut - 1]).all(axis=1)][:, : hops + 3]
    tail = got[(date_of(got[:, hops + 1]) == key[cut - 1, 0]) & (got[:, hops + 1] == key[cut - 1, 1])]
    assert tail.shape[0] > 0 and set(map(tuple, tail.tolist())) <= set(map(tuple, group.tolist()))
    assert top(d, hops, fc, some, below, 0).shape == (0, hops + 3)
    # ascending, every row (n NULL)
    asc = ordered_reference(d, hops, fc, some, below, descending=False)
    got = top(d, hops, fc, some, below, "NULL", descending=False)
    assert np.array_equal(sort_rows(got), sort_rows(asc[:, : hops + 3])) and np.array_equal(got[:, hops + 1], asc[:, hops + 1])


def test_recent_messages_of_friends(db):
    """interactive-complex-2.sql: knows -> message, m_creationdate < :date ORDER BY m_creationdate DESC, m_messageid LIMIT n"""
    d, g, ext, some = db
    check_tail(d, 1, 1, some, 700)


def test_recent_messages_of_friends_of_friends(db):
    """the 2-hop arm of interactive-complex-9.sql:13-18"""
    d, g, ext, some = db
    check_tail(d, 2, 2, some, 350)


@pytest.mark.parametrize("hops", [1, 2])
def test_a_half_open_date_range_as_filter_and_count(db, hops):
    """interactive-complex-4.sql:9,18: m_creationdate >= :lo AND m_creationdate < :hi before the GROUP BY"""
    d, g, ext, some = db
    lo, hi = 200, 420
    select = ", ".join(f"p{c}.p_personid" for c in range(hops + 1)) + ", m.m_messageid, m.rowid"
    base = X.sql_extend(hops, hops, some, select)
    want = d.execute(base + f" AND m.m_creationdate >= {lo} AND m.m_creationdate < {hi}")
    everything = int(d.execute(X.sql_extend(hops, hops, some, "count(*)"))[0, 0])
    args = f"{GRAPH}, {in_list(some)}, {hops}, {MESSAGE}, {hops}, 'm_creationdate', {hops + 1}, {lo}, {hi - 1}"
    rows = d.execute(f"SELECT {id_cols(hops)} FROM gg_khop_extend_filter({args}, false)")
    assert 0 < want.shape[0] < everything and np.array_equal(sort_rows(rows), sort_rows(want))
    count = d.execute(f"SELECT rows, walks, valued FROM gg_khop_extend_filter_count({args}, false)")
    assert count.tolist() == [[want.shape[0], everything, everything]]
    outside = d.execute(f"SELECT {id_cols(hops)} FROM gg_khop_extend_filter({args}, true)")
    want_outside = d.execute(base + f" AND NOT (m.m_creationdate >= {lo} AND m.m_creationdate < {hi})")
    assert np.array_equal(sort_rows(outside), sort_rows(want_outside)) and rows.shape[0] + outside.shape[0] == everything
    # a value of the walk's own column: the friend's id as its value, k_person2id <> :person (interactive-complex-9.sql:12)
    friend = int(want[0, 1])
    args = f"{GRAPH}, {in_list(some)}, {hops}, {MESSAGE}, {hops}, 'p_personid', 1, {friend}, {friend}, true"
    rows = d.execute(f"SELECT {id_cols(hops)} FROM gg_khop_extend_filter({args})")
    want = d.execute(base + f" AND p1.p_personid <> {friend}")
    assert 0 < want.shape[0] < everything and np.array_equal(sort_rows(rows), sort_rows(want))


def test_a_null_value_passes_nothing(db):
    d, g, ext, some = db
    d.execute("CREATE TABLE message_n (m_messageid BIGINT NOT NULL, m_creatorid BIGINT NOT NULL, m_creationdate BIGINT)")
    d.execute("INSERT INTO message_n SELECT m_messageid, m_creatorid, CASE WHEN m_creationdate % 3 = 0 THEN NULL ELSE "
              "m_creationdate END FROM message")
    table = "'message_n', 'm_creatorid', 'm_messageid'"
    select = "p0.p_personid, p1.p_personid, m.m_messageid"
    base = X.sql_extend(1, 1, some, select).replace("message m", "message_n m")
    everything = int(d.execute(X.sql_extend(1, 1, some, "count(*)"))[0, 0])
    for negate, cond in (("false", "m.m_creationdate IS NOT NULL"), ("true", "m.m_creationdate <> 100")):
        lo, hi = ("NULL", "NULL") if negate == "false" else (100, 100)
        args = f"{GRAPH}, {in_list(some)}, 1, {table}, 1, 'm_creationdate', 2, {lo}, {hi}, {negate}"
        rows = d.execute(f"SELECT v0, v1, w FROM gg_khop_extend_filter({args})")
        want = d.execute(base + " AND " + cond)
        assert 0 < want.shape[0] < everything and np.array_equal(sort_rows(rows), sort_rows(want))
        count = d.execute(f"SELECT rows, walks, valued FROM gg_khop_extend_filter_count({args})")
        valued = int(d.execute(base.replace(select, "count(*)") + " AND m.m_creationdate IS NOT NULL")[0, 0])
        assert count.tolist() == [[want.shape[0], everything, valued]] and valued < everything
    got = d.execute(f"SELECT w FROM gg_khop_extend_top({GRAPH}, {in_list(some)}, 1, {table}, 1, 'm_creationdate', 2, NULL, NULL, "
                    "false, true, 2, 50)")
    want = d.execute(base.replace(select, "m.m_messageid") + " AND m.m_creationdate IS NOT NULL ORDER BY m.m_creationdate DESC, "
                     "m.m_messageid LIMIT 50")
    assert np.array_equal(got, want)


def test_two_rows_of_one_message_with_different_values_are_refused(db):
    d, g, (es, ed), some = db
    d.execute("CREATE TABLE message_d AS SELECT * FROM message")
    d.execute(f"INSERT INTO message_d SELECT m_messageid, m_creatorid, m_creationdate + 1 FROM message WHERE m_messageid = {int(ed[0])}")
    args = f"{GRAPH}, {in_list(some)}, 1, 'message_d', 'm_creatorid', 'm_messageid', 1, 'm_creationdate', 2, 0, 100"
    for fn, more in (("gg_khop_extend_filter", ", false"), ("gg_khop_extend_filter_count", ", false"),
                     ("gg_khop_extend_top", ", false, true, NULL, 5")):
        with pytest.raises(RuntimeError, match="different values"):
            d.execute(f"SELECT * FROM {fn}({args}{more})")
    # equal values twice are one value: ext_table repeats rows by design, and message itself is accepted
    good = args.replace("'message_d'", "'message'")
    assert d.execute(f"SELECT count(*) FROM gg_khop_extend_filter({good}, false)")[0, 0] > 0
    # bad arguments
    for bad in (good.replace("'m_creationdate', 2", "'m_creationdate', 3"), good.replace("'m_creationdate', 2", "'no_such', 2"),
                good.replace("'m_creationdate', 2", "NULL, 2")):
        with pytest.raises(RuntimeError):
            d.execute(f"SELECT * FROM gg_khop_extend_filter({bad}, false)")
    with pytest.raises(RuntimeError):
        d.execute(f"SELECT * FROM gg_khop_extend_top({good}, false, true, 5, 5)")  # tie_col outside 0..hops + 1
