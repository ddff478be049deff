"""gg_khop_extend_distinct / gg_khop_extend_distinct_count inside the compiled reference, with the reference's own plans of
`SELECT DISTINCT ...` over the same join chains and tables as the yardstick (no planner rule is on): the messages of friends
[of friends] as a set, the (person, message) pairs under interactive-complex-10's count(DISTINCT m_messageid), and the
plain-walk form — `SELECT DISTINCT k2.k_person2id` of interactive-complex-10.sql:19-24 without its NOT EXISTS.

SQL gives DISTINCT no order, so sorted row sets are compared."""
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
    d.load_table("message", {"m_messageid": ed, "m_creatorid": es})
    d.execute(f"LOAD '{EXT}'")
    knows_hub = int(g.vid[g.su[g.dv == g.index[info["hub"]]][0]])
    light = int(es[(es != info["hub"]) & np.isin(es, g.vid)][0])
    some = np.unique(np.array([knows_hub, info["hub"], info["z"], light], np.int64))
    assert some.size == 4
    yield d, some
    d.close()


def in_list(ids):
    return "'SELECT p_personid FROM person WHERE p_personid IN (" + ", ".join(str(int(s)) for s in ids) + ")'"


def column_name(hops, c):
    return "m.m_messageid" if c == hops + 1 else f"p{c}.p_personid"


def check(d, some, hops, columns, extended=True):
    """one column list against the reference's SELECT DISTINCT over the same chain; returns (distinct rows, joined rows)"""
    select = ", ".join(column_name(hops, c) for c in columns)
    if extended:
        want = d.execute(X.sql_extend(hops, hops, some, "DISTINCT " + select))
        walks = int(d.execute(X.sql_extend(hops, hops, some, "count(*)"))[0, 0])
        tail = f"{MESSAGE}, {hops}"
    else:
        frm, cond = F._chain(hops)
        chain = f" FROM {', '.join(frm)} WHERE " + " AND ".join(cond + F._sources(some))
        want = d.execute("SELECT DISTINCT " + select + chain)
        walks = int(d.execute("SELECT count(*)" + chain)[0, 0])
        tail = "NULL, NULL, NULL, NULL"
    text = ", ".join(str(c) for c in columns)
    args = f"{GRAPH}, {in_list(some)}, {hops}, {tail}, '{text}'"
    names = ", ".join(f"c{j}" for j in range(len(columns)))
    rows = d.execute(f"SELECT {names} FROM gg_khop_extend_distinct({args})")
    assert rows.shape == want.shape and np.array_equal(sort_rows(rows), sort_rows(want))
    assert np.unique(rows, axis=0).shape[0] == rows.shape[0]
    count = d.execute(f"SELECT rows, walks FROM gg_khop_extend_distinct_count({args})")
    assert count.tolist() == [[want.shape[0], walks]]
    return want.shape[0], walks


@pytest.mark.parametrize("hops", [1, 2])
def test_messages_and_person_message_pairs_as_sets(db, hops):
    d, some = db
    messages, walks = check(d, some, hops, [hops + 1])
    pairs, _ = check(d, some, hops, [0, hops + 1])
    assert 0 < messages <= pairs < walks  # a message is reached over several walks
    check(d, some, hops, [hops + 1, 0])   # the list's order is the output's
    check(d, some, hops, list(range(hops + 2)))


@pytest.mark.parametrize("hops", [1, 2])
def test_the_plain_walk_form(db, hops):
    """ext_table NULL: the walk table itself — SELECT DISTINCT k2.k_person2id (interactive-complex-10.sql:19-24)"""
    d, some = db
    ends, walks = check(d, some, hops, [hops], extended=False)
    assert 0 < ends < walks
    check(d, some, hops, [0, hops], extended=False)
    # an empty ext_table name is no extension either
    args = f"{GRAPH}, {in_list(some)}, {hops}, '', 'm_creatorid', 'm_messageid', 0, '{hops}'"
    assert d.execute(f"SELECT count(*) FROM gg_khop_extend_distinct({args})")[0, 0] == ends


def test_argument_errors_name_the_argument(db):
    d, some = db
    good = f"{GRAPH}, {in_list(some)}, 2, {MESSAGE}, 2"
    assert d.execute(f"SELECT count(*) FROM gg_khop_extend_distinct({good}, '3')")[0, 0] > 0
    for fn in ("gg_khop_extend_distinct", "gg_khop_extend_distinct_count"):
        for columns in ("'0,,3'", "'0;3'", "'x'", "''", "'-1'", "NULL",   # malformed
                        "'3, 0, 3'",                                     # a repeated column
                        "'4'", "'0, 17'"):                               # outside 0..hops + 1
            with pytest.raises(RuntimeError, match="columns"):
                d.execute(f"SELECT * FROM {fn}({good}, {columns})")
        plain = f"{GRAPH}, {in_list(some)}, 2, NULL, NULL, NULL, NULL"
        with pytest.raises(RuntimeError, match="columns"):
            d.execute(f"SELECT * FROM {fn}({plain}, '3')")  # without an extension the columns are 0..hops
        with pytest.raises(RuntimeError):
            d.execute(f"SELECT * FROM {fn}({GRAPH}, {in_list(some)}, 2, {MESSAGE}, 3, '0')")  # from_col outside 0..hops
    assert d.execute(f"SELECT count(*) FROM gg_khop_extend_distinct({good}, '0, 3')")[0, 0] > 0  # and the session lives on
