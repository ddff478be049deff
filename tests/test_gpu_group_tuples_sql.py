"""gg_khop_extend_group_columns inside the compiled reference, with the reference's own plans of `SELECT ..., count(*),
count(x), sum(x), min(x), max(x) ... GROUP BY ...` over the same join chains and tables as the yardstick (no planner rule is
on): the count form over two columns of the walk table (`GROUP BY startPerson, friend`,
benchmark/ldbc/queries/bi-10-shortestpath.sql:28-30), the valued form over (v0, w) of an extended table with a NULL value
among the messages' dates (max(l_creationdate) ... GROUP BY, interactive-complex-7.sql:7-12), the empty ext_table form, and
the binder's refusals.

SQL gives GROUP BY no order, so sorted row sets are compared — as text, since sum is a HUGEINT and NULLs occur."""
import os

import numpy as np
import pytest

from oracle import ref_duckdb as R
from tests import edge_filter_ref as F
from tests import extend_ref as X
from tests import triangles_ref as T

EXT = R.EXTENSION

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not (R.available() and os.path.exists(EXT)), reason="reference build / extension not present"),
]

GRAPH = "'person', 'p_personid', 'knows', 'k_person1id', 'k_person2id'"
MESSAGE = "'message_n', 'm_creatorid', 'm_messageid'"
FN = "gg_khop_extend_group_columns"


@pytest.fixture(scope="module")
def db():
    vid, src, dst = T.hard_graph()
    g = T.TriangleGraph(vid, src, dst)
    es, ed, er, info = X.ext_table(g)
    d = R.RefDuckDB(threads=4)
    d.load_ldbc(vid, src, dst)
    d.load_table("message", {"m_messageid": ed, "m_creatorid": es})
    # a date per message of both signs, NULL for one message in five; a score per person just below 2^63, NULL for some
    d.execute("CREATE TABLE message_n (m_messageid BIGINT NOT NULL, m_creatorid BIGINT NOT NULL, m_date BIGINT)")
    d.execute("INSERT INTO message_n SELECT m_messageid, m_creatorid, CASE WHEN m_messageid % 5 = 0 THEN NULL ELSE "
              "(m_messageid * 7919) % 1009 - 500 END FROM message")
    d.execute("CREATE TABLE person_n (p_personid BIGINT NOT NULL, p_score BIGINT)")
    d.execute("INSERT INTO person_n SELECT p_personid, CASE WHEN (p_personid >> 10) % 4 = 0 THEN NULL ELSE "
              "9223372036854775805 + abs((p_personid >> 10) % 3) END FROM person")
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


def chain(hops, some, extended):
    """' FROM ... WHERE ...' of the walks [joined with message_n on the last person]"""
    if extended:
        text = X.sql_extend(hops, hops, some, "1").replace("message m", "message_n m")
        return text[text.index(" FROM "):]
    frm, cond = F._chain(hops)
    return f" FROM {', '.join(frm)} WHERE " + " AND ".join(cond + F._sources(some))


def check(d, some, hops, columns, value=None, extended=True, ext_args=None):
    """one call against the reference's GROUP BY over the same chain, as sorted rows of text; value: (the column of the
    table function's table, value_of, the reference's expression).  Returns the rows."""
    keys = ", ".join(column_name(hops, c) for c in columns)
    tail = ext_args or (f"{MESSAGE}, {hops}" if extended else "NULL, NULL, NULL, NULL")
    text = ", ".join(str(c) for c in columns)
    if value is None:
        want = d.execute_text(f"SELECT {keys}, count(*), 0, 0, NULL, NULL" + chain(hops, some, extended) + f" GROUP BY {keys}")
        more = "NULL, NULL"
    else:
        column, value_of, x = value
        want = d.execute_text(f"SELECT {keys}, count(*), count({x}), sum({x}), min({x}), max({x})"
                              + chain(hops, some, extended) + f" GROUP BY {keys}")
        more = f"'{column}', {value_of}"
    got = d.execute_text(f"SELECT * FROM {FN}({GRAPH}, {in_list(some)}, {hops}, {tail}, '{text}', {more})")
    assert len(got) == len(want) > 0 and sorted(got, key=repr) == sorted(want, key=repr)
    assert len({row[:len(columns)] for row in got}) == len(got)  # one row per tuple
    return got


@pytest.mark.parametrize("hops", [1, 2])
def test_count_form_over_two_columns_of_the_walk_table(db, hops):
    d, some = db
    rows = check(d, some, hops, [0, hops], extended=False)
    assert any(int(r[2]) > 1 for r in rows) or hops == 1  # a friend of a friend is reached over several walks
    assert all(r[3:] == ("0", "0", None, None) for r in rows)
    check(d, some, hops, [hops, 0], extended=False)
    check(d, some, hops, [hops], extended=False)


@pytest.mark.parametrize("hops", [1, 2])
def test_valued_form_over_start_and_message_with_a_null_value(db, hops):
    d, some = db
    rows = check(d, some, hops, [0, hops + 1], ("m_date", hops + 1, "m.m_date"))
    assert any(r[3] == "0" and r[4:] == (None, None, None) for r in rows)  # a message without a date: count 0, NULLs
    assert any(r[3] != "0" and int(r[5]) < 0 for r in rows) and any(r[3] != "0" and int(r[5]) > 0 for r in rows)
    rows = check(d, some, hops, [0], ("m_date", hops + 1, "m.m_date"))      # per start person: the dates of many messages
    assert all(int(r[1]) >= int(r[2]) for r in rows) and any(int(r[2]) > 1 and int(r[4]) < int(r[5]) for r in rows)
    # a property of a person as the value, read from another table of the same key: sums past 2^64
    graph_n = GRAPH.replace("'person'", "'person_n'")
    keys = f"p0.p_personid, p{hops}.p_personid"
    want = d.execute_text(f"SELECT {keys}, count(*), count(n.p_score), sum(n.p_score), min(n.p_score), max(n.p_score)"
                          + chain(hops, some, True).replace(" WHERE ", f", person_n n WHERE n.p_personid = p{hops}.p_personid AND ", 1)
                          + f" GROUP BY {keys}")
    got = d.execute_text(f"SELECT * FROM {FN}({graph_n}, {in_list(some)}, {hops}, {MESSAGE}, {hops}, '0, {hops}', 'p_score', {hops})")
    assert sorted(got, key=repr) == sorted(want, key=repr)
    assert any(r[4] is not None and int(r[4]) > 1 << 64 for r in got) and any(r[3] == "0" and r[4] is None for r in got)


def test_the_empty_ext_table_form(db):
    d, some = db
    rows = check(d, some, 2, [0, 2], extended=False, ext_args="'', 'm_creatorid', 'm_messageid', 0")
    assert sorted(rows, key=repr) == sorted(check(d, some, 2, [0, 2], extended=False), key=repr)
    check(d, some, 2, [2], ("p_personid", 2, "p2.p_personid"), extended=False)  # the key column itself as the value


def test_argument_errors_name_the_argument(db):
    d, some = db
    good = f"{GRAPH}, {in_list(some)}, 2, {MESSAGE}, 2"
    assert d.execute(f"SELECT count(*) FROM {FN}({good}, '3', NULL, NULL)")[0, 0] > 0
    for columns in ("'0,,3'", "'x'", "''", "NULL", "'3, 0, 3'", "'4'"):
        with pytest.raises(RuntimeError, match="columns"):
            d.execute_text(f"SELECT * FROM {FN}({good}, {columns}, NULL, NULL)")
    plain = f"{GRAPH}, {in_list(some)}, 2, NULL, NULL, NULL, NULL"
    with pytest.raises(RuntimeError, match="columns"):
        d.execute_text(f"SELECT * FROM {FN}({plain}, '3', NULL, NULL)")  # without an extension the columns are 0..hops
    with pytest.raises(RuntimeError, match="value_of"):
        d.execute_text(f"SELECT * FROM {FN}({good}, '0', 'm_date', NULL)")
    with pytest.raises(RuntimeError, match="value_of"):
        d.execute_text(f"SELECT * FROM {FN}({good}, '0', 'm_date', 4)")
    with pytest.raises(RuntimeError, match="value_of"):
        d.execute_text(f"SELECT * FROM {FN}({plain}, '0', 'p_personid', 3)")
    with pytest.raises(RuntimeError):
        d.execute_text(f"SELECT * FROM {FN}({good}, '0', 'no_such_column', 3)")
    assert d.execute(f"SELECT count(*) FROM {FN}({good}, '0, 3', 'm_date', 3)")[0, 0] > 0  # and the session lives on
