"""gg_khop_extend_group inside the compiled reference, with the reference's own plan — hash joins, hash aggregate, order —
of the same statement over the same tables as the yardstick (no planner rule is on):
    SELECT <column key_col>, count(*) FROM <chain>, message m WHERE ... GROUP BY 1 ORDER BY 2 DESC, 1 [LIMIT n]
the tail of benchmark/ldbc/queries/interactive-complex-4.sql:1-22 with the key's id in the place of the tag's name."""
import os

import numpy as np
import pytest

from oracle import ref_duckdb as R
from tests import extend_ref as X
from tests import group_by_ref as G
from tests import triangles_ref as T

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
    yield d, g, some
    d.close()


def in_list(ids):
    return "'SELECT p_personid FROM person WHERE p_personid IN (" + ", ".join(str(int(s)) for s in ids) + ")'"


def groups(d, sources_sql, hops, fc, kc, n):
    rows = d.execute(f"SELECT rank, key, rows FROM gg_khop_extend_group({GRAPH}, {sources_sql}, {hops}, {MESSAGE}, {fc}, {kc}, "
                     f"{'NULL' if n is None else n})")
    assert np.array_equal(rows[:, 0], np.arange(rows.shape[0]))  # the ranks, in the order the rows leave
    return rows[:, 1:]


@pytest.mark.parametrize("hops,fc,kc", [(1, 1, 1), (2, 2, 0), (2, 2, 3), (2, 1, 2)])
def test_count_per_key_ordered_equals_the_references_plan(db, hops, fc, kc):
    d, g, some = db
    every = d.execute(G.sql_extend_group(hops, fc, kc, some))
    assert every.shape[0] > 1
    for n in (None, 1, 10, every.shape[0] + 7):
        want = d.execute(G.sql_extend_group(hops, fc, kc, some, n))
        got = groups(d, in_list(some), hops, fc, kc, n)
        assert want.shape[0] == (every.shape[0] if n is None else min(n, every.shape[0]))
        assert np.array_equal(got, want), (hops, fc, kc, n)
    assert groups(d, in_list(some), hops, fc, kc, 0).shape[0] == 0


def test_an_empty_source_list_and_a_source_that_is_no_person(db):
    d, g, some = db
    empty = "'SELECT p_personid FROM person WHERE p_personid < -1000000000000'"
    assert groups(d, empty, 2, 2, 3, None).shape[0] == 0
    assert groups(d, empty, 1, 1, 0, 5).shape[0] == 0
    stranger = f"'SELECT {X.NOT_A_PERSON}'"  # a key of message, but no person: it starts no walk
    assert groups(d, stranger, 1, 0, 0, None).shape[0] == 0
    mixed = (f"'SELECT {X.NOT_A_PERSON} UNION ALL SELECT p_personid FROM person WHERE p_personid IN ("
             + ", ".join(str(int(s)) for s in some) + ")'")
    want = d.execute(G.sql_extend_group(1, 1, 2, some))
    assert want.shape[0] > 0 and np.array_equal(groups(d, mixed, 1, 1, 2, None), want)


def test_bad_arguments_raise_and_the_connection_stays_usable(db):
    d, g, some = db
    s = in_list(some)
    bad = [
        f"{GRAPH}, {s}, 1, {MESSAGE}, 1, 3, 10",     # a key column outside 0..hops + 1
        f"{GRAPH}, {s}, 1, {MESSAGE}, 1, -1, 10",
        f"{GRAPH}, {s}, 1, {MESSAGE}, 1, NULL, 10",
        f"{GRAPH}, {s}, 1, {MESSAGE}, 2, 1, 10",     # from_col outside 0..hops
        f"{GRAPH}, {s}, 8, {MESSAGE}, 0, 0, 10",     # hops outside 1..GG_MAX_HOPS - 1
        f"{GRAPH}, {s}, 1, {MESSAGE}, 1, 1, -1",     # a negative n
        f"{GRAPH}, {s}, 1, 'no_such_table', 'm_creatorid', 'm_messageid', 1, 1, 10",
    ]
    for args in bad:
        with pytest.raises(RuntimeError):
            d.execute(f"SELECT * FROM gg_khop_extend_group({args})")
    want = d.execute(G.sql_extend_group(1, 1, 1, some, 3))
    assert np.array_equal(groups(d, s, 1, 1, 1, 3), want)
