"""gg_triangle_edges inside the compiled reference, with the reference's own plan of the three-join statement selecting
the three rowids as the yardstick, and the late join on those rowids back to the edge table (no planner rule is on)."""
import os

import numpy as np
import pytest

from oracle import ref_duckdb as R
from tests import triangle_edges_ref as E
from tests import triangles_ref as T
from tests.oracle_lib import sort_rows

EXT = R.EXTENSION

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not (R.available() and os.path.exists(EXT)), reason="reference build / extension not present"),
]

GRAPH = "'person', 'p_personid', 'knows', 'k_person1id', 'k_person2id'"
SIX = T.SQL_ROWS + ", k1.rowid, k2.rowid, k3.rowid"


@pytest.fixture(scope="module")
def db():
    vid, src, dst = E.graph()  # dangling rows among the first thousand: a rowid is not an index among the kept rows
    d = R.RefDuckDB(threads=4)
    d.load_ldbc(vid, src, dst)
    d.load_table("persons_of_country", {"personid": np.sort(vid)[::3]})  # a third of the persons
    d.execute(f"LOAD '{EXT}'")
    want = {o: sort_rows(np.asarray(d.execute(T.sql_triangles(SIX, o)), np.int64)) for o in (False, True)}
    yield d, vid, src, dst, want
    d.close()


def flag(ordered):
    return "true" if ordered else "false"


def edges_sql(ordered, graph=GRAPH):
    return f"SELECT v0, v1, v2, e1, e2, e3 FROM gg_triangle_edges({graph}, {flag(ordered)})"


@pytest.mark.parametrize("ordered", [False, True])
def test_six_columns_equal_the_three_join_plan(db, ordered):
    d, vid, src, dst, want = db
    got = np.asarray(d.execute(edges_sql(ordered)), np.int64)
    assert want[ordered].shape[0] > 0 and np.array_equal(sort_rows(got), want[ordered])
    assert np.array_equal(want[ordered], sort_rows(E.rows(vid, src, dst, None, int(ordered))))  # and the restatement
    assert int(d.execute(f"SELECT count(*) FROM gg_triangle_edges({GRAPH}, {flag(ordered)})")[0, 0]) == got.shape[0]


@pytest.mark.parametrize("ordered", [False, True])
def test_the_late_join_on_rowids_reproduces_the_endpoints(db, ordered):
    d, vid, src, dst, want = db
    got = d.execute(
        "SELECT count(*), sum(CASE WHEN k1.k_person1id = t.v0 AND k1.k_person2id = t.v1 AND k2.k_person1id = t.v1 AND "
        "k2.k_person2id = t.v2 AND k3.k_person1id = t.v2 AND k3.k_person2id = t.v0 THEN 1 ELSE 0 END) "
        f"FROM gg_triangle_edges({GRAPH}, {flag(ordered)}) t JOIN knows k1 ON k1.rowid = t.e1 "
        "JOIN knows k2 ON k2.rowid = t.e2 JOIN knows k3 ON k3.rowid = t.e3")
    n = want[ordered].shape[0]
    assert int(got[0, 0]) == n and int(got[0, 1]) == n  # every row joins, and to its own three edge rows


def test_friend_triangles_of_one_country(db):
    """benchmark/ldbc/queries/bi-11.sql:22-33 restated over the persons_of_country table, with its edge rows"""
    d, vid, src, dst, want = db
    ref = sort_rows(np.asarray(d.execute(T.sql_triangles(SIX, True, person="persons_of_country", key="personid")), np.int64))
    got = np.asarray(d.execute(edges_sql(True, "'persons_of_country', 'personid', 'knows', 'k_person1id', 'k_person2id'")),
                     np.int64)
    assert 0 < ref.shape[0] < want[True].shape[0] and np.array_equal(sort_rows(got), ref)


def test_over_a_pinned_graph(db):
    """the pin carries no rowids: the function uses its rowid-carrying companion (built by the first statement) and never
    fails; the ids-only function goes on using the pin itself"""
    d, vid, src, dst, want = db
    d.execute("PRAGMA gg_use_pinned_graphs")
    try:
        d.execute(f"SELECT * FROM gg_graph_pin({GRAPH})")
        for _ in range(2):
            for ordered in (False, True):
                got = np.asarray(d.execute(edges_sql(ordered)), np.int64)
                assert np.array_equal(sort_rows(got), want[ordered])
                ids = np.asarray(d.execute(f"SELECT v0, v1, v2 FROM gg_triangles({GRAPH}, {flag(ordered)})"), np.int64)
                assert np.array_equal(sort_rows(ids), sort_rows(want[ordered][:, :3]))
        assert int(d.execute("SELECT * FROM gg_graph_pins()")[0, 0]) == 1
    finally:
        d.execute("SELECT * FROM gg_graph_unpin()")
        d.execute("PRAGMA gg_ignore_pinned_graphs")


def test_a_missing_column_raises_and_the_connection_stays_usable(db):
    d, vid, src, dst, want = db
    with pytest.raises(RuntimeError):
        d.execute("SELECT * FROM gg_triangle_edges('person', 'p_personid', 'knows', 'no_such_column', 'k_person2id', true)")
    with pytest.raises(RuntimeError):
        d.execute("SELECT * FROM gg_triangle_edges('person', 'no_such_key', 'knows', 'k_person1id', 'k_person2id', false)")
    got = np.asarray(d.execute(edges_sql(True)), np.int64)
    assert np.array_equal(sort_rows(got), want[True])
