"""gg_triangle_count / gg_triangles inside the compiled reference, with the reference's own plan of the three-join
statement over the same tables as the yardstick (no planner rule is on: the joins run as the reference plans them)."""
import os

import numpy as np
import pytest

from oracle import ref_duckdb as R
from tests import triangles_ref as T
from tests.oracle_lib import sort_rows

EXT = R.EXTENSION

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not (R.available() and os.path.exists(EXT)), reason="reference build / extension not present"),
]

GRAPH = "'person', 'p_personid', 'knows', 'k_person1id', 'k_person2id'"


@pytest.fixture(scope="module")
def db():
    vid, src, dst = T.hard_graph()
    d = R.RefDuckDB(threads=4)
    d.load_ldbc(vid, src, dst)
    d.load_table("persons_of_country", {"personid": np.sort(vid)[::3]})  # a third of the persons
    d.execute(f"LOAD '{EXT}'")
    want = {o: sort_rows(d.execute(T.sql_triangles(T.SQL_ROWS, o))) for o in (False, True)}
    yield d, vid, want
    d.close()


def flag(ordered):
    return "true" if ordered else "false"


@pytest.mark.parametrize("ordered", [False, True])
def test_count_and_rows_equal_the_three_join_plan(db, ordered):
    d, vid, want = db
    n = int(d.execute(T.sql_triangles("count(*)", ordered))[0, 0])
    assert n == want[ordered].shape[0] > 0
    got = d.execute(f"SELECT rows, digest, wedges FROM gg_triangle_count({GRAPH}, {flag(ordered)})")
    assert got.shape == (1, 3) and int(got[0, 0]) == n and int(got[0, 2]) >= n > 0
    rows = d.execute(f"SELECT v0, v1, v2 FROM gg_triangles({GRAPH}, {flag(ordered)})")
    assert np.array_equal(sort_rows(rows), want[ordered])
    assert int(d.execute(f"SELECT count(*) FROM gg_triangles({GRAPH}, {flag(ordered)})")[0, 0]) == n


def test_friend_triangles_of_one_country(db):
    """benchmark/ldbc/queries/bi-11.sql:22-33 restated over the persons_of_country table"""
    d, vid, want = db
    n = int(d.execute(T.sql_triangles("count(*)", True, person="persons_of_country", key="personid"))[0, 0])
    got = d.execute("SELECT rows FROM gg_triangle_count('persons_of_country', 'personid', 'knows', 'k_person1id', "
                    "'k_person2id', true)")
    assert int(got[0, 0]) == n and 0 < n < want[True].shape[0]


def test_over_a_pinned_graph(db):
    d, vid, want = db
    d.execute("PRAGMA gg_use_pinned_graphs")
    try:
        d.execute(f"SELECT * FROM gg_graph_pin({GRAPH})")
        for _ in range(2):
            for ordered in (False, True):
                rows = d.execute(f"SELECT v0, v1, v2 FROM gg_triangles({GRAPH}, {flag(ordered)})")
                assert np.array_equal(sort_rows(rows), want[ordered])
                got = d.execute(f"SELECT rows FROM gg_triangle_count({GRAPH}, {flag(ordered)})")
                assert int(got[0, 0]) == want[ordered].shape[0]
        assert int(d.execute("SELECT * FROM gg_graph_pins()")[0, 0]) == 1
    finally:
        d.execute("SELECT * FROM gg_graph_unpin()")
        d.execute("PRAGMA gg_ignore_pinned_graphs")


def test_a_missing_column_raises_and_the_connection_stays_usable(db):
    d, vid, want = db
    with pytest.raises(RuntimeError):
        d.execute("SELECT * FROM gg_triangle_count('person', 'p_personid', 'knows', 'no_such_column', 'k_person2id', true)")
    with pytest.raises(RuntimeError):
        d.execute("SELECT * FROM gg_triangles('person', 'no_such_key', 'knows', 'k_person1id', 'k_person2id', false)")
    got = d.execute(f"SELECT rows FROM gg_triangle_count({GRAPH}, true)")
    assert int(got[0, 0]) == want[True].shape[0]
