"""gg_khop_edge_filter / gg_khop_edge_filter_count inside the compiled reference, with the reference's own plans of the
closed-walk, NOT EXISTS and EXISTS statements (tests/edge_filter_ref.py) over the same tables as the yardstick (no planner
rule is on: the joins run as the reference plans them)."""
import os

import numpy as np
import pytest

from oracle import ref_duckdb as R
from tests import edge_filter_ref as F
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
    g = T.TriangleGraph(vid, src, dst)
    d = R.RefDuckDB(threads=4)
    d.load_ldbc(vid, src, dst)
    d.execute(f"LOAD '{EXT}'")
    indeg = np.bincount(g.dv, minlength=g.V)
    three = np.unique(g.vid[[int(indeg.argmax()), 3] + np.nonzero(g.A.diagonal())[0].tolist()[:1]])
    assert three.size == 3  # the hub, dense index 3, a self-loop vertex
    yield d, g, three
    d.close()


def in_list(ids):
    return "'SELECT p_personid FROM person WHERE p_personid IN (" + ", ".join(str(int(s)) for s in ids) + ")'"


def both(d, sources_sql, hops, fc, tc, mode):
    """(the function's rows, its count row)"""
    args = f"{GRAPH}, {sources_sql}, {hops}, {fc}, {tc}, '{mode}'"
    cols = ", ".join(f"v{c}" for c in range(hops + 1))
    rows = d.execute(f"SELECT {cols} FROM gg_khop_edge_filter({args})")
    count = d.execute(f"SELECT rows, walks, matches FROM gg_khop_edge_filter_count({args})")
    assert count.shape == (1, 3)
    assert int(d.execute(f"SELECT count(*) FROM gg_khop_edge_filter({args})")[0, 0]) == rows.shape[0] == int(count[0, 0])
    return rows, count[0]


def test_closed_four_walks_through_three_persons(db):
    d, g, three = db
    want = d.execute(F.sql_closed_walks(4, three))
    rows, count = both(d, in_list(three), 3, 3, 0, "inner")
    assert want.shape[0] > 0 and np.array_equal(sort_rows(rows), sort_rows(want))
    assert int(count[0]) == int(count[2]) == int(d.execute(F.sql_closed_walks(4, three, "count(*)"))[0, 0])
    assert int(count[1]) == F.walks(g, three, 3).shape[0]


@pytest.mark.parametrize("sources", ["one", "list"])
def test_not_exists_of_complex_10(db, sources):
    d, g, three = db
    ids = three[:1] if sources == "one" else three
    want = d.execute(F.sql_exists(2, 0, 2, True, ids))
    rows, count = both(d, in_list(ids), 2, 0, 2, "anti")
    assert want.shape[0] > 0 and np.array_equal(sort_rows(rows), sort_rows(want))
    assert int(count[0]) == int(d.execute(F.sql_exists(2, 0, 2, True, ids, "count(*)"))[0, 0])


def test_exists(db):
    d, g, three = db
    want = d.execute(F.sql_exists(2, 0, 2, False, three))
    rows, count = both(d, in_list(three), 2, 0, 2, "semi")
    assert want.shape[0] > 0 and np.array_equal(sort_rows(rows), sort_rows(want))
    assert int(count[0]) == int(d.execute(F.sql_exists(2, 0, 2, False, three, "count(*)"))[0, 0])
    assert int(count[2]) >= int(count[0])


@pytest.mark.parametrize("all_sources", ["NULL", "''"])
def test_all_sources_closed_two_walks_are_gg_triangles(db, all_sources):
    d, g, three = db
    rows, count = both(d, all_sources, 2, 2, 0, "inner")
    tri = d.execute(f"SELECT v0, v1, v2 FROM gg_triangles({GRAPH}, false)")
    assert tri.shape[0] > 0 and np.array_equal(sort_rows(rows), sort_rows(tri))


def test_over_a_pinned_graph(db):
    d, g, three = db
    want = sort_rows(d.execute(F.sql_exists(2, 0, 2, True, three)))
    d.execute("PRAGMA gg_use_pinned_graphs")
    try:
        d.execute(f"SELECT * FROM gg_graph_pin({GRAPH})")
        for _ in range(2):
            rows, count = both(d, in_list(three), 2, 0, 2, "anti")
            assert np.array_equal(sort_rows(rows), want)
        assert int(d.execute("SELECT * FROM gg_graph_pins()")[0, 0]) == 1
    finally:
        d.execute("SELECT * FROM gg_graph_unpin()")
        d.execute("PRAGMA gg_ignore_pinned_graphs")


def test_bad_arguments_raise_and_the_connection_stays_usable(db):
    d, g, three = db
    s = in_list(three)
    bad = [
        f"'person', 'p_personid', 'knows', 'no_such_column', 'k_person2id', {s}, 2, 0, 2, 'anti'",  # a missing column
        f"{GRAPH}, {s}, 2, 0, 2, 'outer'",   # a bad mode
        f"{GRAPH}, {s}, 2, 3, 0, 'inner'",   # a column outside 0..hops
        f"{GRAPH}, {s}, 2, 0, -1, 'inner'",
        f"{GRAPH}, {s}, 0, 0, 0, 'inner'",   # hops outside 1..GG_MAX_HOPS
        f"{GRAPH}, {s}, 9, 0, 0, 'inner'",
    ]
    for args in bad:
        for fn in ("gg_khop_edge_filter", "gg_khop_edge_filter_count"):
            with pytest.raises(RuntimeError):
                d.execute(f"SELECT * FROM {fn}({args})")
    rows, count = both(d, s, 2, 0, 2, "anti")
    assert rows.shape[0] == d.execute(F.sql_exists(2, 0, 2, True, three)).shape[0] > 0
