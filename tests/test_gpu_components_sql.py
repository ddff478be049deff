"""gg_components / gg_component_sizes inside the compiled reference, with the reference's own plan of the UNION recursive CTE
under an aggregate (tests/components_ref.sql_components) over the same tables as the yardstick: no planner rule is on, so the
recursion, its hash join and the aggregate run as the reference plans them.  The statement reports the smallest id of a
component where the functions report the id of its first vertex in the vertex table, so both sides are compared as
partitions: vertex -> (smallest id of its component, size)."""
import os

import pytest

from oracle import ref_duckdb as R
from tests import components_ref as K

EXT = R.EXTENSION

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not (R.available() and os.path.exists(EXT)), reason="reference build / extension not present"),
]

GRAPH = "'person', 'p_personid', 'knows', 'k_person1id', 'k_person2id'"


@pytest.fixture(scope="module")
def db():
    """300 vertices: a giant component of 200, four small ones, singletons, rows in one direction only, parallel rows, a
    self-loop and dangling rows; `und` is every kept row in both directions"""
    vid, src, dst = K.islands()
    want = K.components(vid, src, dst)
    assert want["stats"]["largest"] == 200 and want["stats"]["singletons"] > 10
    assert want["stats"]["components"] > want["stats"]["singletons"] + 3
    d = R.RefDuckDB(threads=4)
    d.load_table("person", {"p_personid": vid})
    d.load_table("knows", {"k_person1id": src, "k_person2id": dst})
    d.execute(K.sql_und())
    d.execute(f"LOAD '{EXT}'")
    yield d, want
    d.close()


def reference_partition(d):
    rows = d.query_text(K.sql_components())
    return {int(v): (int(m), int(c)) for v, m, c in rows}


def function_rows(d, graph=GRAPH):
    return [tuple(int(x) for x in r) for r in d.query_text(f"SELECT vertex, component, size FROM gg_components({graph})")]


def size_rows(d, graph=GRAPH):
    return [tuple(int(x) for x in r) for r in d.query_text(f"SELECT component, size FROM gg_component_sizes({graph})")]


def as_partition(rows):
    """{vertex: (smallest id of its component, size)} of (vertex, component, size) rows"""
    smallest = {}
    for v, c, s in rows:
        smallest[c] = min(smallest.get(c, v), v)
    return {v: (smallest[c], s) for v, c, s in rows}


def test_both_functions_equal_the_reference_recursive_cte(db):
    d, want = db
    ref = reference_partition(d)
    assert len(ref) == want["stats"]["vertices"] and ref == K.min_id_partition(want)  # the restatement agrees with the plan
    rows = function_rows(d)
    assert len(rows) == len(ref) and as_partition(rows) == ref
    # the rows themselves: the restatement's table 0 (the pipeline's threads hand the slabs out in any order)
    table0 = zip(want["vertex"].tolist(), want["component"].tolist(), want["size"].tolist())
    assert sorted(rows) == sorted((int(v), int(c), int(s)) for v, c, s in table0)
    # one row per component, with the size the statement counts for each of its members
    sizes = size_rows(d)
    assert sorted(sizes) == sorted(zip(want["components"].tolist(), (int(s) for s in want["sizes"].tolist())))
    by_component = dict(sizes)
    assert len(by_component) == len(sizes) == len({m for m, _ in ref.values()})
    for v, c, s in rows:
        assert by_component[c] == s == ref[v][1]
    # the functions compose with the rest of the statement
    got = d.query_text(f"SELECT count(*), max(size), sum(CASE WHEN size = 1 THEN 1 ELSE 0 END) FROM gg_component_sizes({GRAPH})")
    assert tuple(int(x) for x in got[0]) == (want["stats"]["components"], want["stats"]["largest"], want["stats"]["singletons"])


def test_over_a_pinned_graph_twice(db):
    d, want = db
    ref = reference_partition(d)
    d.execute("PRAGMA gg_use_pinned_graphs")
    try:
        d.execute(f"SELECT * FROM gg_graph_pin({GRAPH})")
        for _ in range(2):
            assert as_partition(function_rows(d)) == ref
            assert len(size_rows(d)) == want["stats"]["components"]
        assert int(d.execute("SELECT * FROM gg_graph_pins()")[0, 0]) == 1
    finally:
        d.execute("SELECT * FROM gg_graph_unpin()")
        d.execute("PRAGMA gg_ignore_pinned_graphs")


def test_bad_arguments_raise_and_the_connection_stays_usable(db):
    d, want = db
    bad = [
        "'person', 'p_personid', 'knows', 'no_such_column', 'k_person2id'",  # a missing column
        "'person', 'no_such_key', 'knows', 'k_person1id', 'k_person2id'",
        "'no_such_table', 'p_personid', 'knows', 'k_person1id', 'k_person2id'",
        "'person', 'p_personid', 'knows', 'k_person1id', NULL",
        "'person', 'p_personid', 'knows', 'k_person1id'",  # an argument short
    ]
    for fn in ("gg_components", "gg_component_sizes"):
        for args in bad:
            with pytest.raises(RuntimeError):
                d.execute(f"SELECT count(*) FROM {fn}({args})")
        assert as_partition(function_rows(d)) == K.min_id_partition(want)
