"""UNION recursive CTEs with a depth counter run as GG_RECURSIVE_LEVELS (level sets on the GPU, under PRAGMA
enable_gpu_recursive_levels) and give the relation the reference's PhysicalRecursiveCTE gives with the rules off: the
friends CTE of bi-10-shortestpath.sql over the populated, mirrored knows under five consumers; several start persons;
duplicate anchor rows; NULL links, keys and nexts; a VARCHAR carried column; a cycle with a bound; an acyclic table
without one; an empty anchor and an empty table; bound 0; a prepared statement executed twice; and a seeded random set
of such statements.  Relations are compared sorted, and in order where the statement has an ORDER BY."""
import os

import numpy as np
import pytest

from oracle import ref_duckdb as R
from tests import ldbc_shapes
from tests.test_plan_rule import _ldbc_database
from tests.test_plan_rule_recursive_levels import BI10_FRIENDS

EXT = R.EXTENSION

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not (R.available() and os.path.exists(EXT) and R.rules_route() == "shim"),
                       reason="reference build / extension / interposition shim not present"),
]

LEVELS = "GG_RECURSIVE_LEVELS"
START = 19791209310731  # the person bi-10-shortestpath.sql starts from


def _key(row):
    return tuple("" if v is None else v for v in row)


def _on(d):
    d.execute("PRAGMA enable_gpu_graph")
    d.execute("PRAGMA enable_gpu_recursive_levels")


def _off(d):
    d.execute("PRAGMA disable_gpu_recursive_levels")
    d.execute("PRAGMA disable_gpu_graph")


def compare(d, sql, ordered=False, nonempty=True):
    """the rules off and on give the same relation; the plan with them on is the level sets'"""
    _off(d)
    assert LEVELS not in d.explain(sql)
    cpu = d.query_text(sql)
    _on(d)
    try:
        assert LEVELS in d.explain(sql), sql
        gpu = d.query_text(sql)
    finally:
        _off(d)
    if nonempty:
        assert len(cpu) > 0, sql
    if ordered:
        assert gpu == cpu, sql
    else:
        assert sorted(gpu, key=_key) == sorted(cpu, key=_key), sql
    return cpu


@pytest.fixture(scope="module")
def db():
    d = _ldbc_database(populated=True)  # (loads the extension)
    d.execute("CREATE TABLE t (k BIGINT, n BIGINT, pay VARCHAR)")
    d.execute("INSERT INTO t VALUES (1, 2, 'a'), (2, 3, 'b'), (3, 1, 'c'), (3, 4, 'd'), (4, NULL, 'e'), (NULL, 5, 'f'), "
              "(5, 6, 'g'), (6, 5, 'h'), (2, 2, 'i'), (2, 3, 'j')")
    d.execute("CREATE TABLE dag (k BIGINT, n BIGINT)")
    d.execute("INSERT INTO dag VALUES (1, 2), (1, 3), (2, 4), (3, 4), (4, 5), (4, 6), (6, 7), (2, 7), (7, NULL), (9, 1)")
    d.execute("CREATE TABLE empty_t (k BIGINT, n BIGINT)")
    yield d
    _off(d)
    d.close()


A, B, X = int(ldbc_shapes.PERSON_A), int(ldbc_shapes.PERSON_B), int(ldbc_shapes.PERSON_X)


@pytest.mark.parametrize("consumer,ordered", [
    ("SELECT * FROM friends", False),
    ("SELECT hopCount, count(*) FROM friends GROUP BY hopCount ORDER BY hopCount", True),
    ("SELECT friend, max(hopCount) FROM friends GROUP BY friend", False),
    ("SELECT DISTINCT friend FROM friends WHERE hopCount BETWEEN 2 AND 4", False),
    ("SELECT f.hopCount, p.p_firstname, p.p_personid FROM friends f, person p WHERE f.friend = p.p_personid", False),
])
def test_bi10_friends_under_five_consumers(db, consumer, ordered):
    rows = compare(db, BI10_FRIENDS + consumer, ordered=ordered)
    assert len(rows) > 5


def _friends(anchor, bound="f.hopCount < 4"):
    return ("WITH RECURSIVE friends(startPerson, hopCount, friend) AS (" + anchor + " UNION SELECT f.startPerson, "
            "f.hopCount + 1, k.k_person2id FROM friends f, knows k WHERE f.friend = k.k_person1id AND " + bound + ") ")


def test_an_in_list_of_start_persons(db):
    sql = _friends(f"SELECT p_personid, 0, p_personid FROM person WHERE p_personid IN ({A}, {B}, {X}, {START}, 12345)")
    rows = compare(db, sql + "SELECT * FROM friends")
    assert len({r[0] for r in rows}) >= 4
    compare(db, sql + "SELECT startPerson, hopCount, count(*) FROM friends GROUP BY startPerson, hopCount "
                      "ORDER BY startPerson, hopCount", ordered=True)


def test_duplicate_anchor_rows(db):
    compare(db, _friends("SELECT 1::BIGINT, 0, k_person1id FROM knows WHERE k_person2id IN "
                         "(SELECT k_person2id FROM knows LIMIT 40)", "f.hopCount < 3") + "SELECT * FROM friends")


def test_null_links_keys_and_nexts(db):
    # anchor rows with a NULL link (they join nothing); T rows with a NULL key (join nothing) and a NULL next (a
    # (a, hop, NULL) row of its level, never expanded)
    compare(db, "WITH RECURSIVE c(a, hop, link) AS (SELECT v.a, 0, v.l FROM (VALUES (1, 3::BIGINT), (2, NULL), (2, NULL), "
                "(3, 4), (4, 2)) v(a, l) UNION SELECT c.a, c.hop + 1, t.n FROM t, c WHERE t.k = c.link AND c.hop < 5) "
                "SELECT * FROM c")


def test_a_varchar_carried_column_and_an_arm_constant(db):
    compare(db, "WITH RECURSIVE c(name, hop, link, tag) AS (SELECT p_firstname, 10, p_personid, 'anchor' FROM person "
                "WHERE p_personid % 11 = 0 UNION SELECT c.name, c.hop + 5, k.k_person2id, 'arm' FROM knows k, c "
                "WHERE k.k_person1id = c.link AND c.hop <= 20) SELECT * FROM c")


def test_a_cycle_with_a_bound(db):
    # 1 -> 2 -> 3 -> 1 (and 2 -> 2, 3 -> 4 -> NULL): the same links come back at every level, with another hop count
    rows = compare(db, "WITH RECURSIVE c(hop, link) AS (SELECT 0, 1::BIGINT UNION SELECT c.hop + 1, t.n FROM t, c "
                       "WHERE t.k = c.link AND c.hop < 12) SELECT * FROM c")
    assert ("12", "1") in rows and ("9", "1") in rows


def test_an_acyclic_table_without_a_bound(db):
    rows = compare(db, "WITH RECURSIVE c(a, hop, link) AS (SELECT v.a, 0, v.l FROM (VALUES (1, 1::BIGINT), (2, 9), (3, 6)) "
                       "v(a, l) UNION SELECT c.a, c.hop + 1, dag.n FROM dag, c WHERE dag.k = c.link) SELECT * FROM c")
    assert ("2", "6", None) in rows  # 9 -> 1 -> 2 -> 4 -> 6 -> 7 -> NULL


def test_an_empty_anchor_and_an_empty_table(db):
    compare(db, _friends("SELECT p_personid, 0, p_personid FROM person WHERE p_personid < 0") + "SELECT * FROM friends",
            nonempty=False)
    compare(db, "WITH RECURSIVE c(a, hop, link) AS (SELECT v.a, 0, v.l FROM (VALUES (1, 1::BIGINT), (1, 1), (2, NULL)) "
                "v(a, l) UNION SELECT c.a, c.hop + 1, e.n FROM empty_t e, c WHERE e.k = c.link AND c.hop < 3) "
                "SELECT * FROM c")


def test_bound_0(db):
    rows = compare(db, _friends(f"SELECT p_personid, 0, p_personid FROM person WHERE p_personid = {A}", "f.hopCount < 0")
                   + "SELECT * FROM friends")
    assert len(rows) == 1


def test_a_prepared_statement_executed_twice(db):
    """planned once with the rules on, executed three times: each execution sinks the tables and runs the levels anew.
    (The rules-off side runs the statement unprepared: the reference's own PhysicalRecursiveCTE keeps the pipelines of a
    prepared plan's first execution and does not survive a second one.)"""
    sql = ("WITH RECURSIVE c(a, hop, link) AS (SELECT 1, 0, {}::BIGINT UNION SELECT c.a, c.hop + 1, t.n FROM t, c "
           "WHERE t.k = c.link AND c.hop < 4) SELECT * FROM c")
    _off(db)
    cpu = [db.query_text(sql.format(v)) for v in (1, 5, 1)]
    _on(db)
    try:
        db.execute(f"PREPARE gpu_q AS {sql.format('?')}")
        assert LEVELS in db.explain(sql.format(1))
        gpu = [db.query_text(f"EXECUTE gpu_q({v})") for v in (1, 5, 1)]
        db.execute("DEALLOCATE gpu_q")
    finally:
        _off(db)
    assert all(len(c) > 1 for c in cpu)
    for g, c in zip(gpu, cpu):
        assert sorted(g, key=_key) == sorted(c, key=_key)


def random_statements(seed=2027, n=16):
    """(table rows as SQL values, statement, anchor rows) of random tables (small id domains: cycles, self-loops,
    duplicates, NULLs) and random arms of the accepted shapes only: a constant start, a positive step, a bound unless the
    table is acyclic, carried / constant columns at random"""
    rng = np.random.default_rng(seed)
    out = []
    for case in range(n):
        n_rows = int(rng.integers(4, 60))
        dom = int(rng.integers(3, 25))
        acyclic = case % 4 == 3
        vals = []
        for _ in range(n_rows):
            a, b = int(rng.integers(0, dom)), int(rng.integers(0, dom))
            if acyclic:
                a, b = min(a, b), max(a, b) + 1  # next > key: no cycle
            k = "NULL" if rng.random() < 0.08 else str(a)
            nxt = "NULL" if rng.random() < 0.08 else str(b)
            vals.append(f"({k}, {nxt}, 'p{int(rng.integers(0, 3))}')")
        n_anchor = int(rng.integers(1, 8))
        with_cls, with_tag = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
        anchor = []
        for _ in range(n_anchor):
            link = "NULL" if rng.random() < 0.1 else str(int(rng.integers(0, dom)))
            anchor.append(f"('c{int(rng.integers(0, 3))}', {link}::INTEGER, '{'arm' if rng.random() < 0.5 else 'anc'}')")
        start, step = int(rng.integers(-3, 4)), int(rng.integers(1, 4))
        cols = (["cls"] if with_cls else []) + ["hop", "link"] + (["tag"] if with_tag else [])
        first = (["v.cls"] if with_cls else []) + [str(start), "v.link"] + (["v.tag"] if with_tag else [])
        arm = (["c.cls"] if with_cls else []) + [f"c.hop + {step}", "rt.n"] + (["'arm'"] if with_tag else [])
        where = "rt.k = c.link"
        if not acyclic or rng.random() < 0.5:
            levels = int(rng.integers(0, 7))
            where += f" AND c.hop {'<' if rng.random() < 0.5 else '<='} {start + step * levels}"
        sql = (f"WITH RECURSIVE c({', '.join(cols)}) AS (SELECT {', '.join(first)} FROM (VALUES {', '.join(anchor)}) "
               f"v(cls, link, tag) UNION SELECT {', '.join(arm)} FROM rt, c WHERE {where}) SELECT * FROM c")
        out.append((vals, sql, n_anchor))
    return out


def test_seeded_random_statements(db):
    """every statement of the set runs as GG_RECURSIVE_LEVELS (compare asserts it) and equals the reference; at least half
    of them return more rows than their anchor has"""
    grew = 0
    statements = random_statements()
    for vals, sql, n_anchor in statements:
        db.execute("DROP TABLE IF EXISTS rt")
        db.execute("CREATE TABLE rt (k INTEGER, n INTEGER, s VARCHAR)")
        db.execute("INSERT INTO rt VALUES " + ", ".join(vals))
        cpu = compare(db, sql)
        grew += len(cpu) > n_anchor
    assert 2 * grew >= len(statements), (grew, len(statements))
