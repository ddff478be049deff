"""UNION recursive CTEs run as GG_RECURSIVE_REACH (the reachability closure on the GPU, under PRAGMA
enable_gpu_recursive_union) and give the relation the reference's PhysicalRecursiveCTE gives with the rules off:
reachability over the populated, mirrored knows; interactive-complex-12.sql over a tag-class hierarchy, with a cycle
added; duplicate anchor rows; NULL links, keys and nexts; anchor constants that differ from the arm's; a VARCHAR carried
column; an empty anchor and an empty table; a prepared statement executed twice; and a seeded random set of such
statements.  Relations are compared sorted, and in order where the statement has an ORDER BY."""
import os

import numpy as np
import pytest

from oracle import ref_duckdb as R
from tests import ldbc_shapes
from tests.test_plan_rule import _ldbc_database, _ldbc_texts

EXT = R.EXTENSION

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not (R.available() and os.path.exists(EXT) and R.rules_route() == "shim"),
                       reason="reference build / extension / interposition shim not present"),
]

REACH = "GG_RECURSIVE_REACH"
IC12_PERSON = 21990232556256  # the person interactive-complex-12.sql starts from


def _key(row):
    return tuple("" if v is None else v for v in row)


def _on(d):
    d.execute("PRAGMA enable_gpu_graph")
    d.execute("PRAGMA enable_gpu_recursive_union")


def _off(d):
    d.execute("PRAGMA disable_gpu_recursive_union")
    d.execute("PRAGMA disable_gpu_graph")


def compare(d, sql, ordered=False, nonempty=True):
    """the rules off and on give the same relation; the plan with them on is the reach closure's"""
    _off(d)
    assert REACH not in d.explain(sql)
    cpu = d.query_text(sql)
    _on(d)
    try:
        assert REACH in d.explain(sql), sql
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


TAGCLASSES = [(1, "Thing", None), (2, "Agent", 1), (3, "Person", 2), (4, "OfficeHolder", 3), (5, "Politician", 4),
              (6, "President", 5), (7, "Judge", 4), (8, "Place", 1), (9, "City", 8), (10, "Orphan", None)]


@pytest.fixture(scope="module")
def db():
    d = _ldbc_database(populated=True)  # (loads the extension)
    d.execute("DELETE FROM tagclass")
    d.execute("INSERT INTO tagclass VALUES " + ", ".join(
        f"({i}, '{n}', 'u', {'NULL' if p is None else p})" for i, n, p in TAGCLASSES))
    # tags under OfficeHolder's subclasses (and some elsewhere), so interactive-complex-12 selects some of them
    d.execute("UPDATE tag SET t_tagclassid = 5 + t_tagid % 5")
    # the person interactive-complex-12 starts from knows a few well-connected persons
    friends = [int(ldbc_shapes.PERSON_A), int(ldbc_shapes.PERSON_B), int(ldbc_shapes.PERSON_X)]
    d.execute("INSERT INTO knows VALUES " + ", ".join(f"('2012-01-01 00:00:00', {IC12_PERSON}, {f})" for f in friends))
    d.execute("CREATE TABLE t (k BIGINT, n BIGINT, pay VARCHAR)")
    d.execute("INSERT INTO t VALUES (1, 2, 'a'), (2, 3, 'b'), (3, 1, 'c'), (3, 4, 'd'), (4, NULL, 'e'), (NULL, 5, 'f'), "
              "(5, 6, 'g'), (6, 5, 'h'), (2, 2, 'i'), (2, 3, 'j')")
    d.execute("CREATE TABLE empty_t (k BIGINT, n BIGINT)")
    yield d
    _off(d)
    d.close()


A = int(ldbc_shapes.PERSON_A)


def _reach(anchor):
    return (f"WITH RECURSIVE reach(p) AS ({anchor} UNION SELECT k.k_person2id FROM reach r, knows k "
            "WHERE r.p = k.k_person1id) SELECT * FROM reach")


def test_reach_from_one_person_over_mirrored_knows(db):
    rows = compare(db, _reach(f"SELECT {A}::BIGINT"))
    assert len(rows) > 10


def test_reach_from_an_in_list(db):
    compare(db, _reach(f"SELECT p_personid FROM person WHERE p_personid IN ({A}, {int(ldbc_shapes.PERSON_B)}, "
                       f"{int(ldbc_shapes.PERSON_X)}, 12345)"))


def test_reach_with_a_class_per_start_and_order_by(db):
    sql = (f"WITH RECURSIVE reach(src, p) AS (SELECT p_personid, p_personid FROM person WHERE p_personid % 7 = 0 "
           "UNION SELECT r.src, k.k_person2id FROM reach r, knows k WHERE r.p = k.k_person1id) "
           "SELECT src, count(*) FROM reach GROUP BY src ORDER BY src")
    compare(db, sql, ordered=True)


def test_duplicate_anchor_rows(db):
    compare(db, _reach("SELECT k_person1id FROM knows WHERE k_person2id IN (SELECT k_person2id FROM knows LIMIT 40)"))


def _ic12():
    return _ldbc_texts()["queries"]["interactive-complex-12.sql"].strip().rstrip(";")


def _extended_tags():
    text = _ic12()
    return text[:text.index("\n)\n") + 3] + "SELECT * FROM extended_tags"


def test_interactive_complex_12_over_a_tag_class_hierarchy(db):
    rows = compare(db, _extended_tags())
    assert ("6", "1") in rows and ("10", "10") in rows and ("9", "2") not in rows
    compare(db, _ic12(), ordered=True)


def test_interactive_complex_12_over_a_hierarchy_with_a_cycle(db):
    db.execute("INSERT INTO tagclass VALUES (2, 'AgentAgain', 'u', 6)")  # 2 -> 3 -> 4 -> 5 -> 6 -> 2
    try:
        compare(db, _extended_tags())
        compare(db, _ic12(), ordered=True)
    finally:
        db.execute("DELETE FROM tagclass WHERE tc_name = 'AgentAgain'")


def test_null_links_keys_and_nexts(db):
    # anchor rows with a NULL link (seen: equal to the arm's (a, NULL); unseen: a constant differs); T rows with a NULL
    # key (joins nothing) and a NULL next (one (a, NULL) row per class)
    compare(db, "WITH RECURSIVE c(a, link) AS (SELECT * FROM (VALUES (1, 3::BIGINT), (2, NULL), (2, NULL), (3, 4)) v "
                "UNION SELECT c.a, t.n FROM t, c WHERE t.k = c.link) SELECT * FROM c")
    compare(db, "WITH RECURSIVE c(a, link, tag) AS (SELECT * FROM (VALUES (1, NULL::BIGINT, 'x'), (1, NULL, 'arm'), "
                "(2, 1, 'arm'), (3, 4, 'x')) v UNION SELECT c.a, t.n, 'arm' FROM t, c WHERE t.k = c.link) SELECT * FROM c")


def test_anchor_constants_that_differ_from_the_arms(db):
    # the anchor row (7, 1, 'anchor') differs from the arm's (7, 1, 'arm'): reached again, 1 is a row of its own
    rows = compare(db, "WITH RECURSIVE c(a, link, tag) AS (SELECT 7, 1::BIGINT, 'anchor' UNION "
                       "SELECT c.a, t.n, 'arm' FROM t, c WHERE t.k = c.link) SELECT * FROM c")
    assert ("7", "1", "anchor") in rows and ("7", "1", "arm") in rows


def test_a_varchar_carried_column(db):
    compare(db, "WITH RECURSIVE c(name, link) AS (SELECT p_firstname, p_personid FROM person WHERE p_personid % 11 = 0 "
                "UNION SELECT c.name, k.k_person2id FROM knows k, c WHERE k.k_person1id = c.link) SELECT * FROM c")


def test_an_empty_anchor_and_an_empty_table(db):
    compare(db, _reach("SELECT p_personid FROM person WHERE p_personid < 0"), nonempty=False)
    compare(db, "WITH RECURSIVE c(a, link) AS (SELECT * FROM (VALUES (1, 1::BIGINT), (1, 1), (2, NULL)) v UNION "
                "SELECT c.a, e.n FROM empty_t e, c WHERE e.k = c.link) SELECT * FROM c")


def test_a_prepared_statement_executed_twice(db):
    """planned once with the rules on, executed three times: each execution sinks the tables and runs the closure anew.
    (The rules-off side runs the statement unprepared: the reference's own PhysicalRecursiveCTE keeps the pipelines of a
    prepared plan's first execution and does not survive a second one.)"""
    sql = ("WITH RECURSIVE c(a, link) AS (SELECT 1, {}::BIGINT UNION SELECT c.a, t.n FROM t, c WHERE t.k = c.link) "
           "SELECT * FROM c")
    _off(db)
    cpu = [db.query_text(sql.format(v)) for v in (1, 5, 1)]
    _on(db)
    try:
        db.execute(f"PREPARE gpu_q AS {sql.format('?')}")
        assert REACH in db.explain(sql.format(1))
        gpu = [db.query_text(f"EXECUTE gpu_q({v})") for v in (1, 5, 1)]
        db.execute("DEALLOCATE gpu_q")
    finally:
        _off(db)
    assert all(len(c) > 1 for c in cpu)
    for g, c in zip(gpu, cpu):
        assert sorted(g, key=_key) == sorted(c, key=_key)


def test_seeded_random_statements(db):
    """random tables (small id domains: cycles, self-loops, duplicates, NULLs) and random arms of the accepted shape"""
    rng = np.random.default_rng(2026)
    for case in range(12):
        n_rows = int(rng.integers(0, 60))
        dom = int(rng.integers(3, 25))
        vals = []
        for _ in range(n_rows):
            k = "NULL" if rng.random() < 0.08 else str(int(rng.integers(0, dom)))
            n = "NULL" if rng.random() < 0.08 else str(int(rng.integers(0, dom)))
            vals.append(f"({k}, {n}, 'p{int(rng.integers(0, 3))}')")
        db.execute("DROP TABLE IF EXISTS rt")
        db.execute("CREATE TABLE rt (k INTEGER, n INTEGER, s VARCHAR)")
        if vals:
            db.execute("INSERT INTO rt VALUES " + ", ".join(vals))
        n_anchor = int(rng.integers(0, 8))
        with_tag = bool(rng.integers(0, 2))
        anchor = []
        for _ in range(n_anchor):
            link = "NULL" if rng.random() < 0.15 else str(int(rng.integers(-1, dom + 1)))
            row = [f"'c{int(rng.integers(0, 3))}'", f"{link}::INTEGER"]
            if with_tag:
                row.append(f"'{'arm' if rng.random() < 0.6 else 'anc'}'")
            anchor.append("(" + ", ".join(row) + ")")
        cols = "cls, link" + (", tag" if with_tag else "")
        if anchor:
            anchor_sql = f"SELECT * FROM (VALUES {', '.join(anchor)}) v"
        else:
            anchor_sql = "SELECT 'c0', 1::INTEGER" + (", 'arm'" if with_tag else "") + " WHERE false"
        arm = "SELECT c.cls, rt.n" + (", 'arm'" if with_tag else "") + " FROM rt, c WHERE rt.k = c.link"
        sql = f"WITH RECURSIVE c({cols}) AS ({anchor_sql} UNION {arm}) SELECT * FROM c"
        compare(db, sql, nonempty=False)
