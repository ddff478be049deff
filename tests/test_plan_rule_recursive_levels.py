"""UNION recursive CTEs with a depth counter over one keyed table (the friends CTE of bi-10-shortestpath.sql under any
consumer but the shortest-path rule's min) are planned as GG_RECURSIVE_LEVELS (gg_plan_rule.cpp, PlanRecursiveWalks;
gg_recursive_levels.cpp) when the connection issued PRAGMA enable_gpu_recursive_levels next to enable_gpu_graph; without
it, and for shapes the level sets do not compute exactly, the reference's PhysicalRecursiveCTE stays.  EXPLAIN only:
nothing here touches a GPU (the GPU suite compares the results, tests/test_gpu_recursive_levels_sql.py)."""
import os
import subprocess
import sys

import pytest

from oracle import ref_duckdb as R
from tests.test_plan_rule import _ldbc_database, _ldbc_texts

EXT = R.EXTENSION

pytestmark = pytest.mark.skipif(
    not (R.available() and os.path.exists(EXT) and R.rules_route() == "shim"),
    reason="reference build / extension / interposition shim not present (the call-outs of a patched reference have no recursive-CTE call-out)")

LEVELS = "GG_RECURSIVE_LEVELS"

SCHEMA = ["CREATE TABLE t (k BIGINT, n BIGINT, pay VARCHAR, f DOUBLE)", "CREATE TABLE u (x BIGINT, y BIGINT)"]


@pytest.fixture(scope="module")
def db():
    d = R.RefDuckDB(threads=2)
    for ddl in SCHEMA:
        d.execute(ddl)
    d.execute("INSERT INTO t VALUES (1, 2, 'a', 0.5), (2, 3, 'b', 1.5), (3, 1, 'c', 2.5), (NULL, 1, 'd', 3.5)")
    d.execute("INSERT INTO u VALUES (2, 2), (3, 3)")
    d.execute(f"LOAD '{EXT}'")
    d.execute("PRAGMA enable_gpu_graph")
    d.execute("PRAGMA enable_gpu_recursive_levels")
    yield d
    d.close()


# (name -> (statement, max_levels in the plan or None))
ACCEPTED = {
    "counter plus link": ("WITH RECURSIVE c(hop, link) AS (SELECT 0, 1::BIGINT UNION "
                          "SELECT c.hop + 1, t.n FROM t, c WHERE t.k = c.link AND c.hop < 4) SELECT * FROM c", 4),
    "carried plus counter plus link": ("WITH RECURSIVE c(a, hop, link) AS (SELECT 7::BIGINT, 0, 1::BIGINT UNION "
                                       "SELECT c.a, c.hop + 1, t.n FROM t, c WHERE t.k = c.link AND c.hop < 3) "
                                       "SELECT * FROM c", 3),
    "constants": ("WITH RECURSIVE c(a, hop, link, tag) AS (SELECT 7::BIGINT, 0, 1::BIGINT, 'anchor' UNION "
                  "SELECT c.a, c.hop + 1, t.n, 'arm' FROM t, c WHERE t.k = c.link) SELECT * FROM c", None),
    # (the arm does not read `tag`, so the optimizer projects the CTE's other columns above the bound's filter)
    "constants with a bound": ("WITH RECURSIVE c(a, hop, link, tag) AS (SELECT 7::BIGINT, 0, 1::BIGINT, 'anchor' UNION "
                               "SELECT c.a, c.hop + 1, t.n, 'arm' FROM t, c WHERE t.k = c.link AND c.hop < 3) "
                               "SELECT * FROM c", 3),
    "<=": ("WITH RECURSIVE c(hop, link) AS (SELECT 0, 1::BIGINT UNION "
           "SELECT c.hop + 1, t.n FROM t, c WHERE t.k = c.link AND c.hop <= 4) SELECT * FROM c", 5),
    "step 2": ("WITH RECURSIVE c(hop, link) AS (SELECT 1, 1::BIGINT UNION "
               "SELECT c.hop + 2, t.n FROM t, c WHERE t.k = c.link AND c.hop < 8) SELECT * FROM c", 4),
    "two counters": ("WITH RECURSIVE c(hop, link, twice) AS (SELECT 0, 1::BIGINT, 10::BIGINT UNION "
                     "SELECT c.hop + 1, t.n, c.twice + 2 FROM t, c WHERE t.k = c.link AND c.hop < 6 AND c.twice < 16) "
                     "SELECT * FROM c", 3),
    "no bound": ("WITH RECURSIVE c(hop, link) AS (SELECT 0, 1::BIGINT UNION "
                 "SELECT c.hop + 1, t.n FROM t, c WHERE t.k = c.link) SELECT * FROM c", None),
}

DECLINED = {
    "second column of the table": ("WITH RECURSIVE c(hop, link, p) AS (SELECT 0, 1::BIGINT, 'x' UNION "
                                   "SELECT c.hop + 1, t.n, t.pay FROM t, c WHERE t.k = c.link AND c.hop < 3) "
                                   "SELECT * FROM c", "UNION: a column of the table other than the next link"),
    "carried column moved": ("WITH RECURSIVE c(a, b, hop, link) AS (SELECT 7::BIGINT, 8::BIGINT, 0, 1::BIGINT UNION "
                             "SELECT c.b, c.a, c.hop + 1, t.n FROM t, c WHERE t.k = c.link AND c.hop < 3) "
                             "SELECT * FROM c", "a CTE column moves to another position"),
    "two tables": ("WITH RECURSIVE c(hop, link) AS (SELECT 0, 1::BIGINT UNION "
                   "SELECT c.hop + 1, t.n FROM t, c, u WHERE t.k = c.link AND u.x = t.n AND c.hop < 3) SELECT * FROM c",
                   None),
    "non-integer link": ("WITH RECURSIVE c(hop, link) AS (SELECT 0, 0.5::DOUBLE UNION "
                         "SELECT c.hop + 1, t.f FROM t, c WHERE t.f = c.link AND c.hop < 3) SELECT * FROM c",
                         "link or key is not an integer column"),
    "step 0": ("WITH RECURSIVE c(hop, link) AS (SELECT 0, 1::BIGINT UNION "
               "SELECT c.hop + 0, t.n FROM t, c WHERE t.k = c.link) SELECT * FROM c", None),
    "negative step": ("WITH RECURSIVE c(hop, link) AS (SELECT 0, 1::BIGINT UNION "
                      "SELECT c.hop + (-1), t.n FROM t, c WHERE t.k = c.link AND c.hop < 3) SELECT * FROM c",
                      "UNION: a depth counter whose step is not positive"),
    "another predicate": ("WITH RECURSIVE c(a, hop, link) AS (SELECT 7::BIGINT, 0, 1::BIGINT UNION "
                          "SELECT c.a, c.hop + 1, t.n FROM t, c WHERE t.k = c.link AND c.hop < 3 AND c.a <> 3) "
                          "SELECT * FROM c", "a CTE-side predicate other than counter < K"),
    "counter anchor not a constant": ("WITH RECURSIVE c(hop, link) AS (SELECT k, n FROM t UNION "
                                      "SELECT c.hop + 1, t.n FROM t, c WHERE t.k = c.link) SELECT * FROM c",
                                      "a counter whose anchor value is not a constant"),
    "counter overflows within the bound": ("WITH RECURSIVE c(hop, link) AS (SELECT 100::TINYINT, 1::BIGINT UNION "
                                           "SELECT c.hop + 10::TINYINT, t.n FROM t, c WHERE t.k = c.link AND c.hop < 125::TINYINT) "
                                           "SELECT * FROM c", "UNION: a depth counter that overflows its type"),
}

BI10_FRIENDS = """WITH RECURSIVE friends(startPerson, hopCount, friend) AS (
    SELECT p_personid, 0, p_personid
      FROM person
     WHERE 1=1
       AND p_personid = 19791209310731
  UNION
    SELECT f.startPerson
         , f.hopCount+1
         , CASE WHEN f.friend = k.k_person1id then k.k_person2id ELSE k.k_person1id END
      FROM friends f
         , knows k
     WHERE 1=1
        -- join
       AND f.friend = k.k_person1id -- note, that knows table have both (p1, p2) and (p2, p1)
        -- filter
        -- stop condition
       AND f.hopCount < 5
)
"""
BI10_CONSUMERS = ["SELECT * FROM friends", "SELECT hopCount, count(*) FROM friends GROUP BY hopCount"]


def _bi10():
    return _ldbc_texts()["queries"]["bi-10-shortestpath.sql"].strip().rstrip(";")


@pytest.mark.parametrize("name", sorted(ACCEPTED))
def test_accepted_shapes(db, name):
    plan = db.explain(ACCEPTED[name][0])
    assert LEVELS in plan and "REC_CTE" not in plan, plan
    assert "GG_RECURSIVE_WALKS" not in plan and "GG_RECURSIVE_REACH" not in plan, plan


@pytest.mark.parametrize("name", sorted(ACCEPTED))
def test_max_levels_in_the_plan(db, name):
    sql, max_levels = ACCEPTED[name]
    plan = " ".join(db.explain(sql).replace("│", " ").split())
    if max_levels is None:
        assert "max_levels" not in plan, plan
    else:
        assert f"max_levels={max_levels} " in plan + " ", plan


def test_the_bi10_friends_cte_is_the_shipped_text():
    assert BI10_FRIENDS.strip() in _bi10()


@pytest.mark.parametrize("consumer", BI10_CONSUMERS)
def test_bi10_friends_under_other_consumers(consumer):
    d = _ldbc_database(populated=True)
    try:
        d.execute("PRAGMA enable_gpu_graph")
        d.execute("PRAGMA enable_gpu_recursive_levels")
        plan = d.explain(BI10_FRIENDS + consumer)
        assert LEVELS in plan and "REC_CTE" not in plan and "max_levels=5" in plan, plan
        d.execute("PRAGMA disable_gpu_recursive_levels")
        plan = d.explain(BI10_FRIENDS + consumer)
        assert LEVELS not in plan and "REC_CTE" in plan, plan
    finally:
        d.close()


@pytest.mark.parametrize("name", sorted(ACCEPTED))
def test_without_the_pragma_the_reference_plan_stays(db, name):
    db.execute("PRAGMA disable_gpu_recursive_levels")
    try:
        plan = db.explain(ACCEPTED[name][0])
        db.execute("PRAGMA enable_gpu_recursive_union")  # the other UNION switch does not take the shape either
        plan_union = db.explain(ACCEPTED[name][0])
    finally:
        db.execute("PRAGMA disable_gpu_recursive_union")
        db.execute("PRAGMA enable_gpu_recursive_levels")
    for p in (plan, plan_union):
        assert LEVELS not in p and "GG_RECURSIVE_REACH" not in p and "REC_CTE" in p, p


def test_the_pragma_needs_enable_gpu_graph(db):
    db.execute("PRAGMA disable_gpu_graph")
    try:
        plan = db.explain(ACCEPTED["counter plus link"][0])
    finally:
        db.execute("PRAGMA enable_gpu_graph")
    assert LEVELS not in plan and "REC_CTE" in plan, plan


@pytest.mark.parametrize("name", sorted(DECLINED))
def test_declined_shapes_keep_the_reference_plan(db, name):
    plan = db.explain(DECLINED[name][0])
    assert LEVELS not in plan and "REC_CTE" in plan, plan


def test_union_all_with_a_counter_still_plans_the_walk_closure(db):
    sql = ACCEPTED["carried plus counter plus link"][0].replace(" UNION ", " UNION ALL ")
    plan = db.explain(sql)
    assert "GG_RECURSIVE_WALKS" in plan and LEVELS not in plan and "REC_CTE" not in plan, plan


def test_union_without_a_counter_still_plans_the_reach_closure(db):
    sql = ("WITH RECURSIVE c(a, link) AS (SELECT 7::BIGINT, 1::BIGINT UNION SELECT c.a, t.n FROM t, c WHERE t.k = c.link) "
           "SELECT * FROM c")
    plan = db.explain(sql)  # only the levels switch is on: the shape is reachability's
    assert LEVELS not in plan and "GG_RECURSIVE_REACH" not in plan and "REC_CTE" in plan, plan
    db.execute("PRAGMA enable_gpu_recursive_union")
    try:
        plan = db.explain(sql)
    finally:
        db.execute("PRAGMA disable_gpu_recursive_union")
    assert "GG_RECURSIVE_REACH" in plan and LEVELS not in plan and "REC_CTE" not in plan, plan


def test_shipped_bi10_still_plans_the_shortest_path_bfs():
    d = _ldbc_database(populated=True)
    try:
        for pragma in ("enable_gpu_graph", "enable_gpu_recursive_union", "enable_gpu_recursive_levels"):
            d.execute("PRAGMA " + pragma)
        plan = d.explain(_bi10())  # (a plan this wide cuts its operators' names short)
        assert "GG_SHORTEST_PA" in plan and "GG_RECURSIVE" not in plan and "REC_CTE" not in plan, plan
    finally:
        d.close()


_TRACE = r"""
import sys
from oracle import ref_duckdb as R
d = R.RefDuckDB(threads=1)
for ddl in sys.argv[2].split(";"):
    d.execute(ddl)
d.execute("LOAD '" + R.EXTENSION + "'")
d.execute("PRAGMA enable_gpu_graph")
for pragma in sys.argv[1].split():
    d.execute("PRAGMA " + pragma)
for sql in sys.argv[3:]:
    d.explain(sql)
d.close()
"""


def _trace(pragmas, sqls):
    env = dict(os.environ, GG_RULE_TRACE="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", _TRACE, pragmas, ";".join(SCHEMA)] + sqls, env=env, cwd=root,
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return out.stderr


def test_declines_are_named_in_the_rule_trace():
    for name, (sql, why) in sorted(DECLINED.items()):
        err = _trace("enable_gpu_recursive_levels", [sql])
        assert "[gg] recursive walks declined: " in err, (name, err)
        if why is not None:
            assert why in err, (name, err)


def test_with_the_pragma_off_the_trace_still_names_the_depth_counter():
    for name, (sql, _) in sorted(ACCEPTED.items()):
        err = _trace("enable_gpu_recursive_union", [sql])
        if name == "constants with a bound":  # without the switch the projected CTE side ends the parse before the counter
            assert "the join does not scan the CTE directly" in err, (name, err)
        else:
            assert "UNION: a depth counter (its rows differ per level)" in err, (name, err)
