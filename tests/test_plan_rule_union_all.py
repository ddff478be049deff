"""UNION ALL recursive CTEs over one keyed table (bi-9.sql post_all, interactive-short-6.sql chain) are planned as
GG_RECURSIVE_WALKS (gg_plan_rule.cpp, PlanRecursiveWalks); shapes the walk closure does not compute exactly keep the
reference's PhysicalRecursiveCTE.  EXPLAIN only: nothing here touches a GPU (the GPU suite compares the results,
tests/test_gpu_recursive_walks_sql.py)."""
import os

import pytest

from oracle import ref_duckdb as R
from tests.test_plan_rule import _ldbc_database, _ldbc_texts

EXT = R.EXTENSION

pytestmark = pytest.mark.skipif(
    not (R.available() and os.path.exists(EXT) and R.rules_route() == "shim"),
    reason="reference build / extension / interposition shim not present (the call-outs of a patched reference have no recursive-CTE call-out)")

WALKS = "GG_RECURSIVE_WALKS"


@pytest.fixture(scope="module")
def db():
    d = R.RefDuckDB(threads=2)
    d.execute("CREATE TABLE t (k BIGINT, n BIGINT, pay VARCHAR)")
    d.execute("CREATE TABLE u (x BIGINT, y BIGINT)")
    d.execute("INSERT INTO t VALUES (1, 2, 'a'), (2, 3, 'b'), (3, NULL, 'c'), (NULL, 1, 'd')")
    d.execute("INSERT INTO u VALUES (2, 2), (3, 3)")
    d.execute("CREATE TABLE e (a BIGINT NOT NULL, b BIGINT NOT NULL)")
    d.execute("INSERT INTO e VALUES (1, 2), (2, 3), (3, 4), (2, 5)")
    d.execute(f"LOAD '{EXT}'")
    d.execute("PRAGMA enable_gpu_graph")
    yield d
    d.close()


def test_shipped_bi9_and_interactive_short6_get_the_walk_closure():
    """the shipped texts, over the LDBC schema with the populated rows of tests/ldbc_shapes.py"""
    d = _ldbc_database(populated=True)
    try:
        d.execute("PRAGMA enable_gpu_graph")
        for name in ("bi-9.sql", "interactive-short-6.sql"):
            plan = d.explain(_ldbc_texts()["queries"][name].strip().rstrip(";"))
            assert WALKS in plan, (name, plan)
            assert "REC_CTE" not in plan, name
        d.execute("PRAGMA disable_gpu_graph")
        assert WALKS not in d.explain(_ldbc_texts()["queries"]["bi-9.sql"].strip().rstrip(";"))
    finally:
        d.close()


ACCEPTED = {
    "carried, table column, constant": "WITH RECURSIVE c(a, link, p) AS (SELECT 7::BIGINT, 1::BIGINT, 'x' UNION ALL "
                                       "SELECT c.a, t.n, 'y' FROM t, c WHERE t.k = c.link) SELECT * FROM c",
    "depth counter with a bound": "WITH RECURSIVE c(a, hop, link) AS (SELECT 7::BIGINT, 0, 1::BIGINT UNION ALL "
                                  "SELECT c.a, c.hop + 1, t.n FROM t, c WHERE t.k = c.link AND c.hop < 5) SELECT * FROM c",
    "table on the other side": "WITH RECURSIVE c(link, p) AS (SELECT k, pay FROM t WHERE k = 1 UNION ALL "
                               "SELECT t.n, t.pay FROM c, t WHERE c.link = t.k) SELECT count(*) FROM c",
}

DECLINED = {
    "arm joins two tables": "WITH RECURSIVE c(a, link) AS (SELECT 7::BIGINT, 1::BIGINT UNION ALL "
                            "SELECT c.a, t.n FROM t, c, u WHERE t.k = c.link AND u.x = t.n) SELECT * FROM c",
    "carried column moved": "WITH RECURSIVE c(a, b, link) AS (SELECT 7::BIGINT, 8::BIGINT, 1::BIGINT UNION ALL "
                            "SELECT c.b, c.a, t.n FROM t, c WHERE t.k = c.link) SELECT * FROM c",
    "non-counter CTE predicate": "WITH RECURSIVE c(a, link) AS (SELECT 7::BIGINT, 1::BIGINT UNION ALL "
                                 "SELECT c.a, t.n FROM t, c WHERE t.k = c.link AND c.a <> 3) SELECT * FROM c",
    "counter bound on a non-constant start": "WITH RECURSIVE c(hop, link) AS (SELECT k, n FROM t WHERE k = 1 UNION ALL "
                                             "SELECT c.hop + 1, t.n FROM t, c WHERE t.k = c.link AND c.hop < 5) "
                                             "SELECT * FROM c",
    "next link is not a table column": "WITH RECURSIVE c(a, link) AS (SELECT 7::BIGINT, 1::BIGINT UNION ALL "
                                       "SELECT c.a, c.link + 1 FROM t, c WHERE t.k = c.link) SELECT * FROM c",
    "UNION without ALL": "WITH RECURSIVE c(a, link) AS (SELECT 7::BIGINT, 1::BIGINT UNION "
                         "SELECT c.a, t.n FROM t, c WHERE t.k = c.link) SELECT * FROM c",
}


@pytest.mark.parametrize("name", sorted(ACCEPTED))
def test_accepted_shapes(db, name):
    plan = db.explain(ACCEPTED[name])
    assert WALKS in plan and "REC_CTE" not in plan, plan


def test_counter_bound_becomes_max_levels(db):
    assert "max_levels=5" in db.explain(ACCEPTED["depth counter with a bound"])
    le = ACCEPTED["depth counter with a bound"].replace("c.hop < 5", "c.hop <= 5")
    assert "max_levels=6" in db.explain(le)


@pytest.mark.parametrize("name", sorted(DECLINED))
def test_declined_shapes_keep_the_reference_plan(db, name):
    plan = db.explain(DECLINED[name])
    assert WALKS not in plan and "REC_CTE" in plan, plan


# subplans under the walk sinks are planned with every gg rule suspended: their pipelines are built by the reference's
# own traversal, which knows no graph scan with sinks of its own
NESTED = {
    "anchor another rule would take": "WITH RECURSIVE r(id) AS (SELECT e2.b FROM e e1, e e2 WHERE e1.a = 1 AND "
                                      "e1.b = e2.a UNION ALL SELECT t.n FROM t, r WHERE t.k = r.id) SELECT * FROM r",
    "chained pair of recursive CTEs": "WITH RECURSIVE a(id) AS (SELECT 1::BIGINT UNION ALL SELECT t.n FROM t, a "
                                      "WHERE t.k = a.id), b(id) AS (SELECT id FROM a UNION ALL SELECT t.n FROM t, b "
                                      "WHERE t.k = b.id) SELECT * FROM b",
}


def test_the_anchor_alone_is_a_walk_plan(db):
    assert "GG_PATH_EXPAND" in db.explain("SELECT e2.b FROM e e1, e e2 WHERE e1.a = 1 AND e1.b = e2.a")


@pytest.mark.parametrize("name", sorted(NESTED))
def test_subplans_under_the_walk_sinks_keep_the_reference_operators(db, name):
    plan = db.explain(NESTED[name])
    names = [w for w in plan.split() if w.startswith("GG_")]
    assert names.count(WALKS) == 1 and set(names) == {WALKS, "GG_WALK_ANCHOR_SINK", "GG_WALK_TABLE_SINK"}, plan
    assert ("REC_CTE" in plan) == name.startswith("chained"), plan
