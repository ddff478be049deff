"""UNION recursive CTEs over one keyed table (reachability; interactive-complex-12.sql's extended_tags) are planned as
GG_RECURSIVE_REACH (gg_plan_rule.cpp, PlanRecursiveWalks; gg_recursive_reach.cpp) when the connection issued
PRAGMA enable_gpu_recursive_union next to enable_gpu_graph; without it, and for shapes the reachability closure does not
compute exactly, the reference's PhysicalRecursiveCTE stays.  EXPLAIN only: nothing here touches a GPU (the GPU suite
compares the results, tests/test_gpu_recursive_union_sql.py)."""
import os
import subprocess
import sys

import pytest

from oracle import ref_duckdb as R
from tests.test_plan_rule import _ldbc_database, _ldbc_texts
from tests.test_plan_rule_union_all import DECLINED as UNION_ALL_DECLINED

EXT = R.EXTENSION

pytestmark = pytest.mark.skipif(
    not (R.available() and os.path.exists(EXT) and R.rules_route() == "shim"),
    reason="reference build / extension / interposition shim not present (the call-outs of a patched reference have no recursive-CTE call-out)")

REACH = "GG_RECURSIVE_REACH"


@pytest.fixture(scope="module")
def db():
    d = R.RefDuckDB(threads=2)
    d.execute("CREATE TABLE t (k BIGINT, n BIGINT, pay VARCHAR, f DOUBLE)")
    d.execute("CREATE TABLE u (x BIGINT, y BIGINT)")
    d.execute("INSERT INTO t VALUES (1, 2, 'a', 0.5), (2, 3, 'b', 1.5), (3, 1, 'c', 2.5), (NULL, 1, 'd', 3.5)")
    d.execute("INSERT INTO u VALUES (2, 2), (3, 3)")
    d.execute(f"LOAD '{EXT}'")
    d.execute("PRAGMA enable_gpu_graph")
    d.execute("PRAGMA enable_gpu_recursive_union")
    yield d
    d.close()


ACCEPTED = {
    "reach(x)": "WITH RECURSIVE reach(p) AS (SELECT 1::BIGINT UNION SELECT t.n FROM reach r, t WHERE r.p = t.k) "
                "SELECT * FROM reach",
    "carried plus link": "WITH RECURSIVE c(a, link) AS (SELECT 7::BIGINT, 1::BIGINT UNION "
                         "SELECT c.a, t.n FROM t, c WHERE t.k = c.link) SELECT * FROM c",
    "constants": "WITH RECURSIVE c(a, link, tag) AS (SELECT 7::BIGINT, 1::BIGINT, 'anchor' UNION "
                 "SELECT c.a, t.n, 'arm' FROM t, c WHERE t.k = c.link) SELECT * FROM c",
    "UNION ALL's declined UNION shape": UNION_ALL_DECLINED["UNION without ALL"],
}

DECLINED = {
    "depth counter": "WITH RECURSIVE c(hop, link) AS (SELECT 0, 1::BIGINT UNION "
                     "SELECT c.hop + 1, t.n FROM t, c WHERE t.k = c.link) SELECT * FROM c",
    "second column of the table": "WITH RECURSIVE c(link, p) AS (SELECT 1::BIGINT, 'x' UNION "
                                  "SELECT t.n, t.pay FROM t, c WHERE t.k = c.link) SELECT * FROM c",
    "carried column moved": "WITH RECURSIVE c(a, b, link) AS (SELECT 7::BIGINT, 8::BIGINT, 1::BIGINT UNION "
                            "SELECT c.b, c.a, t.n FROM t, c WHERE t.k = c.link) SELECT * FROM c",
    "two tables": "WITH RECURSIVE c(a, link) AS (SELECT 7::BIGINT, 1::BIGINT UNION "
                  "SELECT c.a, t.n FROM t, c, u WHERE t.k = c.link AND u.x = t.n) SELECT * FROM c",
    "non-counter CTE predicate": "WITH RECURSIVE c(a, link) AS (SELECT 7::BIGINT, 1::BIGINT UNION "
                                 "SELECT c.a, t.n FROM t, c WHERE t.k = c.link AND c.a <> 3) SELECT * FROM c",
    "non-integer link": "WITH RECURSIVE c(a, link) AS (SELECT 7::BIGINT, 0.5::DOUBLE UNION "
                        "SELECT c.a, t.f FROM t, c WHERE t.f = c.link) SELECT * FROM c",
}


def _ic12():
    return _ldbc_texts()["queries"]["interactive-complex-12.sql"].strip().rstrip(";")


@pytest.mark.parametrize("name", sorted(ACCEPTED))
def test_accepted_shapes(db, name):
    plan = db.explain(ACCEPTED[name])
    assert REACH in plan and "REC_CTE" not in plan, plan
    assert "GG_RECURSIVE_WALKS" not in plan, plan


def test_parameters_in_the_plan(db):
    plan = db.explain(ACCEPTED["carried plus link"])
    assert "link=#1 key=#1 next=#0" in plan, plan  # (the table's scan projects n, k)


@pytest.mark.parametrize("name", sorted(ACCEPTED))
def test_without_the_pragma_the_reference_plan_stays(db, name):
    db.execute("PRAGMA disable_gpu_recursive_union")
    try:
        plan = db.explain(ACCEPTED[name])
    finally:
        db.execute("PRAGMA enable_gpu_recursive_union")
    assert REACH not in plan and "REC_CTE" in plan, plan


def test_the_pragma_needs_enable_gpu_graph(db):
    db.execute("PRAGMA disable_gpu_graph")
    try:
        plan = db.explain(ACCEPTED["reach(x)"])
    finally:
        db.execute("PRAGMA enable_gpu_graph")
    assert REACH not in plan and "REC_CTE" in plan, plan


@pytest.mark.parametrize("name", sorted(DECLINED))
def test_declined_shapes_keep_the_reference_plan(db, name):
    plan = db.explain(DECLINED[name])
    assert REACH not in plan and "REC_CTE" in plan, plan


def test_union_all_still_plans_the_walk_closure(db):
    sql = ACCEPTED["carried plus link"].replace(" UNION ", " UNION ALL ")
    plan = db.explain(sql)
    assert "GG_RECURSIVE_WALKS" in plan and REACH not in plan and "REC_CTE" not in plan, plan


def test_shipped_interactive_complex_12():
    """the shipped text, over the LDBC schema with the populated rows of tests/ldbc_shapes.py"""
    d = _ldbc_database(populated=True)
    try:
        d.execute("PRAGMA enable_gpu_graph")
        d.execute("PRAGMA enable_gpu_recursive_union")
        plan = d.explain(_ic12())
        assert REACH in plan and "REC_CTE" not in plan, plan
        d.execute("PRAGMA disable_gpu_recursive_union")
        plan = d.explain(_ic12())
        assert REACH not in plan and "REC_CTE" in plan, plan
    finally:
        d.close()


_TRACE = r"""
import sys
from oracle import ref_duckdb as R
d = R.RefDuckDB(threads=1)
d.execute("CREATE TABLE t (k BIGINT, n BIGINT, pay VARCHAR, f DOUBLE)")
d.execute("LOAD '" + R.EXTENSION + "'")
d.execute("PRAGMA enable_gpu_graph")
d.execute("PRAGMA enable_gpu_recursive_union")
for sql in sys.argv[1:]:
    d.explain(sql)
d.close()
"""


def test_declines_are_named_in_the_rule_trace():
    env = dict(os.environ, GG_RULE_TRACE="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sqls = [DECLINED["depth counter"], DECLINED["second column of the table"], DECLINED["non-counter CTE predicate"]]
    out = subprocess.run([sys.executable, "-c", _TRACE] + sqls, env=env, cwd=root, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    for why in ("UNION: a depth counter", "UNION: a column of the table other than the next link",
                "UNION: a CTE-side predicate"):
        assert why in out.stderr, out.stderr
