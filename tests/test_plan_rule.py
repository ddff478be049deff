"""Planner rules (duckdb_pgq_amd/host/gg_plan_rule.cpp), CPU part: which logical plans of the compiled
reference are taken over and which are left alone.  Only EXPLAIN is used here — planning touches no GPU
(the scans open at execution time); result parity of the substituted plans is in
tests/test_duckdb_extension.py (-m gpu).  Needs oracle/_ref (the compiled reference), the extension and
the interposition shim, all built by __graft_entry__.build() where /root/reference exists."""
import json
import os

import pytest

from oracle import ref_duckdb as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT = R.EXTENSION  # (the build that goes with the reference variant under test: oracle/ref_duckdb.py)

pytestmark = pytest.mark.skipif(
    not (R.available() and os.path.exists(EXT) and bool(R.rules_route())),
    reason="reference build / extension / plan hook not present")


@pytest.fixture(scope="module")
def db():
    d = R.RefDuckDB(threads=2)
    d.execute("CREATE TABLE person (p_personid BIGINT PRIMARY KEY)")
    d.execute("CREATE TABLE person_nokey (p_personid BIGINT NOT NULL)")
    d.execute("CREATE TABLE knows (k_person1id BIGINT NOT NULL, k_person2id BIGINT NOT NULL, k_weight INTEGER)")
    d.execute("CREATE TABLE knows_nullable (a BIGINT, b BIGINT)")
    d.execute("CREATE TABLE e32 (a INTEGER NOT NULL, b INTEGER NOT NULL)")
    d.execute("INSERT INTO person VALUES (1), (2), (3)")
    d.execute("INSERT INTO knows VALUES (1, 2, 1), (2, 3, 2), (3, 1, 3)")
    # (statistics propagation turns joins over empty tables into EMPTY_RESULT before any rule sees them)
    d.execute("INSERT INTO person_nokey VALUES (1), (2), (3)")
    d.execute("INSERT INTO knows_nullable VALUES (1, 2), (2, 3), (3, NULL)")
    d.execute("INSERT INTO e32 VALUES (1, 2), (2, 3), (3, 1)")
    d.execute(f"LOAD '{EXT}'")
    yield d
    d.execute("PRAGMA disable_gpu_graph")
    d.close()


def chain(h, table="knows", a="k_person1id", b="k_person2id", select="count(*)"):
    frm = ", ".join(f"{table} k{i}" for i in range(1, h + 1))
    cond = " AND ".join(f"k{i}.{b} = k{i+1}.{a}" for i in range(1, h))
    return f"SELECT {select} FROM {frm} WHERE {cond}"


TAKEN = [
    # count(*) of ONE equi-join on an integer key that is not a walk (common neighbour, same-source fan, two tables):
    # the build side's degrees summed over the probe side's keys (test/sql/join/inner/test_join_duplicates.test)
    ("SELECT count(*) FROM knows k1, knows k2 WHERE k1.k_person2id = k2.k_person2id", "GG_JOIN_COUNT", "1 hop"),
    ("SELECT count(*) FROM knows k1, knows k2 WHERE k1.k_person1id = k2.k_person1id", "GG_JOIN_COUNT", "1 hop"),
    ("SELECT count(*) FROM person p JOIN knows k ON p.p_personid = k.k_person2id", "GG_JOIN_COUNT", "1 hop"),
    (chain(2, table="knows_nullable", a="a", b="b"), "GG_JOIN_COUNT", "1 hop"),
    # edge-only chains (interactive-complex-3.sql:9-11 idiom)
    (chain(2), "GG_PATH_COUNT", "2 hops"),
    (chain(4), "GG_PATH_COUNT", "4 hops"),
    (chain(3, select="k1.k_person1id, k3.k_person2id"), "GG_PATH_EXPAND", "3 hops"),
    (chain(2, table="e32", a="a", b="b", select="k1.a, k2.b"), "GG_PATH_EXPAND", "2 hops"),
    # the far end written first: the walk is read in the other direction
    ("SELECT count(*) FROM knows k1, knows k2 WHERE k2.k_person1id = k1.k_person2id", "GG_PATH_COUNT", "2 hops"),
    # vertex-validated chains (the oracle's SQL formulation, oracle/ref_duckdb.py sql_khop)
    (R.sql_khop(1), "GG_PATH_COUNT", "vertices: person.p_personid"),
    (R.sql_khop(2), "GG_PATH_COUNT", "vertices: person.p_personid"),
    (R.sql_khop_rows(2), "GG_PATH_EXPAND", "2 hops"),
    # a predicate on an edge instance's payload column: evaluated above the rows fetched by rowid
    ("SELECT k1.k_weight FROM knows k1, knows k2 WHERE k1.k_person2id = k2.k_person1id AND k2.k_weight > 1",
     "GG_PATH_EDGES", "2 hops"),
    ("SELECT k2.k_person2id FROM knows k1, knows k2 WHERE k1.k_person2id = k2.k_person1id AND k1.k_weight = 2 "
     "AND k1.k_person1id = 2", "GG_PATH_EDGES", "2 hops"),
    # payload columns of the edge instances: the walks come with their edges' rowids, the columns by rowid
    (chain(2, select="k1.k_weight"), "GG_PATH_EDGES", "with 1 edge column by rowid"),
    (chain(3, select="k1.k_person1id, k1.k_weight, k3.k_weight, k3.k_person2id, k1.k_weight"), "GG_PATH_EDGES",
     "with 2 edge columns by rowid"),
    (chain(2, select="k2.k_weight") + " AND k1.k_person1id = 2", "GG_PATH_EDGES", "from 2"),
    # single source pinned by a constant
    (chain(2, select="k2.k_person2id") + " AND k1.k_person1id = 2", "GG_PATH_EXPAND", "from 2"),
    (chain(2) + " AND k2.k_person2id = 3", "GG_PATH_COUNT", "from 3"),
    # predicates on other walk positions stay as a filter above the GPU scan (interactive-complex-3.sql:9-11:
    # `k1.k_person1id = C and k1.k_person2id = k2.k_person1id and k2.k_person2id <> X`)
    (chain(2, select="k2.k_person2id") + " AND k1.k_person1id = 2 AND k2.k_person2id <> 1", "GG_PATH_EXPAND", "from 2"),
    (chain(2) + " AND k1.k_person1id > 2", "GG_PATH_EXPAND", "2 hops"),
    (chain(2) + " AND k2.k_person1id = 2", "GG_PATH_EXPAND", "2 hops"),
    (chain(3, select="k3.k_person2id") + " AND k1.k_person1id = 1 AND k3.k_person2id = 1", "GG_PATH_EXPAND", "3 hops"),
]

LEFT_ALONE = [
    # not a walk: self-loop filter, cycle (the ROWS of a common-neighbour or same-source join are not walks either;
    # their count(*) alone is one equi-join's cardinality: GG_JOIN_COUNT, in TAKEN)
    "SELECT k1.k_person1id, k2.k_person1id FROM knows k1, knows k2 WHERE k1.k_person2id = k2.k_person2id",
    "SELECT count(*) FROM knows k1, knows k2 WHERE k1.k_person2id = k2.k_person1id AND k2.k_person2id = k1.k_person1id",
    # only part of the walk is validated against the vertex table
    "SELECT count(*) FROM knows k1, knows k2, person p WHERE k1.k_person2id = k2.k_person1id AND p.p_personid = k2.k_person2id",
    # vertex key without a uniqueness constraint: a duplicate id would multiply rows on the CPU side
    "SELECT count(*) FROM person_nokey p0, knows k1, person_nokey p1 "
    "WHERE p0.p_personid = k1.k_person1id AND k1.k_person2id = p1.p_personid",
    # nullable edge columns in an edge-only chain: the outer ends are not join keys (the count of the two-table form,
    # chain(2), is one equi-join's cardinality and NULL-safe: GG_JOIN_COUNT takes it)
    chain(3, table="knows_nullable", a="a", b="b"),
    chain(2, table="knows_nullable", a="a", b="b", select="k1.a, k2.b"),
    # non-equality predicates, outer joins, other filters
    "SELECT count(*) FROM knows k1, knows k2 WHERE k1.k_person2id < k2.k_person1id",
    "SELECT count(*) FROM knows k1 LEFT JOIN knows k2 ON k1.k_person2id = k2.k_person1id",
    # aggregates other than an ungrouped count(*) keep their aggregate; the join under them is still a walk
]


def test_rules_are_inert_until_enabled(db):
    db.execute("PRAGMA disable_gpu_graph")
    plan = db.explain(chain(2))
    assert "HASH_JOIN" in plan and "GG_" not in plan


@pytest.mark.parametrize("sql,operator,detail", TAKEN)
def test_walk_patterns_are_taken_over(db, sql, operator, detail):
    db.execute("PRAGMA enable_gpu_graph")
    plan = db.explain(sql)
    assert operator in plan and "HASH_JOIN" not in plan, plan
    assert detail in " ".join(plan.replace("│", " ").split()), plan


@pytest.mark.parametrize("sql", LEFT_ALONE)
def test_everything_else_is_left_to_the_reference(db, sql):
    db.execute("PRAGMA enable_gpu_graph")
    plan = db.explain(sql)
    assert "GG_" not in plan, plan


def test_sub_chain_of_a_larger_join_and_grouped_aggregate(db):
    db.execute("PRAGMA enable_gpu_graph")
    # grouped aggregate: the aggregate stays, the join below it is substituted
    plan = db.explain(chain(2, select="k1.k_person1id, count(*)") + " GROUP BY k1.k_person1id")
    assert "GG_PATH_EXPAND" in plan and "HASH_GROUP_BY" in plan and "HASH_JOIN" not in plan
    # a walk joined with something else: the walk part is substituted where the reference's join-order
    # optimiser keeps it together as a subtree (a derived table does)
    plan = db.explain("SELECT count(*) FROM (SELECT k2.k_person2id AS f FROM knows k1, knows k2 "
                      "WHERE k1.k_person2id = k2.k_person1id) w, knows_nullable x WHERE x.a = w.f")
    assert "GG_PATH_EXPAND" in plan and plan.count("HASH_JOIN") == 1


# ---- recursive CTE + min(hop)  ->  64-lane BFS --------------------------------------------------------
def friends(seed_where="WHERE p_personid = 2", union="UNION", step_from="friends f, knows k",
            step_where="f.friend = k.k_person1id AND f.hopCount < 5", nxt="k.k_person2id", inc="f.hopCount+1",
            agg="min(hopCount)", vertex="person"):
    return f"""WITH RECURSIVE friends(startPerson, hopCount, friend) AS (
        SELECT p_personid, 0, p_personid FROM {vertex} {seed_where}
      {union}
        SELECT f.startPerson, {inc}, {nxt} FROM {step_from} WHERE {step_where})
    SELECT startPerson, {agg} AS hopCount, friend FROM friends GROUP BY startPerson, friend"""


BI10_CASE = "CASE WHEN f.friend = k.k_person1id then k.k_person2id ELSE k.k_person1id END"

BFS_TAKEN = [
    (friends(), "from 1 id"),
    # the literal friends / friends_shortest text of benchmark/ldbc/queries/bi-10-shortestpath.sql:8-31
    (friends(seed_where="WHERE 1=1 AND p_personid = 2", nxt=BI10_CASE,
             step_where="1=1 AND f.friend = k.k_person1id AND f.hopCount < 5"), "vertices: endpoint ids"),
    (friends(seed_where="WHERE p_personid IN (1, 3)"), "from 2 ids"),
    (friends(seed_where="WHERE p_personid IN (" + ", ".join(str(i * 3 + 1) for i in range(40)) + ")"), "from 40 ids"),
    (friends(seed_where="WHERE p_personid IN (1, 2)"), "from person where"),   # consecutive values: becomes a pushed-down range
    (friends(seed_where=""), "from every person"),
    (friends(step_where="f.friend = k.k_person1id AND f.hopCount <= 2"), "min hops <= 3"),
    # the oracle's formulation: the new vertex validated against the vertex table
    (R.sql_shortest([1, 2], 4), "vertices: person.p_personid"),
]

BFS_LEFT_ALONE = [
    friends(union="UNION ALL"),                                   # bag semantics: not a fixpoint of sets
    friends(step_where="f.friend = k.k_person1id"),               # no hop bound
    friends(inc="f.hopCount+2"),
    friends(agg="max(hopCount)"),
    friends(nxt="k.k_person1id"),                                 # does not advance along the edge
    friends(step_where="f.friend = k.k_person1id AND f.hopCount < 5 AND k.k_weight > 1"),
    friends(step_from="friends f, knows_nullable k", step_where="f.friend = k.a AND f.hopCount < 5", nxt="k.b"),
    friends(step_from="friends f, knows k, person_nokey p",
            step_where="f.friend = k.k_person1id AND k.k_person2id = p.p_personid AND f.hopCount < 5"),
]


@pytest.mark.parametrize("sql,detail", BFS_TAKEN)
def test_friends_cte_with_min_hop_becomes_bfs(db, sql, detail):
    db.execute("PRAGMA enable_gpu_graph")
    plan = db.explain(sql)
    assert "GG_SHORTEST_PATH_BFS" in plan and "REC_CTE" not in plan and "HASH_GROUP_BY" not in plan, plan
    assert detail in " ".join(plan.replace("│", " ").split()), plan


@pytest.mark.parametrize("sql", BFS_LEFT_ALONE)
def test_other_recursive_ctes_are_left_alone(db, sql):
    db.execute("PRAGMA enable_gpu_graph")
    plan = db.explain(sql)
    assert "GG_" not in plan and "REC_CTE" in plan, plan


# ---- walks whose vertices share a neighbour in a second edge table (Train Benchmark ConnectedSegments) ----
from tests.trainbenchmark import connectedsegments_sql  # noqa: E402
from tests import ldbc_shapes  # noqa: E402


@pytest.fixture(scope="module")
def traindb():
    from tests import trainbenchmark as tb

    d = R.RefDuckDB(threads=2)
    # benchmark/trainbenchmark/schema.sql (load.sql:3,10-11): INT ids, primary keys
    d.execute("CREATE TABLE Segment (id int NOT NULL, length int NOT NULL DEFAULT 1, PRIMARY KEY (id))")
    d.execute("CREATE TABLE connectsTo (TrackElement1_id int NOT NULL, TrackElement2_id int NOT NULL, "
              "PRIMARY KEY (TrackElement1_id, TrackElement2_id))")
    d.execute("CREATE TABLE monitoredBy (TrackElement_id int NOT NULL, Sensor_id int NOT NULL, "
              "PRIMARY KEY (TrackElement_id, Sensor_id))")
    for name, rows in tb.tables().items():
        for i in range(0, rows.shape[0], 500):
            d.execute(f"INSERT INTO {name} VALUES " +
                      ", ".join("(" + ", ".join(str(int(x)) for x in r) + ")" for r in rows[i:i + 500]))
    d.execute(f"LOAD '{EXT}'")
    yield d
    d.execute("PRAGMA disable_gpu_graph")
    d.close()


def test_connectedsegments_query_text_becomes_one_operator(traindb):
    traindb.execute("PRAGMA enable_gpu_graph")
    plan = traindb.explain(connectedsegments_sql())
    assert "GG_SAME_NEIGHBOUR_WALKS" in plan and "HASH_JOIN" not in plan, plan
    flat = " ".join(plan.replace("│", " ").split())
    assert "5 hops" in flat and "from every segment" in flat
    for hops in (1, 2, 6):
        assert "GG_SAME_NEIGHBOUR_WALKS" in traindb.explain(connectedsegments_sql(hops))
    # without the Segment table: walks may start anywhere
    no_source = connectedsegments_sql(2).replace("FROM Segment\nINNER JOIN connectsTo as ct1 ON Segment.id = ct1.TrackElement1_id",
                                                  "FROM connectsTo as ct1")
    plan = traindb.explain(no_source)
    assert "GG_SAME_NEIGHBOUR_WALKS" in plan and "from every" not in " ".join(plan.replace("│", " ").split())


@pytest.mark.parametrize("sql", [
    connectedsegments_sql(2, extra=" AND ct1.TrackElement1_id > 5"),                    # another predicate
    connectedsegments_sql(2).replace("mb1.Sensor_id = mb3.Sensor_id", "mb1.Sensor_id = mb3.TrackElement_id"),
    connectedsegments_sql(2).replace("mb3.TrackElement_id = ct2.TrackElement2_id", "mb3.TrackElement_id = ct2.TrackElement1_id"),
    connectedsegments_sql(2, segment="LEFT JOIN"),
])
def test_near_misses_of_the_same_neighbour_pattern_are_left_alone(traindb, sql):
    traindb.execute("PRAGMA enable_gpu_graph")
    assert "GG_SAME_NEIGHBOUR_WALKS" not in traindb.explain(sql)


def test_payload_column_keeps_its_join_on_the_cpu(traindb):
    """Segment.length is not a key: the join with Segment stays a hash join, the walk part below it (which
    the reference's join order keeps together) is still substituted."""
    traindb.execute("PRAGMA enable_gpu_graph")
    plan = traindb.explain(connectedsegments_sql(2).replace("mb1.Sensor_id AS sensor", "Segment.length AS sensor"))
    assert "HASH_JOIN" in plan


# ---- the reference's own LDBC query texts (benchmark/ldbc/, stored as shipped: tests/golden/make_ldbc_queries.py) ----
LDBC_TEXTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ldbc_queries.json")


def _ldbc_texts():
    with open(LDBC_TEXTS) as f:
        return json.load(f)


def _ldbc_database(populated=False):
    """benchmark/ldbc/schema.sql as shipped, one plausible row per table (joins over empty tables are folded
    to EMPTY_RESULT before any planner rule sees them) and a few knows rows; `populated` adds the few thousand
    rows of tests/ldbc_shapes.py on top."""
    d = R.RefDuckDB(threads=2)
    ddl = _ldbc_texts()["schema.sql"]
    for stmt in ddl.split(";"):
        lines = [ln for ln in stmt.splitlines() if not ln.strip().startswith("--")]
        if "".join(lines).strip():
            d.execute("\n".join(lines))
    defaults = {"BIGINT": "1", "INTEGER": "1", "VARCHAR": "'x'", "TIMESTAMP": "'2012-01-01 00:00:00'", "DATE": "'2012-01-01'",
                "BOOLEAN": "true"}
    for name in [r.split()[2].strip("(") for r in ddl.lower().splitlines() if r.startswith("create table")]:
        res = R._Result()
        cols = []
        d.L.duckdb_value_varchar.restype = R.C.c_void_p
        assert d.L.duckdb_query(d.con, f"PRAGMA table_info('{name}')".encode(), R.C.byref(res)) == 0
        for i in range(res.row_count):
            p = d.L.duckdb_value_varchar(R.C.byref(res), 2, i)
            cols.append(R.C.string_at(p).decode().upper())
        d.L.duckdb_destroy_result(R.C.byref(res))
        d.execute(f"INSERT INTO {name} VALUES (" + ", ".join(defaults.get(c.split("(")[0], "NULL") for c in cols) + ")")
    d.execute("INSERT INTO knows VALUES ('2012-01-01 00:00:00', 21990232556256, 2), ('2012-01-01 00:00:00', 2, 3), "
              "('2012-01-01 00:00:00', 6597069767251, 2), ('2012-01-01 00:00:00', 19791209310731, 2)")
    if populated:
        ldbc_shapes.populate(d, create=False)
    d.execute(f"LOAD '{EXT}'")
    return d


def test_statements_shaped_like_the_ldbc_queries_get_gpu_operators():
    """tests/ldbc_shapes.py generates five statements with the shape of interactive-complex-3/5/6/9/11 over a
    populated database (the GPU suite compares their results under both plans): each gets its friends UNION
    friends-of-friends table planned as GG_WALK_ENDPOINTS (the dedupe included), and its result under the reference's
    own plan is not empty."""
    d = R.RefDuckDB(threads=2)
    ldbc_shapes.populate(d)
    d.execute(f"LOAD '{EXT}'")
    for name, sql in ldbc_shapes.statements().items():
        assert len(d.execute_text(sql)) > 0, name
        d.execute("PRAGMA enable_gpu_graph")
        plan = d.explain(sql)
        d.execute("PRAGMA disable_gpu_graph")
        assert "GG_WALK_ENDPOINTS" in plan and "GG_PATH_EXPAND" not in plan, (name, plan)
    d.close()


def test_the_build_side_is_planned_as_pipeline_sinks_over_the_references_table_scans(db, monkeypatch):
    """Join, count and distinct rules hang the tables under the GPU operator as GG_*_SINK operators over the
    reference's own SEQ_SCANs (scheduled by its executor through the BuildPipelines case, gg_pipeline.cpp).  A
    connection that uses pinned graphs, or GG_NO_PIPELINE_SINKS, gets the scan-function form (tables read from the
    scan's init)."""
    db.execute("PRAGMA enable_gpu_graph")
    count = "SELECT count(*) FROM knows k1, knows k2 WHERE k1.k_person2id = k2.k_person1id"
    keyed = ("SELECT p0.p_personid, p2.p_personid FROM person p0, knows k1, person p1, knows k2, person p2 "
             "WHERE p0.p_personid = k1.k_person1id AND k1.k_person2id = p1.p_personid "
             "AND p1.p_personid = k2.k_person1id AND k2.k_person2id = p2.p_personid")
    try:
        plan = db.explain(count)
        assert "GG_PATH_COUNT" in plan and "GG_EDGE_SINK" in plan and "SEQ_SCAN" in plan and "GG_VERTEX_SINK" not in plan
        plan = db.explain(keyed)
        if "GG_PATH_EXPAND" in plan:  # (the keyed form needs a declared-unique key: see the fixture)
            assert "GG_VERTEX_SINK" in plan and "GG_EDGE_SINK" in plan
        plan = db.explain(BFS_TAKEN[0][0])  # the shortest-path rule takes the same route (seeds read once the graph exists)
        assert "GG_SHORTEST_PATH_BFS" in plan and "GG_EDGE_SINK" in plan and "SEQ_SCAN" in plan and "REC_CTE" not in plan
        db.execute("PRAGMA gg_use_pinned_graphs")
        plan = db.explain(count)
        assert "GG_PATH_COUNT" in plan and "GG_EDGE_SINK" not in plan
        db.execute("PRAGMA gg_ignore_pinned_graphs")
        monkeypatch.setenv("GG_NO_PIPELINE_SINKS", "1")
        plan = db.explain(count)
        assert "GG_PATH_COUNT" in plan and "GG_EDGE_SINK" not in plan
        plan = db.explain(BFS_TAKEN[0][0])
        assert "GG_SHORTEST_PATH_BFS" in plan and "GG_EDGE_SINK" not in plan
    finally:
        db.execute("PRAGMA gg_ignore_pinned_graphs")
        db.execute("PRAGMA disable_gpu_graph")


def test_unions_that_are_not_friends_and_friends_of_friends_keep_their_dedupe():
    """The distinct rule takes a UNION only if it is exactly {1-hop endpoints of C} UNION {2-hop endpoints of C
    [with predicates on the endpoint]} over one edge table.  Anything else keeps the reference's UNION + hash
    aggregate (the 2-hop branch alone may still become GG_PATH_EXPAND)."""
    d = R.RefDuckDB(threads=2)
    ldbc_shapes.populate(d)
    d.execute("CREATE TABLE knows_nullable (a BIGINT, b BIGINT)")
    d.execute("INSERT INTO knows_nullable SELECT k_person1id, k_person2id FROM knows")
    d.execute(f"LOAD '{EXT}'")
    d.execute("PRAGMA enable_gpu_graph")
    a, b = ldbc_shapes.PERSON_A, ldbc_shapes.PERSON_B
    one = "select k_person2id from knows where k_person1id = {}"
    two = ("select k2.k_person2id from knows k1, knows k2 where k1.k_person1id = {} "
           "and k1.k_person2id = k2.k_person1id{}")
    taken = one.format(a) + " union " + two.format(a, "")
    assert "GG_WALK_ENDPOINTS" in d.explain(taken)
    assert "GG_WALK_ENDPOINTS" in d.explain(two.format(a, " and k2.k_person2id > 1000000") + " union " + one.format(a))
    near_misses = [
        one.format(a) + " union " + two.format(b, ""),                                   # two different people
        one.format(a) + " union all " + two.format(a, ""),                               # no dedupe asked for
        one.format(a) + " union " + two.format(a, " and k1.k_person2id <> 5"),           # predicate on the middle vertex
        one.format(a) + " and k_person2id <> 7 union " + two.format(a, ""),              # predicate on the 1-hop branch
        "select k_person1id from knows where k_person1id = {} union ".format(a) + two.format(a, ""),  # not the endpoint
        one.format(a) + " union " + two.format(a, "").replace("select k2.k_person2id", "select k2.k_person1id"),
        one.format(a) + " except " + two.format(a, ""),
        ("select b from knows_nullable where a = {0} union select k2.b from knows_nullable k1, knows_nullable k2 "
         "where k1.a = {0} and k1.b = k2.a").format(a),                                  # a NULL endpoint would be a row
    ]
    for sql in near_misses:
        assert "GG_WALK_ENDPOINTS" not in d.explain(sql), sql
    # distinct rule 2: SELECT DISTINCT <end vertex> of a pinned walk of h >= 2 edges is the set image of h hops
    three = ("select distinct k3.k_person2id from knows k1, knows k2, knows k3 where k1.k_person1id = {} "
             "and k1.k_person2id = k2.k_person1id and k2.k_person2id = k3.k_person1id{}")
    for sql in (two.format(a, "").replace("select ", "select distinct ", 1),
                two.format(a, " and k2.k_person2id <> {}".format(a)).replace("select ", "select distinct ", 1),
                three.format(a, ""), three.format(a, " and k3.k_person2id > 1000")):
        plan = d.explain(sql)
        assert "GG_WALK_ENDPOINTS" in plan and "HASH_GROUP_BY" not in plan, (sql, plan)
    for sql in (three.format(a, " and k2.k_person2id <> 5"),                                  # predicate on an inner vertex
                three.format(a, "").replace("distinct k3.k_person2id", "distinct k2.k_person2id"),  # not the end vertex
                three.format(a, "").replace("distinct k3.k_person2id", "distinct k1.k_person1id, k3.k_person2id"),
                "select distinct k2.k_person2id from knows k1, knows k2 where k1.k_person2id = k2.k_person1id",  # no source
                "select distinct k2.b from knows_nullable k1, knows_nullable k2 where k1.a = {} and k1.b = k2.a".format(a)):
        assert "GG_WALK_ENDPOINTS" not in d.explain(sql), sql
    d.close()


@pytest.mark.parametrize("populated", [False, True])
def test_the_references_ldbc_queries_get_gpu_operators(populated):
    """The LDBC interactive queries of the reference that walk KNOWS twice (friends of friends:
    interactive-complex-3/5/6/9/11) get their `knows k1, knows k2` join planned as GG_PATH_EXPAND — from the
    query files as shipped, inside plans that join the result with person, place, message, ..."""
    d = _ldbc_database(populated)
    d.execute("PRAGMA enable_gpu_graph")
    # (interactive-complex-10 and bi-10 hold the same shapes, but their other predicates — string
    # constants, dates — let statistics propagation fold the whole plan to EMPTY_RESULT on one-row tables;
    # bi-10's friends/friends_shortest text is covered by test_friends_cte_with_min_hop_becomes_bfs)
    # the friends UNION friends-of-friends table of these five is ONE device operator (distinct walk endpoints)
    expect = {"interactive-complex-3.sql": "GG_WALK_ENDPOINTS", "interactive-complex-5.sql": "GG_WALK_ENDPOINTS",
              "interactive-complex-6.sql": "GG_WALK_ENDPOINTS", "interactive-complex-9.sql": "GG_WALK_ENDPOINTS",
              "interactive-complex-11.sql": "GG_WALK_ENDPOINTS"}
    seen = {}
    for name, text in sorted(_ldbc_texts()["queries"].items()):
        sql = text.strip().rstrip(";")
        try:
            plan = d.explain(sql)
        except RuntimeError:
            continue  # a few of the shipped texts do not bind in this version of the reference either
        seen[name] = [op for op in ("GG_PATH_EXPAND", "GG_PATH_COUNT", "GG_SHORTEST_PATH_BFS", "GG_SAME_NEIGHBOUR_WALKS",
                                    "GG_WALK_ENDPOINTS")
                      if op in plan]
    d.close()
    for name, op in expect.items():
        assert op in seen.get(name, []), (name, seen.get(name))


def test_the_rule_switch_belongs_to_one_connection(db):
    """PRAGMA enable_gpu_graph acts on the connection that issues it (the reference's pragmas are ClientContext
    state, client_context.hpp:61-95): a second connection keeps the reference's plan until it says so itself."""
    sql = "SELECT count(*) FROM knows k1, knows k2 WHERE k1.k_person2id = k2.k_person1id"
    other = db.connect()
    try:
        db.execute("PRAGMA enable_gpu_graph")
        assert "GG_" in db.explain(sql) and "GG_" not in other.explain(sql)
        other.execute("PRAGMA enable_gpu_graph")
        db.execute("PRAGMA disable_gpu_graph")
        assert "GG_" not in db.explain(sql) and "GG_" in other.explain(sql)
    finally:
        other.execute("PRAGMA disable_gpu_graph")
        other.close()
        db.execute("PRAGMA disable_gpu_graph")
