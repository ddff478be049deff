"""Every statement the plan-rule tests hold, planned under each PRAGMA combination they use: per statement the EXPLAIN
text, what GG_RULE_TRACE wrote to stderr while it was planned, and by how much gg_plan_rules_fired() advanced.

A refactor of duckdb_pgq_amd/host/gg_plan_rule.cpp must leave this output byte-identical on both routes:

    python scripts/plan_trace.py > sinks.txt
    GG_NO_PIPELINE_SINKS=1 python scripts/plan_trace.py > scan_function.txt

once with the extension built before the change and once after, then diff.  Planning touches no device, so this runs on
a CPU; it needs the compiled reference and the extension under oracle/_ref/ (__graft_entry__.build()).
"""
import ctypes
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["GG_RULE_TRACE"] = "1"

from oracle import ref_duckdb as R  # noqa: E402
from tests import ldbc_shapes, test_plan_rule as walks, trainbenchmark  # noqa: E402
from tests import test_plan_rule_recursive_levels as levels  # noqa: E402
from tests import test_plan_rule_recursive_union as union  # noqa: E402
from tests import test_plan_rule_union_all as union_all  # noqa: E402

GRAPH = ["enable_gpu_graph"]
EVERY_SWITCH = [GRAPH, GRAPH + ["gg_use_pinned_graphs"], GRAPH + ["enable_gpu_joins"]]
RECURSIVE_SWITCHES = [GRAPH, GRAPH + ["enable_gpu_recursive_union"], GRAPH + ["enable_gpu_recursive_levels"],
                      GRAPH + ["enable_gpu_recursive_union", "enable_gpu_recursive_levels"]]
ALL_PRAGMAS = ["gpu_graph", "gpu_joins", "gpu_recursive_union", "gpu_recursive_levels"]


def first(entries):
    return [e if isinstance(e, str) else e[0] for e in entries]


def walks_db():
    d = R.RefDuckDB(threads=2)
    for sql in ("CREATE TABLE person (p_personid BIGINT PRIMARY KEY)",
                "CREATE TABLE person_nokey (p_personid BIGINT NOT NULL)",
                "CREATE TABLE knows (k_person1id BIGINT NOT NULL, k_person2id BIGINT NOT NULL, k_weight INTEGER)",
                "CREATE TABLE knows_nullable (a BIGINT, b BIGINT)",
                "CREATE TABLE e32 (a INTEGER NOT NULL, b INTEGER NOT NULL)",
                "INSERT INTO person VALUES (1), (2), (3)",
                "INSERT INTO knows VALUES (1, 2, 1), (2, 3, 2), (3, 1, 3)",
                "INSERT INTO person_nokey VALUES (1), (2), (3)",
                "INSERT INTO knows_nullable VALUES (1, 2), (2, 3), (3, NULL)",
                "INSERT INTO e32 VALUES (1, 2), (2, 3), (3, 1)"):
        d.execute(sql)
    return d


def train_db():
    d = R.RefDuckDB(threads=2)
    d.execute("CREATE TABLE Segment (id int NOT NULL, length int NOT NULL DEFAULT 1, PRIMARY KEY (id))")
    d.execute("CREATE TABLE connectsTo (TrackElement1_id int NOT NULL, TrackElement2_id int NOT NULL, "
              "PRIMARY KEY (TrackElement1_id, TrackElement2_id))")
    d.execute("CREATE TABLE monitoredBy (TrackElement_id int NOT NULL, Sensor_id int NOT NULL, "
              "PRIMARY KEY (TrackElement_id, Sensor_id))")
    for name, rows in trainbenchmark.tables().items():
        for i in range(0, rows.shape[0], 500):
            d.execute(f"INSERT INTO {name} VALUES " +
                      ", ".join("(" + ", ".join(str(int(x)) for x in r) + ")" for r in rows[i:i + 500]))
    return d


def recursive_db():
    d = R.RefDuckDB(threads=2)
    for ddl in levels.SCHEMA:
        d.execute(ddl)
    d.execute("INSERT INTO t VALUES (1, 2, 'a', 0.5), (2, 3, 'b', 1.5), (3, 1, 'c', 2.5), (NULL, 1, 'd', 3.5)")
    d.execute("INSERT INTO u VALUES (2, 2), (3, 3)")
    d.execute("CREATE TABLE e (a BIGINT NOT NULL, b BIGINT NOT NULL)")
    d.execute("INSERT INTO e VALUES (1, 2), (2, 3), (3, 4), (2, 5)")
    return d


def shapes_db():
    d = R.RefDuckDB(threads=2)
    ldbc_shapes.populate(d)
    d.execute("CREATE TABLE knows_nullable (a BIGINT, b BIGINT)")
    d.execute("INSERT INTO knows_nullable SELECT k_person1id, k_person2id FROM knows")
    return d


def distinct_statements():
    a, b = ldbc_shapes.PERSON_A, ldbc_shapes.PERSON_B
    one = "select k_person2id from knows where k_person1id = {}"
    two = "select k2.k_person2id from knows k1, knows k2 where k1.k_person1id = {} and k1.k_person2id = k2.k_person1id{}"
    three = ("select distinct k3.k_person2id from knows k1, knows k2, knows k3 where k1.k_person1id = {} "
             "and k1.k_person2id = k2.k_person1id and k2.k_person2id = k3.k_person1id{}")
    nullable = "from knows_nullable k1, knows_nullable k2 where k1.a = {} and k1.b = k2.a".format(a)
    return [
        one.format(a) + " union " + two.format(a, ""),
        two.format(a, " and k2.k_person2id > 1000000") + " union " + one.format(a),
        one.format(a) + " union " + two.format(b, ""),
        one.format(a) + " union all " + two.format(a, ""),
        one.format(a) + " union " + two.format(a, " and k1.k_person2id <> 5"),
        one.format(a) + " and k_person2id <> 7 union " + two.format(a, ""),
        "select k_person1id from knows where k_person1id = {} union ".format(a) + two.format(a, ""),
        one.format(a) + " union " + two.format(a, "").replace("select k2.k_person2id", "select k2.k_person1id"),
        one.format(a) + " except " + two.format(a, ""),
        "select b from knows_nullable where a = {} union select k2.b ".format(a) + nullable,
        two.format(a, "").replace("select ", "select distinct ", 1),
        two.format(a, " and k2.k_person2id <> {}".format(a)).replace("select ", "select distinct ", 1),
        three.format(a, ""),
        three.format(a, " and k3.k_person2id > 1000"),
        three.format(a, " and k2.k_person2id <> 5"),
        three.format(a, "").replace("distinct k3.k_person2id", "distinct k2.k_person2id"),
        three.format(a, "").replace("distinct k3.k_person2id", "distinct k1.k_person1id, k3.k_person2id"),
        "select distinct k2.k_person2id from knows k1, knows k2 where k1.k_person2id = k2.k_person1id",
        "select distinct k2.b " + nullable,
    ]


def connected_segments():
    cs = trainbenchmark.connectedsegments_sql
    return [cs(), cs(1), cs(2), cs(6),
            cs(2).replace("FROM Segment\nINNER JOIN connectsTo as ct1 ON Segment.id = ct1.TrackElement1_id",
                          "FROM connectsTo as ct1"),
            cs(2, extra=" AND ct1.TrackElement1_id > 5"),
            cs(2).replace("mb1.Sensor_id = mb3.Sensor_id", "mb1.Sensor_id = mb3.TrackElement_id"),
            cs(2).replace("mb3.TrackElement_id = ct2.TrackElement2_id", "mb3.TrackElement_id = ct2.TrackElement1_id"),
            cs(2, segment="LEFT JOIN"),
            cs(2).replace("mb1.Sensor_id AS sensor", "Segment.length AS sensor")]


def recursive_statements():
    sqls = []
    for module in (union_all, union, levels):
        for table in (module.ACCEPTED, module.DECLINED):
            sqls += first(table[name] for name in sorted(table))
    sqls += [union_all.NESTED[name] for name in sorted(union_all.NESTED)]
    return sqls


def ldbc_statements():
    texts = walks._ldbc_texts()["queries"]
    return [texts[name].strip().rstrip(";") for name in sorted(texts)] + \
           [levels.BI10_FRIENDS + consumer for consumer in levels.BI10_CONSUMERS]


def stderr_of(call):
    """(call's result, what the process wrote to file descriptor 2 meanwhile)"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as capture:
        os.dup2(capture.fileno(), 2)
        try:
            result = call()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        capture.seek(0)
        return result, capture.read().decode()


def run(title, make_db, switches, statements, load=True):
    d = make_db()
    if load:
        d.execute(f"LOAD '{R.EXTENSION}'")
    fired = ctypes.CDLL(R.EXTENSION).gg_plan_rules_fired
    fired.restype = ctypes.c_uint64
    for pragmas in switches:
        for pragma in pragmas:
            d.execute("PRAGMA " + pragma)
        for i, sql in enumerate(statements):
            print(f"==== {title} [{' '.join(pragmas)}] #{i}\n{sql}")
            before = fired()

            def explain():
                try:
                    return d.explain(sql)
                except RuntimeError as e:  # (a few of the shipped LDBC texts do not bind in this reference)
                    return f"error: {e}"
            plan, trace = stderr_of(explain)
            print(f"---- plan (rules fired: +{fired() - before})\n{plan}\n---- trace\n{trace}", end="")
        for pragma in ALL_PRAGMAS:
            d.execute("PRAGMA disable_" + pragma)
        d.execute("PRAGMA gg_ignore_pinned_graphs")
    d.close()


def main():
    if not (R.available() and os.path.exists(R.EXTENSION) and R.rules_route()):
        sys.exit("the compiled reference, the extension or the plan hook is missing under oracle/_ref/")
    print("route:", "scan function" if os.environ.get("GG_NO_PIPELINE_SINKS") else "pipeline sinks")
    run("walks", walks_db, EVERY_SWITCH,
        first(walks.TAKEN) + walks.LEFT_ALONE + first(walks.BFS_TAKEN) + walks.BFS_LEFT_ALONE)
    run("connected segments", train_db, EVERY_SWITCH[:2], connected_segments())
    run("distinct", shapes_db, EVERY_SWITCH[:2], distinct_statements() + list(ldbc_shapes.statements().values()))
    run("recursive", recursive_db, RECURSIVE_SWITCHES, recursive_statements())
    for populated in (False, True):
        run(f"ldbc populated={populated}", lambda: walks._ldbc_database(populated), [RECURSIVE_SWITCHES[0],
                                                                                      RECURSIVE_SWITCHES[3]],
            ldbc_statements(), load=False)  # (_ldbc_database loads the extension itself)


if __name__ == "__main__":
    main()
