"""gg_cheapest_path_rows inside the compiled reference, on tests/test_gpu_cheapest_sql.py's graph: its rows equal the
restatement in python integers (tests/cheapest_paths_ref.py) as sorted rows — the tables have fewer than 2^20 rows, so
they reach the device in rowid order and the pinned choice among equally cheap paths applies — and, joined back to the
edge table on rowid = edge_rowid inside the reference, every step's row connects the previous vertex to this one, the
weights of a pair's rows add up to the cost gg_cheapest_path reports for it, and its steps number that function's hops."""
import os

import numpy as np
import pytest

from oracle import ref_duckdb as R
from tests import cheapest_paths_ref as PR
from tests import cheapest_ref as CR
from tests import triangles_ref as T

EXT = R.EXTENSION

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not (R.available() and os.path.exists(EXT)), reason="reference build / extension not present"),
]

GRAPH = "'person', 'p_personid', 'knows', 'k_person1id', 'k_person2id', 'k_weight'"
COLUMNS = "src, dst, step, vertex, coalesce(edge_rowid, -1), cost"


@pytest.fixture(scope="module")
def db():
    vid, src, dst = T.hard_graph(V=300, rows=3000, seed=0x51, hub_fan=120)
    wt = CR.hashed_weights(src.size)
    g = CR.WeightedGraph(vid, src, dst, wt)
    d = R.RefDuckDB(threads=4)
    d.load_table("person", {"p_personid": vid})
    d.load_table("knows", {"k_person1id": src, "k_person2id": dst, "k_weight": wt})
    d.execute(f"LOAD '{EXT}'")
    tg = T.TriangleGraph(vid, src, dst)
    hub = int(np.bincount(tg.dv, minlength=tg.V).argmax())
    loop = int(np.nonzero(tg.A.diagonal())[0][0])
    six = [int(x) for x in g.vid[[hub, 3, loop, 17, 250]].tolist()] + [-123456789]  # the last one is no vertex
    five = [int(x) for x in g.vid[[3, 40, 7, 299, hub]].tolist()]
    seventy = [int(x) for x in g.vid[100:170].tolist()]  # two batches
    yield d, g, six, five, seventy
    d.close()


def pairs_sql(pairs):
    """a relation of the pairs as they stand, duplicates and NULLs included"""
    cell = lambda x: "NULL::BIGINT" if x is None else f"{int(x)}::BIGINT"
    return "'SELECT * FROM (VALUES " + ", ".join(f"({cell(a)}, {cell(b)})" for a, b in pairs) + ") t(a, b)'"


def function_rows(d, pairs, columns=COLUMNS):
    rows = d.query_text(f"SELECT {columns} FROM gg_cheapest_path_rows({GRAPH}, {pairs_sql(pairs)})")
    return sorted(tuple(int(x) for x in r) for r in rows)


def restated(g, pairs):
    s, t = [a for a, _ in pairs], [b for _, b in pairs]
    return PR.id_rows(PR.pair_paths(g, s, t)["rows"], s, t)


def test_six_sources_by_five_targets_equal_the_restatement(db):
    d, g, six, five, _ = db
    pairs = [(s, t) for s in six for t in five]
    want = restated(g, pairs)
    assert len(want) > 3 * 25 and not any(r[0] == six[-1] for r in want)
    assert function_rows(d, pairs) == want
    # the edge of step 0 is NULL, and only that one
    nulls = d.query_text(f"SELECT step, count(*) FROM gg_cheapest_path_rows({GRAPH}, {pairs_sql(pairs)}) "
                         "WHERE edge_rowid IS NULL GROUP BY step")
    assert [tuple(int(x) for x in r) for r in nulls] == [(0, 25)]


def test_seventy_sources_in_two_batches_equal_the_restatement(db):
    d, g, _, five, seventy = db
    pairs = [(s, t) for s in seventy for t in five[:3]]
    want = restated(g, pairs)
    assert len({r[0] for r in want}) > 64
    assert function_rows(d, pairs) == want


def test_a_null_in_a_pair_duplicates_and_pairs_without_a_path(db):
    d, g, six, five, _ = db
    s, t = six[1], five[1]
    pairs = [(s, t), (None, t), (s, None), (s, t), (s, s), (six[-1], t), (s, -999), (None, None)]
    real = [(a, b) for a, b in pairs if a is not None and b is not None]  # a pair with a NULL is skipped
    want = restated(g, real)
    path = [r for r in want if r[:2] == (s, t)]
    assert len(path) >= 4 and len(path) % 2 == 0 and path[0::2] == path[1::2]  # the duplicate pair has its rows twice
    assert want == sorted(path + [(s, s, 0, s, -1, 0)])
    assert function_rows(d, pairs) == want
    assert function_rows(d, [(six[-1], t), (None, t)]) == []


def test_join_back_to_the_edge_table_and_to_the_costs(db):
    d, g, six, five, _ = db
    pairs = [(s, t) for s in six for t in five]
    rows = f"gg_cheapest_path_rows({GRAPH}, {pairs_sql(pairs)})"
    # each step's row connects the previous vertex to this one
    joined = d.query_text(
        f"WITH r AS (SELECT * FROM {rows}) "
        "SELECT count(*), sum(CASE WHEN k.k_person1id = a.vertex AND k.k_person2id = b.vertex "
        "AND b.cost - a.cost = k.k_weight THEN 1 ELSE 0 END) "
        "FROM r a, r b, knows k WHERE a.src = b.src AND a.dst = b.dst AND a.step + 1 = b.step AND k.rowid = b.edge_rowid")
    steps, good = (int(x) for x in joined[0])
    want = restated(g, pairs)
    assert steps == good == sum(1 for r in want if r[2] >= 1) > 50
    # per pair: the weights add up to gg_cheapest_path's cost, the rows minus one are its hops
    sources = "'SELECT x FROM (VALUES " + ", ".join(f"({s})" for s in six) + ") t(x)'"
    summed = d.query_text(
        f"WITH r AS (SELECT * FROM {rows}) "
        "SELECT r.src, r.dst, coalesce(sum(k.k_weight), 0), count(*) - 1 FROM r LEFT JOIN knows k ON k.rowid = r.edge_rowid "
        "GROUP BY r.src, r.dst")
    costs = d.query_text(f"SELECT source, vertex, cost, hops FROM gg_cheapest_path({GRAPH}, {sources}, NULL, NULL)")
    asked = set(pairs)
    want_costs = sorted(t for t in (tuple(int(x) for x in r) for r in costs) if t[:2] in asked)
    assert sorted(tuple(int(x) for x in r) for r in summed) == want_costs and len(want_costs) == 25
