"""gg_shortest_path_rows inside the compiled reference, with the reference itself as the yardstick: friends_shortest by
the bi-10 recursive CTE (no planner rule is on), from it the predecessor relation in plain SQL — pred(s, x) the person
with the smallest rowid among the knows sources one hop closer, the edge min(k.rowid) — and every row the function
returns is looked up in it.  Every pair of friends_shortest is asked for, none is left out.

The min(rowid) yardstick is the pinned relation only where the base tables reach the device in rowid order: tables of up
to 2^20 rows, which one thread reads (host/gg_ingest.cpp), as here.  Larger tables are read by several tasks whose chunks
interleave; the function then still returns one valid shortest path per pair with true edge rowids, but its choice among
equally short paths follows the order of arrival and this yardstick does not apply."""
import os

import numpy as np
import pytest

from duckdb_pgq_amd import datagen
from oracle import ref_duckdb as R
from tests.oracle_lib import sort_rows

EXT = R.EXTENSION

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not (R.available() and os.path.exists(EXT)), reason="reference build / extension not present"),
]

GRAPH = "'person', 'p_personid', 'knows', 'k_person1id', 'k_person2id'"
MAX_HOPS = 3


@pytest.fixture(scope="module")
def db():
    vid, src, dst = datagen.ldbc_knows(1500, 24_000, 0xBEEF)
    # parallel rows (several rowids for one edge), a self-loop, dangling rows
    src = np.concatenate([src, src[:300], np.array([vid[7], -5, vid[3]], np.int64)])
    dst = np.concatenate([dst, dst[:300], np.array([vid[7], vid[2], -6], np.int64)])
    d = R.RefDuckDB(threads=4)
    d.load_ldbc(vid, src, dst)
    d.execute(f"LOAD '{EXT}'")
    sources = datagen.pick_sources(vid, 70, 5)  # > 64: two bit-lane batches
    d.execute("CREATE TABLE fs AS " + R.sql_shortest(sources, MAX_HOPS))
    # pred(s, x): the person with minimal rowid among the knows sources one hop closer; then the edge with minimal rowid
    d.execute("""CREATE TABLE pred_row AS
        SELECT f.startPerson AS s, f.friend AS x, f.hopCount AS h, min(p.rowid) AS prow
          FROM fs f, knows k, fs g, person p
         WHERE f.hopCount >= 1 AND k.k_person2id = f.friend AND g.startPerson = f.startPerson
           AND g.friend = k.k_person1id AND g.hopCount = f.hopCount - 1 AND p.p_personid = k.k_person1id
         GROUP BY f.startPerson, f.friend, f.hopCount""")
    d.execute("""CREATE TABLE pred AS
        SELECT r.s AS s, r.x AS x, r.h AS h, p.p_personid AS u, min(k.rowid) AS erow
          FROM pred_row r, person p, knows k
         WHERE p.rowid = r.prow AND k.k_person1id = p.p_personid AND k.k_person2id = r.x
         GROUP BY r.s, r.x, r.h, p.p_personid""")
    yield d, vid, sources
    d.close()


def rows_sql(pairs_sql, max_hops=MAX_HOPS, select="src, dst, step, vertex, edge_rowid"):
    return f"SELECT {select} FROM gg_shortest_path_rows({GRAPH}, '{pairs_sql}', {max_hops})"


def check_rows(d, got):
    """got: (src, dst, step, vertex, edge_rowid) rows for the pairs of fs — against fs and pred"""
    fs = d.execute("SELECT startPerson, friend, hopCount FROM fs")
    pred = {(s, x): (h, u, e) for s, x, h, u, e in d.execute("SELECT s, x, h, u, erow FROM pred").tolist()}
    assert len(pred) == int((fs[:, 2] >= 1).sum())  # the relation covers every pair with a hop
    got = sort_rows(got)  # by (src, dst, step)
    hops = {(s, t): h for s, t, h in fs.tolist()}
    seen = {}
    prev = None
    for s, t, step, v, e in got.tolist():
        assert (s, t) in hops
        assert step == seen.get((s, t), -1) + 1  # 0, 1, 2, ... without gaps
        seen[(s, t)] = step
        if step == 0:
            assert v == s
        else:
            h, u, erow = pred[(s, v)]
            assert h == step and prev == u and e == erow, (s, t, step, v, e, pred[(s, v)])
        if step == hops[(s, t)]:
            assert v == t
        prev = v
    assert {k: v for k, v in seen.items()} == hops  # every pair, each up to its hop count
    return got


def test_every_friends_shortest_pair(db):
    d, vid, sources = db
    got = d.execute(rows_sql("SELECT startPerson, friend FROM fs"))
    got = check_rows(d, got)
    assert got.shape[0] > 5 * len(sources)
    # the edge of step 0 is NULL, and only that one
    nulls = d.execute(rows_sql("SELECT startPerson, friend FROM fs", select="step, count(*)") +
                      " WHERE edge_rowid IS NULL GROUP BY step")
    assert nulls.tolist() == [[0, int(d.execute("SELECT count(*) FROM fs")[0, 0])]]


def test_pairs_without_a_path_ids_that_are_no_person_and_duplicates(db):
    d, vid, sources = db
    s = int(sources[0])
    far = d.execute(f"SELECT p_personid FROM person WHERE p_personid NOT IN (SELECT friend FROM fs WHERE startPerson = {s}) "
                    "ORDER BY p_personid LIMIT 1")
    pairs = [(s, s), (s, -6), (-5, int(vid[2])), (s, s)]
    if far.shape[0]:
        pairs.append((s, int(far[0, 0])))
    values = ", ".join(f"({a}::BIGINT, {b}::BIGINT)" for a, b in pairs)
    got = d.execute(rows_sql(f"SELECT * FROM (VALUES {values}) v(a, b)"))
    assert got.tolist() == [[s, s, 0, s, 0], [s, s, 0, s, 0]]  # (a NULL reads as 0 through the C API)
    # cut by max_hops: the pairs three hops apart have no rows at two
    got = d.execute(rows_sql("SELECT startPerson, friend FROM fs", max_hops=2, select="src, dst, max(step)") +
                    " GROUP BY src, dst")
    want = d.execute("SELECT startPerson, friend, hopCount FROM fs WHERE hopCount <= 2")
    assert np.array_equal(sort_rows(got), sort_rows(want))


def test_join_back_to_the_edge_table_on_edge_rowid(db):
    d, vid, sources = db
    sql = ("WITH r AS (" + rows_sql("SELECT startPerson, friend FROM fs") + ") "
           "SELECT b.src, b.dst, b.step, a.vertex, b.vertex, k.k_person1id, k.k_person2id "
           "FROM r a, r b, knows k WHERE a.src = b.src AND a.dst = b.dst AND a.step + 1 = b.step AND k.rowid = b.edge_rowid")
    got = d.execute(sql)
    assert got.shape[0] == int(d.execute("SELECT sum(hopCount) FROM fs")[0, 0])
    assert np.array_equal(got[:, 3], got[:, 5]) and np.array_equal(got[:, 4], got[:, 6])  # the edge of a step is its row


def test_over_a_pinned_graph(db):
    d, vid, sources = db
    plain = sort_rows(d.execute(rows_sql("SELECT startPerson, friend FROM fs")))
    d.execute("PRAGMA gg_use_pinned_graphs")
    try:
        d.execute(f"SELECT * FROM gg_graph_pin({GRAPH})")
        for _ in range(2):  # the second statement finds the pin's rowid-carrying companion already built
            assert np.array_equal(sort_rows(d.execute(rows_sql("SELECT startPerson, friend FROM fs"))), plain)
        assert int(d.execute("SELECT * FROM gg_graph_pins()")[0, 0]) == 1
    finally:
        d.execute("SELECT * FROM gg_graph_unpin()")
        d.execute("PRAGMA gg_ignore_pinned_graphs")


def test_an_empty_and_a_failing_pairs_statement(db):
    d, vid, sources = db
    assert d.execute(rows_sql("SELECT startPerson, friend FROM fs WHERE hopCount < 0")).shape[0] == 0
    with pytest.raises(RuntimeError, match="pairs"):
        d.execute(rows_sql("SELECT no_such_column, friend FROM fs"))
    with pytest.raises(RuntimeError, match="two integer columns"):
        d.execute(rows_sql("SELECT friend FROM fs"))
    # the connection is usable afterwards
    assert d.execute(rows_sql(f"SELECT {int(sources[0])}::BIGINT, {int(sources[0])}::BIGINT")).shape[0] == 1
