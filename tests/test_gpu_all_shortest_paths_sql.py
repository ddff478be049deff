"""gg_all_shortest_path_rows and gg_shortest_path_counts inside the compiled reference, with the reference itself as the
yardstick and no planner rule on: friends_shortest by the bi-10 recursive CTE, then a recursive UNION ALL CTE that walks
knows forward under fs.hopCount = h + 1 and carries the edge rowids as a comma-joined string — every row of it is one
shortest path, their set per pair is what ALL SHORTEST means, and count(*) GROUP BY over it is the count."""
import os
from collections import defaultdict

import numpy as np
import pytest

from duckdb_pgq_amd import datagen
from oracle import ref_duckdb as R

EXT = R.EXTENSION

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not (R.available() and os.path.exists(EXT)), reason="reference build / extension not present"),
]

GRAPH = "'person', 'p_personid', 'knows', 'k_person1id', 'k_person2id'"
MAX_HOPS = 3
PAIRS = "SELECT startPerson, friend FROM fs"


@pytest.fixture(scope="module")
def db():
    vid, src, dst = datagen.ldbc_knows(400, 4000, 0xBEEF)
    # parallel rows (several rowids for one edge), a self-loop, dangling rows
    src = np.concatenate([src, src[:100], np.array([vid[7], -5, vid[3]], np.int64)])
    dst = np.concatenate([dst, dst[:100], np.array([vid[7], vid[2], -6], np.int64)])
    d = R.RefDuckDB(threads=4)
    d.load_ldbc(vid, src, dst)
    d.execute(f"LOAD '{EXT}'")
    sources = datagen.pick_sources(vid, 70, 5)  # > 64: two bit-lane batches
    d.execute("CREATE TABLE fs AS " + R.sql_shortest(sources, MAX_HOPS))
    walks = d.query_text("""
        WITH RECURSIVE walk(s, x, h, edges) AS (
            SELECT startPerson, friend, 0, '' FROM fs WHERE hopCount = 0
          UNION ALL
            SELECT w.s, k.k_person2id, w.h + 1, w.edges || ',' || CAST(k.rowid AS VARCHAR)
              FROM walk w, knows k, fs f
             WHERE k.k_person1id = w.x AND f.startPerson = w.s AND f.friend = k.k_person2id AND f.hopCount = w.h + 1
        )
        SELECT s, x, h, edges FROM walk""")
    want = defaultdict(list)  # (s, t) -> the paths, each the tuple of its edge rowids
    for s, x, h, edges in walks:
        path = tuple(int(e) for e in edges.split(",")[1:])
        assert len(path) == int(h)
        want[(int(s), int(x))].append(path)
    for paths in want.values():
        assert len(set(paths)) == len(paths)  # a path is a sequence of edge rows: no two alike
    yield d, vid, sources, want
    d.close()


def rows_sql(pairs_sql=PAIRS, max_hops=MAX_HOPS, path_limit=0, select="src, dst, path, step, vertex, edge_rowid"):
    return f"SELECT {select} FROM gg_all_shortest_path_rows({GRAPH}, '{pairs_sql}', {max_hops}, {path_limit})"


def assemble(got):
    """(src, dst, path, step, vertex, edge_rowid) rows -> {(s, t): {path index: edge rowids}}, steps checked on the way"""
    got = got[np.lexsort((got[:, 3], got[:, 2], got[:, 1], got[:, 0]))]
    out = defaultdict(dict)
    for s, t, path, step, v, e in got.tolist():
        edges = out[(s, t)].setdefault(path, [])
        if step == 0:
            assert v == s and not edges
            edges.append(None)  # the marker of step 0 (its edge is NULL)
        else:
            assert len(edges) == step
            edges.append(e)
    return {k: {p: tuple(e[1:]) for p, e in v.items()} for k, v in out.items()}


def test_the_graph_is_the_size_the_issue_states(db):
    d, vid, sources, want = db
    assert len(want) == int(d.execute("SELECT count(*) FROM fs")[0, 0]) == 26_774
    assert sum(len(p) for p in want.values()) == 70_127
    assert sum(len(q) + 1 for p in want.values() for q in p) == 257_607


def test_counts_equal_the_reference(db):
    d, vid, sources, want = db
    got = d.execute(f"SELECT src, dst, hops, CAST(paths AS BIGINT) FROM gg_shortest_path_counts({GRAPH}, '{PAIRS}', {MAX_HOPS})")
    assert got.shape[0] == len(want)
    hops = {(s, t): h for s, t, h in d.execute("SELECT startPerson, friend, hopCount FROM fs").tolist()}
    for s, t, h, n in got.tolist():
        assert n == len(want[(s, t)]) and h == hops[(s, t)], (s, t)
    assert len({(s, t) for s, t, _, _ in got.tolist()}) == len(want)
    # the column is a HUGEINT, so that 2^64 - 1 is exact
    text = d.query_text(f"SELECT typeof(paths), sum(paths) FROM gg_shortest_path_counts({GRAPH}, '{PAIRS}', {MAX_HOPS}) GROUP BY 1")
    assert text == [("HUGEINT", "70127")]


def test_paths_equal_the_reference_set_pair_by_pair(db):
    d, vid, sources, want = db
    got = assemble(d.execute(rows_sql()))
    assert got.keys() == want.keys()
    for pair, paths in got.items():
        assert sorted(paths) == list(range(len(paths))), pair  # path indices 0..n-1 without gaps
        assert len(set(paths.values())) == len(paths) and set(paths.values()) == set(want[pair]), pair
    # the edge of step 0 is NULL, and only that one
    nulls = d.execute(rows_sql(select="step, count(*)") + " WHERE edge_rowid IS NULL GROUP BY step")
    assert nulls.tolist() == [[0, 70_127]]


def test_path_limit_returns_the_first_few_of_every_pair(db):
    d, vid, sources, want = db
    got = assemble(d.execute(rows_sql(path_limit=3)))
    assert got.keys() == want.keys()
    for pair, paths in got.items():
        assert sorted(paths) == list(range(min(3, len(want[pair])))), pair
        assert len(set(paths.values())) == len(paths) and set(paths.values()) <= set(want[pair]), pair
    # they are the first three by rank: the rows of the unlimited statement with path < 3
    full = d.execute(rows_sql())
    lim = d.execute(rows_sql(path_limit=3))
    key = lambda a: a[np.lexsort((a[:, 3], a[:, 2], a[:, 1], a[:, 0]))]  # noqa: E731
    assert np.array_equal(key(full[full[:, 2] < 3]), key(lim))


def test_path_zero_is_the_row_set_of_gg_shortest_path_rows(db):
    d, vid, sources, want = db
    one = d.execute(f"SELECT src, dst, step, vertex, edge_rowid FROM gg_shortest_path_rows({GRAPH}, '{PAIRS}', {MAX_HOPS})")
    first = d.execute(rows_sql(path_limit=1, select="src, dst, step, vertex, edge_rowid"))
    key = lambda a: a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]  # noqa: E731
    assert np.array_equal(key(one), key(first))


def test_pairs_without_a_path_duplicates_and_a_failing_pairs_statement(db):
    d, vid, sources, want = db
    s = int(sources[0])
    pairs = [(s, s), (s, -6), (-5, int(vid[2])), (s, s)]
    values = ", ".join(f"({a}::BIGINT, {b}::BIGINT)" for a, b in pairs)
    got = d.execute(rows_sql(f"SELECT * FROM (VALUES {values}) v(a, b)"))
    assert got.tolist() == [[s, s, 0, 0, s, 0], [s, s, 0, 0, s, 0]]  # (a NULL reads as 0 through the C API)
    got = d.execute(f"SELECT src, dst, hops, CAST(paths AS BIGINT) FROM gg_shortest_path_counts({GRAPH}, "
                    f"'SELECT * FROM (VALUES {values}) v(a, b)', -1)")
    assert got.tolist() == [[s, s, 0, 1], [s, s, 0, 1]]
    assert d.execute(rows_sql(PAIRS + " WHERE hopCount < 0")).shape[0] == 0
    with pytest.raises(RuntimeError, match="pairs"):
        d.execute(rows_sql("SELECT no_such_column, friend FROM fs"))
    with pytest.raises(RuntimeError, match="path_limit"):
        d.execute(rows_sql(path_limit=-1))
    assert d.execute(rows_sql(f"SELECT {s}::BIGINT, {s}::BIGINT")).shape[0] == 1  # the connection is usable afterwards
