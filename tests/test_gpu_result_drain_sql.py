"""The drain of device-resident results (GGResultDrain, host/gg_operators.hpp) where it is more than its degenerate form:
a batch, a part or a table of several slabs of 2^18 rows claimed by several pipeline threads, and a batch or part replaced
while claims on the previous one are still being fetched.  Every comparison is exact on sorted rows; each case asserts
from its yardstick that the result really spans the slabs it is meant to."""
import os

import numpy as np
import pytest

from duckdb_pgq_amd import datagen
from oracle import ref_duckdb as R
from tests import shortest_path_ref as S
from tests import triangles_ref as T
from tests.oracle_lib import sort_rows

EXT = R.EXTENSION

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not (R.available() and os.path.exists(EXT)), reason="reference build / extension not present"),
]

GRAPH = "'person', 'p_personid', 'knows', 'k_person1id', 'k_person2id'"
SLAB = 1 << 18  # GGResultSlab::SLAB_ROWS
NO_PERSON = "SELECT p_personid FROM person WHERE p_personid <> p_personid"


def open_db(vid, src, dst):
    d = R.RefDuckDB(threads=4)
    d.load_ldbc(vid, src, dst)
    d.execute(f"LOAD '{EXT}'")
    return d


# ---- hop counts: 130 sources = batches of 64, 64 and 2; any 64 of them reach more than one slab of rows ----------------
MAX_HOPS = 8


@pytest.fixture(scope="module")
def knows():
    vid, src, dst = datagen.ldbc_knows(6000, 150_000, 0xD4A1)
    d = open_db(vid, src, dst)
    yield d, vid, src, dst
    d.close()


def forward_csr(vid, src, dst):
    """(off, nbr, dense index of an id or -1) over the edge rows whose two ends are persons; dense order = table order"""
    order = np.argsort(vid, kind="stable")
    keys = vid[order]

    def dense(ids):
        at = np.minimum(np.searchsorted(keys, ids), keys.size - 1)
        return np.where(keys[at] == ids, order[at], -1)

    su, dv = dense(src), dense(dst)
    keep = (su >= 0) & (dv >= 0)
    su, dv = su[keep], dv[keep]
    off = np.zeros(vid.size + 1, np.int64)
    np.cumsum(np.bincount(su, minlength=vid.size), out=off[1:])
    return off, dv[np.argsort(su, kind="stable")], dense


def test_hop_counts_of_batches_of_several_slabs(knows):
    d, vid, src, dst = knows
    sources = datagen.pick_sources(vid, 130, 9)
    assert np.unique(sources).size == 130
    off, nbr, dense = forward_csr(vid, src, dst)
    want, per_source = [], []
    for s_id, s in zip(sources.tolist(), dense(sources).tolist()):
        dist = S.bfs_dist(off, nbr, s, MAX_HOPS)
        reached = np.flatnonzero(dist >= 0)
        per_source.append(reached.size)
        want.append(np.stack([np.full(reached.size, s_id, np.int64), vid[reached], dist[reached]], axis=1))
    # whatever order the sources arrive in, a batch of 64 has more rows than one slab
    assert int(np.sort(per_source)[:64].sum()) > SLAB
    src_sql = "SELECT p_personid FROM person WHERE p_personid IN (" + ", ".join(str(s) for s in sources.tolist()) + ")"
    got = d.execute(f"SELECT * FROM gg_shortest_path({GRAPH}, '{src_sql}', {MAX_HOPS})")
    assert np.array_equal(sort_rows(got), sort_rows(np.concatenate(want)))


# ---- path rows: a directed line, 65 sources (two batches) x the last three vertices ------------------------------------
LINE = 3000


def line_id(i):
    return 10 + 7 * np.asarray(i, np.int64)


@pytest.fixture(scope="module")
def line():
    at = np.arange(LINE, dtype=np.int64)
    d = open_db(line_id(at), line_id(at[:-1]), line_id(at[1:]))  # rowid i is the edge i -> i + 1
    pairs = [(i, t) for i in range(65) for t in (LINE - 3, LINE - 2, LINE - 1)]  # grouped by source, sources ascending
    d.load_table("pairs", {"a": line_id([p[0] for p in pairs]), "b": line_id([p[1] for p in pairs])})
    yield d, pairs
    d.close()


def line_rows(pairs):
    """(src, dst, step, vertex, edge rowid; 0 where it is NULL) of the one path of every pair (i, t): i, i + 1, ..., t"""
    out = []
    for i, t in pairs:
        step = np.arange(t - i + 1, dtype=np.int64)
        edge = np.maximum(i + step - 1, 0)
        edge[0] = 0  # (NULL: no edge leads into the first vertex)
        out.append(np.stack([np.full(step.size, line_id(i)), np.full(step.size, line_id(t)), step, line_id(i + step),
                             edge], axis=1))
    return np.concatenate(out)


def test_path_rows_of_batches_of_several_slabs(line):
    d, pairs = line
    first = [p for p in pairs if p[0] < 64]  # the first batch: the first 64 distinct sources of the pairs statement
    want_first = line_rows(first)
    assert want_first.shape[0] > 2 * SLAB
    sql = "SELECT src, dst, step, vertex, edge_rowid FROM gg_shortest_path_rows({}, '{}', -1)"
    got = d.execute(sql.format(GRAPH, "SELECT a, b FROM pairs"))
    assert np.array_equal(sort_rows(got), sort_rows(line_rows(pairs)))
    nulls = d.execute("SELECT step, count(*) FROM gg_shortest_path_rows({}, '{}', -1) WHERE edge_rowid IS NULL GROUP BY step"
                      .format(GRAPH, "SELECT a, b FROM pairs"))
    assert nulls.tolist() == [[0, len(pairs)]]
    # one batch only: the matching subset
    got = d.execute(sql.format(GRAPH, f"SELECT a, b FROM pairs WHERE a < {int(line_id(64))}"))
    assert np.array_equal(sort_rows(got), sort_rows(want_first))


# ---- triangle rows: one table of more than two slabs -------------------------------------------------------------------
def dense_mirrored_graph(n=400, degree=84, seed=0x7E1):
    """every unordered pair with probability degree / (n - 1), both directions as rows: about degree^3 triangle rows"""
    rng = np.random.RandomState(seed)
    a, b = np.triu_indices(n, 1)
    keep = rng.rand(a.size) < degree / (n - 1)
    a, b = a[keep].astype(np.int64), b[keep].astype(np.int64)
    vid = 1000 + 3 * rng.permutation(n).astype(np.int64)
    return vid, np.concatenate([vid[a], vid[b]]), np.concatenate([vid[b], vid[a]])


@pytest.fixture(scope="module")
def dense_graph():
    vid, src, dst = dense_mirrored_graph()
    d = open_db(vid, src, dst)
    yield d, T.TriangleGraph(vid, src, dst).trace_cube()
    d.close()


@pytest.mark.parametrize("ordered", [False, True])
def test_triangle_rows_of_several_slabs(dense_graph, ordered):
    d, trace = dense_graph
    n = int(d.execute(f"SELECT rows FROM gg_triangle_count({GRAPH}, false)")[0, 0])
    assert n == trace > 2 * SLAB
    want = sort_rows(d.execute(T.sql_triangles(T.SQL_ROWS, ordered)))
    assert want.shape[0] == (n // 6 if ordered else n)  # (no self-loops, no parallel rows: six rotations and reflections)
    flag = "true" if ordered else "false"
    got = d.execute(f"SELECT v0, v1, v2 FROM gg_triangles({GRAPH}, {flag})")
    assert np.array_equal(sort_rows(got), want)


# ---- walks: the 1- and 2-hop tables of every source (the product form, by middle vertex), whole and part by part ------
@pytest.fixture(scope="module")
def dense_walks(dense_graph):
    d, trace = dense_graph
    one, two = d.execute(R.sql_khop_rows(1)), d.execute(R.sql_khop_rows(2))
    assert two.shape[0] > 2 * SLAB  # about 400 * 84 * 84 rows: the 2-hop table alone is ten slabs
    want = np.concatenate([np.concatenate([np.full((one.shape[0], 1), 1), one, np.zeros((one.shape[0], 1), np.int64)], axis=1),
                           np.concatenate([np.full((two.shape[0], 1), 2), two], axis=1)])  # (a NULL reads as 0)
    return sort_rows(want)


@pytest.mark.parametrize("budget_mb", [None, 24], ids=["one_part", "parts_of_several_slabs"])
def test_walk_rows_of_several_slabs_and_parts(dense_graph, dense_walks, monkeypatch, budget_mb):
    d, trace = dense_graph
    if budget_mb:
        # 71 MB of ids (3 columns of 8 bytes) against 24 MB: three parts by bytes, four as the planner rounds up, of
        # about 0.7 M rows each — parts of more than one slab, replaced while claims on them are being fetched
        assert 3 * (budget_mb << 20) > dense_walks.shape[0] * 24 > 2 * (budget_mb << 20) > 4 * SLAB * 24
        monkeypatch.setenv("GG_RESULT_BUDGET_MB", str(budget_mb))
    got = d.execute(f"SELECT hops, v0, v1, v2 FROM gg_khop({GRAPH}, 1, 2)")
    assert np.array_equal(sort_rows(got), dense_walks)


# ---- nothing to drain --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("statement", [
    f"SELECT * FROM gg_shortest_path({GRAPH}, '{NO_PERSON}', 4)",
    f"SELECT * FROM gg_shortest_path_rows({GRAPH}, 'SELECT a, b FROM pairs WHERE a < 0', -1)",
    f"SELECT * FROM gg_triangles({GRAPH}, false)",  # (a directed line closes no walk)
], ids=["no_sources", "no_pairs", "no_triangles"])
def test_an_empty_drain(line, statement):
    d, pairs = line
    assert d.execute(statement).shape[0] == 0
    assert int(d.execute("SELECT count(*) FROM person")[0, 0]) == LINE  # the connection is usable afterwards
    assert d.execute(statement).shape[0] == 0
