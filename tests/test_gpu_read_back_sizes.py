"""Every entry point whose host read-backs go through gg::read_back / scan_total_* (csrc/gg_runtime.hip), at the sizes
where the chained scan behind the read-back changes shape: 1 element, one element short of a scan tile, exactly one tile
(SCAN_TILE = 4096) and one element past it.  N is the length of the array that is scanned -- the source, key, seed or
pair list, or the vertex table for the calls that count per vertex -- and every result is compared, exactly, with the
reference the entry point's own test file uses.  No fault injection here."""
import numpy as np
import pytest

from duckdb_pgq_amd import datagen
from tests import shortest_path_ref as ref
from tests import triangles_ref as T
from tests.oracle_lib import endpoint_sets, sort_rows
from tests.test_gpu_level_sets import exact_levels
from tests.test_gpu_parity import build_both
from tests.test_gpu_reach_closure import exact_reach
from tests.test_gpu_walk_closure import exact_closure

pytestmark = pytest.mark.gpu

SCAN_TILE = 4096
SIZES = [1, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1]


@pytest.fixture(scope="module")
def knows(orc):
    """one mirrored graph with more vertices than the longest list, and the oracle's CSR of it"""
    vid, src, dst = datagen.ldbc_knows(4300, 17_000, 23)
    rc, g = orc.csr_build(vid, src, dst)
    assert rc == 0 and vid.size > SIZES[-1]
    yield vid, src, dst, g
    g.close()


@pytest.fixture
def csr(gg, knows):
    vid, src, dst, g = knows
    gg.staging_clear()
    gg.append_vertices(vid)
    gg.append_edges(src, dst)
    c = gg.build_csr()
    yield c
    c.close()


def _fetch(res):
    try:
        got = res.fetch()
        assert sum(res.rows()) == got[0].size
        return got
    finally:
        res.close()


def _same(got, want, dtypes=False):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert np.array_equal(g, w) and (not dtypes or g.dtype == w.dtype)


@pytest.mark.parametrize("n", SIZES)
def test_expand_khop_from_a_source_list(gg, knows, csr, n):
    vid, src, dst, g = knows
    assert gg.expand_khop(csr, 1, 3, sources=vid[:n]) == g.khop(1, 3, sources_dense=g.lookup(vid[:n]).astype(np.uint32))


@pytest.mark.parametrize("n", SIZES)
def test_join_probe(gg, knows, csr, n):
    vid, src, dst, g = knows
    keys = vid[:n]
    order = np.argsort(src, kind="stable")  # rowid = append position; a key's rows in rowid order
    lo, hi = np.searchsorted(src[order], keys, "left"), np.searchsorted(src[order], keys, "right")
    want = np.concatenate([np.stack([np.full(h - l, i, np.int64), order[l:h].astype(np.int64)], axis=1)
                           for i, (l, h) in enumerate(zip(lo, hi))])
    got = gg.join_probe(csr, keys)
    assert got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("n", SIZES)
def test_walk_closure(gg, knows, csr, n):
    vid, src, dst, g = knows
    _same(_fetch(gg.walk_closure(csr, vid[:n], 2)), exact_closure(src, dst, np.arange(src.size, dtype=np.int64), vid[:n], 2),
          dtypes=True)


@pytest.mark.parametrize("n", SIZES)
def test_reach_closure(gg, knows, csr, n):
    vid, src, dst, g = knows
    seeds, classes, seen = vid[:n], (np.arange(n) % 3).astype(np.uint32), (np.arange(n) % 2).astype(bool)
    want = exact_reach(src, dst, g.arrays()[3], seeds, classes, seen)
    for mode in (1, 2):  # bitmap, hash set
        gg.debug_reach_visited(mode, 0)
        _same(_fetch(gg.reach_closure(csr, seeds, classes, seen)), want)


@pytest.mark.parametrize("order_mode", [1, 2])  # claim and sort, read the rows off the bitmap
@pytest.mark.parametrize("n", SIZES)
def test_level_sets(gg, knows, csr, n, order_mode):
    vid, src, dst, g = knows
    seeds, classes = vid[:n], (np.arange(n) % 3).astype(np.uint32)
    gg.debug_level_sets(1, order_mode)
    _same(_fetch(gg.level_sets(csr, seeds, classes, max_levels=2)),
          exact_levels(src, dst, g.arrays()[3], seeds, classes, 2))


@pytest.mark.parametrize("n", SIZES)
def test_shortest_path_rows(gg, knows, csr, n):
    vid, src, dst, g = knows
    s, t = vid[np.arange(n) % 8], vid[(np.arange(n) * 7 + 3) % vid.size]  # one batch of 8 sources, n pairs
    off, nbr, eid, v = g.arrays()
    _same(gg.shortest_paths(csr, s, t, -1, edges=True), ref.shortest_paths(off, nbr, eid, v, s, t, -1, True), dtypes=True)


@pytest.mark.parametrize("n", SIZES)
def test_triangles_from_a_source_list(gg, orc, knows, csr, n):
    vid, src, dst, g = knows
    tg = T.TriangleGraph(vid, src, dst)
    rows, wedges = tg.rows(0, vid[:n].tolist())
    want = {"rows": rows.shape[0], "digest": orc.digest_rows(rows.astype(np.uint32)), "wedges": wedges}
    st, res = gg.triangles(csr, vid[:n], materialise=True)
    try:
        assert st == want and res.rows(2) == want["rows"]
        got = [res.fetch(2, o) for o in range(0, res.rows(2), 1024)]
        got = np.concatenate(got, axis=0) if got else np.empty((0, 3), np.int64)
        assert np.array_equal(sort_rows(got), sort_rows(tg.id_rows(rows)))
    finally:
        res.close()


@pytest.mark.parametrize("n_vertices", SIZES)
def test_walk_endpoints_and_bfs_pairs_count_per_vertex(gg, orc, n_vertices):
    """these two scan one count per VERTEX: the graph itself has 1, 4095, 4096 and 4097 vertices"""
    vid, src, dst = datagen.small_graph(n_vertices, 3 * n_vertices, 31)
    csr, g = build_both(gg, orc, vid, src, dst)
    try:
        off, nbr, _, o_vid = g.arrays()
        sources = vid[: min(64, n_vertices)]
        dense = np.unique(g.lookup(sources))
        masks = endpoint_sets(off, nbr, dense, 3)
        ids, got = gg.walk_endpoints(csr, sources, 3)
        keep = np.flatnonzero(masks)
        assert np.array_equal(ids, o_vid[keep]) and np.array_equal(got, masks[keep])

        dist, stats = g.bfs64(g.lookup(sources), -1)
        lane, v = np.nonzero(dist >= 0)
        want = sort_rows(np.stack([sources[lane], o_vid[v], dist[lane, v].astype(np.int64)], axis=1))
        rows, st = gg.bfs64_pairs(csr, sources, -1)
        assert st == stats and np.array_equal(sort_rows(rows), want)
    finally:
        csr.close()
        g.close()
