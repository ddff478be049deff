"""GG.triangles (gg_triangles) against the numpy restatement (tests/triangles_ref.py): count, digest, wedges and the
materialised rows, for both orders, on every route the kernel has (LDS-staged and global in-rows, split launches) and
on every build form.  The 2^32-row refusal of the materialising form cannot be reached at test size; it is checked by
reading csrc/gg_triangles.hip only."""
import numpy as np
import pytest

from duckdb_pgq_amd import GGError
from tests import triangles_ref as T
from tests.oracle_lib import sort_rows

pytestmark = pytest.mark.gpu

GG_ERR_INVALID_ARG, GG_ERR_STATE = -1, -6


@pytest.fixture(scope="module")
def hard(orc):
    """the graph and, per order, what the restatement says: (sorted id rows, rows, digest, wedges)"""
    vid, src, dst = T.hard_graph()
    g = T.TriangleGraph(vid, src, dst)
    want = {}
    for order in (0, 1):
        rows, wedges = g.rows(order)
        want[order] = (sort_rows(g.id_rows(rows)), rows.shape[0], orc.digest_rows(rows.astype(np.uint32)), wedges)
    hub_in = int(np.bincount(g.dv, minlength=g.V).max())
    assert hub_in > 500 and want[0][1] > want[1][1] > 0  # the hub's in-row is the long one; both orders have rows
    return vid, src, dst, g, want


def build(gg, vid, src, dst):
    gg.staging_clear()
    gg.append_vertices(np.asarray(vid, np.int64))
    gg.append_edges(np.asarray(src, np.int64), np.asarray(dst, np.int64))
    return gg.build_csr()


def fetch_all(res):
    n = res.rows(2)
    parts = [res.fetch(2, o) for o in range(0, n, 1024)]
    return np.concatenate(parts, axis=0) if parts else np.empty((0, 3), np.int64)


def check(gg, csr, want, order, sources=None):
    rows_sorted, n, digest, wedges = want
    st = gg.triangles(csr, sources, ordered=bool(order))
    print("order", order, "device", st, "restatement", {"rows": n, "digest": digest, "wedges": wedges})
    assert st == {"rows": n, "digest": digest, "wedges": wedges}
    st2, res = gg.triangles(csr, sources, ordered=bool(order), materialise=True)
    try:
        assert st2 == st and res.rows(2) == n
        assert res.digest(csr, 2) == (n, digest)  # gg_result_digest of the rows = the count-mode digest
        assert np.array_equal(sort_rows(fetch_all(res)), rows_sorted)
    finally:
        res.close()


ROUTES = ["default", "tile64", "grid3", "legacy_build", "no_rowid"]


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("route", ROUTES)
def test_every_route_equals_the_restatement(gg, hard, route, order):
    vid, src, dst, g, want = hard
    if route == "legacy_build":
        gg.force_legacy_build(True)
    if route == "no_rowid":
        gg.set_edge_rowid(False)
    csr = build(gg, vid, src, dst)
    if route == "tile64":
        gg.debug_triangle_tile(64)  # the hub's in-row (> 500 entries) no longer fits: searched in global memory
    if route == "grid3":
        gg.max_grid_tiles(3)
    try:
        check(gg, csr, want[order], order)
    finally:
        csr.close()


@pytest.mark.parametrize("order", [0, 1])
def test_source_lists(gg, hard, orc, order):
    vid, src, dst, g, want = hard
    csr = build(gg, vid, src, dst)
    try:
        hub = int(vid[np.bincount(g.dv, minlength=g.V).argmax()])
        lists = [[hub], [hub, -123456789, int(vid[0]), hub, int(vid[1])], []]
        for sources in lists:
            rows, wedges = g.rows(order, sources)
            check(gg, csr, (sort_rows(g.id_rows(rows)), rows.shape[0], orc.digest_rows(rows.astype(np.uint32)), wedges),
                  order, np.asarray(sources, np.int64))
        assert gg.triangles(csr, np.empty(0, np.int64), ordered=bool(order)) == {"rows": 0, "digest": 0, "wedges": 0}
    finally:
        csr.close()


def test_degenerate_graphs(gg):
    vid = np.array([10, 20, 30], np.int64)
    cases = [
        ([], [], 0, 0),                          # no edges
        ([10], [10], 1, 0),                      # a single self-loop
        ([10, 20, 30], [20, 30, 10], 3, 1),      # a directed 3-cycle stored once, ids ascending along it
        ([30, 20, 10], [20, 10, 30], 3, 0),      # ... ids descending along it
    ]
    for src, dst, n0, n1 in cases:
        csr = build(gg, vid, np.array(src, np.int64), np.array(dst, np.int64))
        try:
            g = T.TriangleGraph(vid, src, dst)
            for order, n in ((0, n0), (1, n1)):
                st, res = gg.triangles(csr, ordered=bool(order), materialise=True)
                try:
                    assert st["rows"] == n == res.rows(2) == g.rows(order)[0].shape[0]
                    assert np.array_equal(sort_rows(fetch_all(res)), sort_rows(g.id_rows(g.rows(order)[0])))
                finally:
                    res.close()
        finally:
            csr.close()


def test_errors_leave_the_context_usable(gg, hard):
    import ctypes as C

    from duckdb_pgq_amd.gg import TriStats

    vid, src, dst, g, want = hard
    gg.staging_clear()
    gg.append_vertices(vid)
    gg.append_edges(src, dst)
    shard = gg.build_csr_shard(0, 2)
    csr = gg.build_csr()
    try:
        with pytest.raises(GGError) as e:
            gg.triangles(shard)
        assert e.value.code == GG_ERR_STATE
        st, res = TriStats(), C.c_void_p()
        assert gg.lib.gg_triangles(gg.ctx, csr.handle, None, 0, 2, 0, C.byref(st), C.byref(res)) == GG_ERR_INVALID_ARG
        assert gg.triangles(csr, ordered=True)["rows"] == want[1][1]
    finally:
        shard.close()
        csr.close()
