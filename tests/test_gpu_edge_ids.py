"""The operations written after tests/test_gpu_build_forms.py — triangles and triangle edges, khop_aggregate,
khop_aggregate_top, khop_pair_counts, components, all shortest paths, filter_edge, extend_edge, group_by — on vertex ids at
the 32-bit and 64-bit boundaries and under every id dictionary (tests/edge_ids.py: the placements and why each takes the
dictionary it names), each against the restatement the suite already has, fed (vid, src, dst) of the same graph.  Every
comparison is between integers and exact.  tests/test_edge_ids_cpu.py proves that none of the answers is empty and that
each holds an edge id.

The checks are the ones of each operation's own test module, called on these graphs, so every property those assert
(stats, digests, order, determinism, the count-only forms) is asserted here too.

Ordered triangles rank the vertices by id (tri_ranks, csrc/gg_triangles.hip): ids whose 32-bit halves equal 0xFFFFFFFF, the
shared radix sort's "no element" key, are what that ranking once lost; V = 1 and V = 2 are where one lost element empties
the sort."""
import numpy as np
import pytest

from tests import all_shortest_paths_ref as AP
from tests import edge_filter_ref as F
from tests import edge_ids as EI
from tests import extend_ref as X
from tests import khop_aggregate_ref as K
from tests import khop_aggregate_top_ref as TOP
from tests import shortest_path_ref as SP
from tests import test_gpu_all_shortest_paths as t_all_paths
from tests import test_gpu_components as t_components
from tests import test_gpu_edge_filter as t_filter
from tests import test_gpu_extend as t_extend
from tests import test_gpu_group_by as t_group
from tests import test_gpu_khop_aggregate as t_aggregate
from tests import test_gpu_khop_aggregate_top as t_top
from tests import test_gpu_khop_pair_counts as t_pairs
from tests import test_gpu_triangle_edges as t_tri_edges
from tests import test_gpu_triangles as t_triangles
from tests import triangle_edges_ref as E
from tests import triangles_ref as T
from tests.oracle_lib import sort_rows

pytestmark = pytest.mark.gpu


def _build(ctx, vid, src, dst):
    ctx.staging_clear()
    ctx.append_vertices(np.asarray(vid, np.int64))
    ctx.append_edges(np.asarray(src, np.int64), np.asarray(dst, np.int64))
    return ctx.build_csr()


@pytest.fixture(scope="module", params=EI.PLACEMENTS)
def placed(request, _gg_session):
    """(the placement's graph, its references, its CSR by the default build with rowids): one build per placement for the
    tests that only read it"""
    eg = EI.edge_graph(request.param)
    _gg_session.debug_reset()
    csr = _build(_gg_session, eg.vid, eg.src, eg.dst)
    g = eg.tri
    assert (csr.V, csr.E) == (g.V, g.su.size) and csr.dropped == eg.src.size - g.su.size > 0
    off, nbr, eid, vid = csr.export()
    want = AP.csr_of(eg.vid, eg.src, eg.dst)
    for got, w in zip((off, nbr, eid, vid), want):
        assert np.array_equal(got, w)  # the restatements below may read either
    yield eg, EI.references(eg), csr
    csr.close()


# ---- triangles ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["all", "list"])
@pytest.mark.parametrize("order", [0, 1])
def test_triangles_count_and_rows(gg, orc, placed, order, which):
    eg, ref, csr = placed
    g = eg.tri
    rows, wedges = ref["triangles"][(order, which)]
    want = (sort_rows(g.id_rows(rows)), rows.shape[0], orc.digest_rows(rows.astype(np.uint32)), wedges)
    t_triangles.check(gg, csr, want, order, None if which == "all" else ref["sources"])


@pytest.mark.parametrize("which", ["all", "list"])
@pytest.mark.parametrize("order", [0, 1])
def test_triangle_edges(gg, placed, order, which):
    eg, ref, csr = placed
    sources = None if which == "all" else ref["sources"]
    want = E.rows(eg.vid, eg.src, eg.dst, None, order, sources)
    assert want.shape[0] == ref["triangles"][(order, which)][0].shape[0] > 0
    t_tri_edges.check(gg, csr, sort_rows(want), order, sources)


@pytest.mark.parametrize("name", ["one_vertex", "two_vertices"])
def test_one_and_two_vertices(gg, name):
    """V = 1 (the id -1) and V = 2 (-1 and INT64_MAX, joined both ways): no triangle rows in either order, and the
    components"""
    vid, src, dst = EI.tiny_graphs()[name]
    g = T.TriangleGraph(vid, src, dst)
    csr = _build(gg, vid, src, dst)
    try:
        for order in (0, 1):
            rows, wedges = g.rows(order)
            assert rows.shape[0] == 0
            for sources in (None, vid[::-1].copy(), EI.LISTED):
                w = wedges if sources is None else g.rows(order, sources)[1]
                assert gg.triangles(csr, sources, ordered=bool(order)) == {"rows": 0, "digest": 0, "wedges": w}
                st, res = gg.triangles(csr, sources, ordered=bool(order), materialise=True)
                try:
                    assert st["rows"] == res.rows(2) == 0 and st["wedges"] == w
                finally:
                    res.close()
                st, res = gg.triangles_edges(csr, sources, ordered=bool(order))
                try:
                    assert st["rows"] == res.rows(2) == 0 and st["wedges"] == w
                finally:
                    res.close()
        assert g.rows(0)[1] == (2 if name == "two_vertices" else 0) and g.rows(1)[1] == 0
        want = t_components.K.components(vid, src, dst)
        got = t_components.check(gg, csr, want)
        assert got["components"].tolist() == [-1] and got["sizes"].tolist() == [vid.size]
    finally:
        csr.close()


# ---- aggregates --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group_by", K.GROUPS)
def test_khop_aggregate(gg, placed, group_by):
    eg, ref, csr = placed
    t_aggregate.check(gg, csr, eg.tri, 1, 2, group_by, None, ref["weights"], ref["aggregate"][(group_by, False)])


@pytest.mark.parametrize("group_by", K.GROUPS)
def test_khop_aggregate_top_when_the_id_alone_decides(gg, placed, group_by):
    """All weights zero: every group ties on the total, so the id word alone orders the rows — ascending, signed, in both
    directions; and ordered by walks, where ties are frequent.  n below, at and above the group count."""
    eg, ref, csr = placed
    zeros = np.zeros(eg.vid.size, np.int64)
    levels = ref["aggregate"][(group_by, True)]
    agg = gg.khop_aggregate(csr, 1, 2, group_by, None, zeros)
    try:
        for h in (1, 2):
            G = len(levels[h][1])
            assert K.same(agg.fetch(h), levels[h]) and G > 24
            for n in (1, 24, G - 1, G, G + 1):
                for order_by, descending in t_top.EVERY_ORDER:
                    got, st = t_top.check_top(gg, agg, levels[h], h, n, order_by, descending)
                    if order_by == "total":  # pinned without the restatement: the ids ascend as signed integers
                        ids = [int(x) for x in got[0]]
                        assert ids == sorted(int(x) for x in levels[h][0])[:n]
            for route in (1, 2):  # both sort routes of the survivors
                gg.debug_aggregate_top(route, 0)
                t_top.check_top(gg, agg, levels[h], h, G, "total", True, forced=route)
                t_top.check_top(gg, agg, levels[h], h, 30, "walks", False, forced=route)
            gg.debug_aggregate_top(0, 0)
    finally:
        agg.close()


def test_khop_aggregate_top_of_weighted_totals(gg, placed):
    eg, ref, csr = placed
    levels = ref["aggregate"][("end", False)]
    agg = gg.khop_aggregate(csr, 1, 2, "end", None, ref["weights"])
    try:
        G = len(levels[2][1])
        for n in (7, G):
            for order_by, descending in t_top.EVERY_ORDER:
                t_top.check_top(gg, agg, levels[2], 2, n, order_by, descending)
    finally:
        agg.close()


def test_khop_pair_counts(gg, placed):
    eg, ref, csr = placed
    t_pairs.check(gg, csr, eg.tri, 1, 2, ref["sources"], ref["pair_targets"], ref["pair_counts"])
    t_pairs.check(gg, csr, eg.tri, 1, 2, ref["sources"], None, ref["pair_counts_all"])


# ---- components --------------------------------------------------------------------------------------------------------
def test_components(gg, placed):
    eg, ref, csr = placed
    t_components.check(gg, csr, ref["components"])
    few = _build(gg, eg.vid, *ref["few_rows"])  # many components, one of them the 24 wired vertices
    try:
        got = t_components.check(gg, few, ref["components_few_rows"])
        assert np.isin(got["components"], eg.wired).sum() == 1
    finally:
        few.close()


# ---- shortest paths ----------------------------------------------------------------------------------------------------
def test_bfs_pairs_and_shortest_paths_between_edge_ids(gg, placed):
    eg, ref, csr = placed
    off, nbr, eid, vid = AP.csr_of(eg.vid, eg.src, eg.dst)
    s, t = EI.path_pairs(eg)
    for max_hops in (-1, 2):
        want = SP.shortest_paths(off, nbr, eid, vid, s, t, max_hops, True)
        got = gg.shortest_paths(csr, s, t, max_hops, True)
        assert want[0].size > 0
        for name, a, b in zip(("pair", "step", "vertex", "edge"), got, want):
            assert a.dtype == b.dtype and np.array_equal(a, b), (name, max_hops)
        t_all_paths.check_pairs(gg, csr, s, t, max_hops)
        t_all_paths.check_pairs(gg, csr, s, t, max_hops, path_limit=2, edges=False)
        # the reached (source, vertex, distance) rows of one batch: its sources are the distinct ends that are vertices
        sources = np.unique(s[np.isin(s, eg.vid)])
        assert 8 < sources.size <= 64
        index = eg.tri.index
        rows = []
        for src_id in sources.tolist():
            dist = SP.bfs_dist(off, nbr, index[src_id], max_hops)
            v = np.flatnonzero(dist >= 0)
            rows.append(np.stack([np.full(v.size, src_id, np.int64), eg.vid[v], dist[v]], axis=1))
        got_rows, st = gg.bfs64_pairs(csr, sources, max_hops)
        assert np.array_equal(sort_rows(got_rows), sort_rows(np.concatenate(rows)))
        assert st["reached_pairs"] == got_rows.shape[0]


# ---- walk tables probed against a second CSR ---------------------------------------------------------------------------
def _table(gg, ref, csr):
    """the 2-hop table of a source list of edge ids; the second CSR of every call below is the table's own, so the probed
    cells are edge ids (on `wide` one of them is INT64_MIN, the 16-byte table's empty key)"""
    table = gg.expand_khop_result(csr, EI.TABLE_HOPS, ref["table_sources"])
    try:
        assert np.array_equal(t_extend.fetch_all(table, EI.TABLE_HOPS), ref["table"])
    except BaseException:
        table.close()
        raise
    return table


def _filter_edge(gg, orc, eg, ref, csr, table):
    for fc, tc in EI.FILTER_COLUMNS:
        for mode in F.MODES:
            st, _ = t_filter.check(gg, orc, csr, eg.tri, table, ref["table_dense"], EI.TABLE_HOPS, fc, tc, mode)
            assert st == ref["filter"][(fc, tc, mode)][1] and st["rows_out"] > 0


def _extend_edge(gg, eg, ref, csr, table):
    hops = EI.TABLE_HOPS
    for fc in range(hops + 1):
        want_rows, want_rid, want = ref["extend"][fc]
        count_only = gg.extend_edge(table, hops, csr, fc, materialise=False)
        for edges in (False, True):
            st, res = gg.extend_edge(table, hops, csr, fc, edges=edges)
            try:
                print(fc, edges, "device", st, "restatement", want)
                assert st == want == count_only and res.rows(hops + 1) == want["rows_out"] > 0
                assert res.digest(csr, hops + 1) == (want["rows_out"],
                                                     F.digest_dense_rows(X.dense_rows(eg.tri.index, want_rows)))
                assert np.array_equal(t_extend.fetch_all(res, hops + 1), want_rows)
                if edges:
                    assert np.array_equal(t_extend.fetch_all(res, hops + 1, edges=True)[:, hops], want_rid)
            finally:
                res.close()


def _group_by(gg, eg, ref, csr, table):
    w = ref["weights"]
    for route in (1, 2):
        gg.debug_group(route)
        for (kc, wc), (want, want_st) in ref["group_by"].items():
            st, got = t_group.check(gg, table, EI.TABLE_HOPS, ref["table"], kc, csr, eg.vid, wc, None, None,
                                    None if wc is None else w, route=t_group.route_for(csr.V, wc is not None, route))
            assert K.same(got, want) and {k: v for k, v in st.items() if k != "route"} == want_st
    gg.debug_group(0)
    # the top of a grouped table whose keys are edge ids: ties on walks are broken by the signed id
    kc = EI.TABLE_HOPS
    level = ref["group_by"][(kc, None)][0]
    agg = gg.group_by(table, EI.TABLE_HOPS, kc, csr)
    try:
        for descending in (True, False):
            top = gg.khop_aggregate_top(agg, EI.TABLE_HOPS, "walks", descending, 40)
            try:
                assert K.same(top.fetch(EI.TABLE_HOPS), TOP.top(level, 40, "walks", descending))
            finally:
                top.close()
    finally:
        agg.close()


def test_filter_edge(gg, orc, placed):
    eg, ref, csr = placed
    table = _table(gg, ref, csr)
    try:
        _filter_edge(gg, orc, eg, ref, csr, table)
    finally:
        table.close()


def test_extend_edge(gg, placed):
    eg, ref, csr = placed
    table = _table(gg, ref, csr)
    try:
        _extend_edge(gg, eg, ref, csr, table)
    finally:
        table.close()


def test_group_by_on_both_routes(gg, placed):
    eg, ref, csr = placed
    table = _table(gg, ref, csr)
    try:
        _group_by(gg, eg, ref, csr, table)
    finally:
        table.close()


@pytest.mark.parametrize("op", ["filter_edge", "extend_edge", "group_by"])
def test_wide_ids_on_the_multipass_build(gg, orc, op):
    """the same three on a CSR of the multi-pass build (gg_debug_force_legacy_build), which fills the 16-byte id table on
    first use (ensure_ht) instead of during the build"""
    eg = EI.edge_graph("wide")
    ref = EI.references(eg)
    gg.force_legacy_build(True)
    csr = _build(gg, eg.vid, eg.src, eg.dst)
    table = None
    try:
        table = _table(gg, ref, csr)
        if op == "filter_edge":
            _filter_edge(gg, orc, eg, ref, csr, table)
        elif op == "extend_edge":
            _extend_edge(gg, eg, ref, csr, table)
        else:
            _group_by(gg, eg, ref, csr, table)
    finally:
        if table is not None:
            table.close()
        csr.close()
