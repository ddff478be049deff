"""Walks of 5 to 8 hops on every expansion route, against exact references.

GG_MAX_HOPS is 8 and the planner sends join chains of up to 8 edges to the device; the code that only runs past 4 hops
(k_mat_last with 5..8 parent columns, k_mat_fill's deep levels, the explicit-frontier product forms at levels >= 3,
k_mat_rows_edges with 6..9 columns, chained k_wc_pull passes, the filter at 6..7 hops, endpoint mask bits 5..8) is
checked here on the sparse multigraphs of tests/deep_graphs.py, and every case asserts that the kernels it targets were
launched, so that a changed threshold cannot quietly turn it into a repeat of a shallower test."""
import numpy as np
import pytest

from duckdb_pgq_amd import GGError, datagen
from tests import deep_graphs as D
from tests.oracle_lib import endpoint_sets, exact_walk_counts, sort_rows

pytestmark = pytest.mark.gpu

KS = [(k_min, k_max) for k_max in (5, 6, 7, 8) for k_min in sorted({1, k_max - 1, k_max})]
SHAPES = list(D.SHAPES)
MOD64 = 1 << 64


def build_both(gg, orc, vid, src, dst, rowid=None):
    gg.staging_clear()
    gg.append_vertices(vid)
    gg.append_edges(src, dst, rowid)
    csr = gg.build_csr()
    rc, g = orc.csr_build(vid, src, dst, rowid)
    assert rc == 0
    return csr, g


def launches(gg, fn):
    """fn() with every kernel launch recorded: (its result, {kernel name: number of launches})."""
    gg.profile_reset()
    gg.profile_select(None)
    gg.profile(True)
    try:
        out = fn()
    finally:
        gg.profile(False)
    counts = {name: n for name, (n, _) in gg.profile_get().items()}
    gg.profile_reset()
    return out, counts


def launched(gg, fn):
    """fn() with every kernel launch recorded: (its result, the names of the kernels it launched)."""
    out, counts = launches(gg, fn)
    return out, set(counts)


_exact = {}


def exact_counts(name, how, exact_sources):
    """exact_walk_counts of a shape and a selection, up to 8 hops, computed once (a count of h hops does not depend on
    how far the walk goes on)."""
    if (name, how) not in _exact:
        vid, src, dst = D.shape(name)
        _exact[name, how] = exact_walk_counts(vid, src, dst, 8, sources=exact_sources)
    return _exact[name, how]


def selections(name, vid, g):
    """(label, gg sources, oracle selection, exact-reference sources, range) for all sources, a list and a range."""
    sources = D.sources_of(name, vid)
    dense = g.lookup(sources)
    dense = dense[dense >= 0].astype(np.uint32)
    lo, hi = vid.size // 4, vid.size - vid.size // 5
    return [("all", None, {}, None), ("list", sources, {"sources_dense": dense}, sources),
            ("range", (lo, hi), {"lo": lo, "hi": hi}, vid[lo:hi])]


def expand(gg, csr, how, sel, k_min, k_max, materialise=False):
    if how == "range":
        return gg.expand_khop_range(csr, sel[0], sel[1], k_min, k_max, materialise=materialise)
    return gg.expand_khop(csr, k_min, k_max, sources=sel, materialise=materialise)


def read_table(res, h):
    n = res.rows(h)
    if n == 0:
        return np.zeros((0, h + 1), np.int64)
    return np.concatenate([res.fetch(h, o) for o in range(0, n, 1024)])


# ---- count mode --------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", SHAPES)
@pytest.mark.parametrize("k_min,k_max", KS)
def test_deep_counts_and_digests_under_every_frontier_form(gg, orc, name, k_min, k_max):
    """expand_khop / expand_khop_range in count mode equal the oracle's khop (rows, digests, traversed edges) under
    knobs 0 (automatic), 1 (frontier kernels), 2 (pairs + sort + k_expand_front for the last two hops) and 3
    (k_expand_mid3 over the sorted frontier); khop_count equals the exact walk counts."""
    vid, src, dst = D.shape(name)
    csr, g = build_both(gg, orc, vid, src, dst)
    try:
        for how, sel, osel, exact_sources in selections(name, vid, g):
            ref = g.khop(k_min, k_max, **osel)
            exact, exact64 = exact_counts(name, how, exact_sources)
            assert ref["rows"][k_min:k_max + 1] == exact64[k_min:k_max + 1], how
            for knob in (0, 1, 2, 3):
                gg.force_frontier(knob)
                got, names = launched(gg, lambda: expand(gg, csr, how, sel, k_min, k_max))
                assert got == ref, (how, knob)
                # the last two hops start from the frontier of level k_max - 2 (>= 3): what ran there
                last2 = exact[k_max - 1] > 0
                if knob == 1 and exact[1] > 0:
                    assert "expand_step" in names, (how, names)
                if knob == 2 and last2:
                    assert {"expand_pairs", "expand_front"} <= names, (how, names)
                if knob == 3 and last2:
                    assert "expand_front3" in names, (how, names)
                if knob == 0 and name == "funnel":  # levels of 70 000+ walks, above an eighth of the edge table
                    assert "expand_front3" in names, (how, names)
                if knob == 0 and name == "funnel_wide" and how != "range":  # > 65 536 walks, < an eighth of the table
                    assert {"expand_pairs", "expand_front"} <= names and "expand_front3" not in names, (how, names)
            gg.force_frontier(0)
            if how != "range":
                counts, names = launched(gg, lambda: gg.khop_count(csr, k_min, k_max, sources=sel))
                assert counts[k_min:k_max + 1] == exact64[k_min:k_max + 1], how
                assert "wc_pull" in names, names
    finally:
        gg.force_frontier(0)
        csr.close()
        g.close()


# ---- materialised ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", SHAPES)
@pytest.mark.parametrize("k_min,k_max", KS)
def test_deep_materialised_tables_and_their_digests(gg, orc, name, k_min, k_max):
    """Every table h in [k_min, k_max] of a materialising expansion (all sources, a source list, a range; knobs 1 and
    2) equals the oracle's rows; gg_result_digest of every table equals the count-mode digest; and the last table
    read at offsets that are not multiples of 1024, with max_rows < 1024, gives the same rows in the same places."""
    vid, src, dst = D.shape(name)
    csr, g = build_both(gg, orc, vid, src, dst)
    try:
        for how, sel, osel, exact_sources in selections(name, vid, g):
            if name == "funnel_wide" and how == "all":
                continue  # (600 000 one-hop rows into the sink: the list and the range hold the deep walks)
            want = g.khop_rows(k_min, k_max, **osel)
            counted = g.khop(k_min, k_max, **osel)
            exact, _ = exact_counts(name, how, exact_sources)
            for knob in (1, 2):
                gg.force_frontier(knob)
                got, names = launched(gg, lambda: expand(gg, csr, how, sel, k_min, k_max, materialise=True))
                for h in range(k_min, k_max + 1):
                    assert np.array_equal(sort_rows(got["tables"][h]), sort_rows(want[h])), (how, knob, h)
                if exact[k_max]:
                    assert "mat_last" in names, (how, names)  # (k_mat_front takes walks of up to 4 hops only)
                if any(exact[1:k_max]):
                    assert "mat_fill" in names, (how, names)
            gg.force_frontier(0)
            if how == "range":
                continue
            res = gg.expand_khop_result(csr, k_max, sources=sel, k_min=k_min)
            try:
                for h in range(k_min, k_max + 1):
                    assert res.digest(csr, h) == (counted["rows"][h], counted["digest"][h]), (how, h)
                full = read_table(res, k_max)
                n = full.shape[0]
                for off, m in ((1, 1000), (1023, 5), (1025, 1023), (n // 3 + 7, 999), (max(0, n - 3), 700)):
                    part = res.fetch(k_max, off, m)
                    assert np.array_equal(part, full[off:off + m]), (how, off, m)
            finally:
                res.close()
    finally:
        gg.force_frontier(0)
        csr.close()
        g.close()


def test_digest_takes_any_hops_up_to_the_result_range(gg, orc):
    """gg_result_digest accepts every hops in [k_min, k_max] of the result, 8 included, and nothing outside it."""
    vid, src, dst = D.shape("multigraph")
    csr, g = build_both(gg, orc, vid, src, dst)
    ref = g.khop(6, 8)
    res = gg.expand_khop_result(csr, 8, k_min=6)
    try:
        for h in (6, 7, 8):
            assert res.digest(csr, h) == (ref["rows"][h], ref["digest"][h])
        for h in (0, 5, 9):
            with pytest.raises(GGError):
                res.digest(csr, h)
    finally:
        res.close()
        csr.close()
        g.close()


# ---- edge rowids -------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", D.SMALL + ["funnel"])
@pytest.mark.parametrize("k", [5, 6, 7, 8])
def test_deep_walks_with_their_edge_rowids(gg, orc, name, k):
    """expand_khop_edges at 5..8 hops, with explicit non-contiguous rowids and with append positions: the vertex
    columns are the oracle's rows, edge j of every row is a table row (v_{j-1}, v_j), an edge sequence repeats only as
    often as its source does in the list, and every vertex sequence comes as often as the product of its edges'
    multiplicities (times its source's)."""
    vid, src, dst = D.shape(name)
    rowid = (np.arange(src.size, dtype=np.int64) * 13 + 5000)[::-1].copy()
    keep = np.isin(src, vid) & np.isin(dst, vid)
    mult = {}
    for a, b in zip(src[keep].tolist(), dst[keep].tolist()):
        mult[(a, b)] = mult.get((a, b), 0) + 1
    sources = D.sources_of(name, vid)
    for explicit in (True, False):
        gg.staging_clear()
        gg.set_edge_rowid(True)
        gg.append_vertices(vid)
        gg.append_edges(src, dst, rowid if explicit else None)
        csr = gg.build_csr()
        rc, g = orc.csr_build(vid, src, dst)
        assert rc == 0
        dense = g.lookup(sources)
        dense = dense[dense >= 0].astype(np.uint32)
        ids = rowid if explicit else np.arange(src.size, dtype=np.int64)
        order = np.argsort(ids)
        try:
            for srcs, osel in ((None, {}), (sources, {"sources_dense": dense})):
                if name == "funnel" and srcs is None:
                    continue  # (the list is the funnel's 70 000 sources)
                want = g.khop_rows(k, k, **osel)[k]
                res, names = launched(gg, lambda: gg.expand_khop_edges(csr, k, sources=srcs))
                try:
                    v = read_table(res, k)
                    n = res.rows(k)
                    e = (np.concatenate([res.fetch_edges(k, o) for o in range(0, n, 1024)]) if n
                         else np.zeros((0, k), np.int64))
                finally:
                    res.close()
                assert np.array_equal(sort_rows(v), sort_rows(want)), (explicit, srcs is None)
                if n:
                    assert "mat_rows_edges" in names and "mat_fill" in names, names
                at = order[np.searchsorted(ids, e, sorter=order)]
                assert np.array_equal(ids[at], e)  # every edge id is one of the table's
                for j in range(k):
                    assert np.array_equal(src[at[:, j]], v[:, j]) and np.array_equal(dst[at[:, j]], v[:, j + 1]), j
                # a walk is its sequence of edge rows: it comes once per occurrence of its source in the list
                times = (lambda v0: 1) if srcs is None else (lambda v0: int((srcs == v0).sum()))
                if n:
                    _, at_seq, counts = np.unique(e, axis=0, return_index=True, return_counts=True)
                    assert all(c == times(v[a, 0]) for a, c in zip(at_seq.tolist(), counts.tolist()))
                    rows, counts = np.unique(v, axis=0, return_counts=True)
                    for r, c in zip(rows.tolist(), counts.tolist()):
                        assert c == times(r[0]) * int(np.prod([mult[(r[j], r[j + 1])] for j in range(k)])), r
        finally:
            csr.close()
            g.close()


# ---- endpoints and the same-neighbour filter ---------------------------------------------------------------------


@pytest.mark.parametrize("name", D.SMALL + ["funnel"])
@pytest.mark.parametrize("k_max", [5, 6, 7, 8])
def test_deep_walk_endpoints(gg, orc, name, k_max):
    """gg_walk_endpoints with mask bits up to 8 against the set images of the oracle's CSR."""
    vid, src, dst = D.shape(name)
    csr, g = build_both(gg, orc, vid, src, dst)
    o_off, o_nbr, _, o_vid = g.arrays()
    try:
        for sources in (D.sources_of(name, vid), vid[[3, 3]], np.array([-5], np.int64)):
            dense = g.lookup(sources)
            dense = np.unique(dense[dense >= 0])
            want = endpoint_sets(o_off, o_nbr, dense, k_max)
            ids, masks = gg.walk_endpoints(csr, sources, k_max)
            keep = np.flatnonzero(want)
            assert np.array_equal(ids, o_vid[keep]) and np.array_equal(masks, want[keep])
    finally:
        csr.close()
        g.close()


@pytest.mark.parametrize("name", ["multigraph", "cycle_chords", "hub"])
def test_same_neighbour_filter_at_depth(gg, orc, name):
    """gg_result_filter_common_neighbour over 5-, 6- and 7-hop tables (its output at 7 hops fills the last column slot)
    against a plain restatement: for every path row and every filter neighbour w of v0, the row (w, v0..vh) comes
    prod_c mult(v_c, w) times.  8 hops are refused: the output would need a tenth column."""
    vid, src, dst = D.shape(name)
    rng = np.random.default_rng(91)
    sensors = vid.max() + 1000 + np.arange(3, dtype=np.int64)
    # most vertices watched by sensor 0 (some twice), a few by sensor 1 as well or instead, some by none
    m_src, m_dst = [], []
    for v in vid.tolist():
        r = rng.random()
        ws = [0] if r < 0.75 else [0, 0] if r < 0.85 else [0, 1] if r < 0.93 else [1] if r < 0.97 else []
        for w in ws:
            m_src.append(v)
            m_dst.append(int(sensors[w]))
    m_src, m_dst = np.array(m_src, np.int64), np.array(m_dst, np.int64)
    mult = {}
    for a, b in zip(m_src.tolist(), m_dst.tolist()):
        mult[(a, b)] = mult.get((a, b), 0) + 1
    rc, g = orc.csr_build(vid, src, dst)
    assert rc == 0
    gg.staging_clear()
    gg.append_vertices(np.concatenate([vid, sensors]))
    gg.append_edges(src, dst)
    path_csr = gg.build_csr()
    gg.staging_clear_edges()
    gg.append_edges(m_src, m_dst)
    filter_csr = gg.build_csr()
    try:
        for hops in (5, 6, 7):
            paths = g.khop_rows(hops, hops)[hops]
            want = []
            for r in paths.tolist():
                for w in sensors.tolist():
                    m = int(np.prod([mult.get((v, w), 0) for v in r]))
                    want += [[w] + r] * m
            want = np.array(want, np.int64).reshape(-1, hops + 2)
            got, names = launched(gg, lambda: gg.connected_paths_same_neighbour(path_csr, filter_csr, hops))
            assert np.array_equal(sort_rows(got), sort_rows(want)), hops
            if want.shape[0]:
                assert "filter_fill" in names, names
        with pytest.raises(GGError):
            gg.connected_paths_same_neighbour(path_csr, filter_csr, 8)
    finally:
        path_csr.close()
        filter_csr.close()
        g.close()


# ---- sizes the oracle cannot enumerate ---------------------------------------------------------------------------


def test_walk_counts_past_two_to_the_32(gg):
    """khop_count at 8 hops on 10^5 vertices (power-law degrees, ~10 rows per vertex): per-vertex walk counts and the
    totals pass 2^32; they must be the exact counts mod 2^64, from every vertex and from a source list."""
    vid, src, dst = datagen.ldbc_knows(100_000, 1_000_000, 0xD33B)
    gg.staging_clear()
    gg.append_vertices(vid)
    gg.append_edges(src, dst)
    csr = gg.build_csr()
    sources = np.concatenate([datagen.pick_sources(vid, 5000, 3), vid[:10], np.array([-2], np.int64)])
    try:
        for sel in (None, sources):
            exact, exact64, w_max = exact_walk_counts(vid, src, dst, 8, sources=sel, with_max=True)
            assert exact[8] > 1 << 32 and exact[5] > 1 << 32
            assert w_max[7] > 1 << 32  # (one vertex's walk count: what a 32-bit per-vertex weight would wrap)
            counts, names = launched(gg, lambda: gg.khop_count(csr, 1, 8, sources=sel))
            assert counts[1:9] == exact64[1:9], sel is None
            assert "wc_pull" in names
    finally:
        csr.close()


def test_walk_counts_past_two_to_the_64(gg):
    """Three vertices with 300 parallel rows per ordered pair (self-loops included): 3 * 900^h walks, past 2^64 from
    7 hops on.  khop_count must give the exact counts mod 2^64 (the counting expansion is not asked: 10^24 walks)."""
    vid = np.array([11, -4, 1 << 50], np.int64)
    pairs = [(a, b) for a in vid for b in vid]
    src = np.repeat(np.array([a for a, _ in pairs], np.int64), 300)
    dst = np.repeat(np.array([b for _, b in pairs], np.int64), 300)
    gg.staging_clear()
    gg.append_vertices(vid)
    gg.append_edges(src, dst)
    csr = gg.build_csr()
    try:
        for sel in (None, np.array([11, 11, 99, 1 << 50], np.int64)):
            exact, exact64 = exact_walk_counts(vid, src, dst, 8, sources=sel)
            assert exact[8] > MOD64 and exact[7] > MOD64
            for k_min in (1, 7, 8):
                counts = gg.khop_count(csr, k_min, 8, sources=sel)
                assert counts[k_min:9] == exact64[k_min:9], (sel is None, k_min)
    finally:
        csr.close()


def test_hundreds_of_millions_of_deep_walks(gg):
    """10^6 vertices, 2.5 * 10^6 rows: 10^8 walks of 5 hops and 2.5 * 10^8 of 6.  Counts equal the exact reference and
    the digests agree across the four frontier forms; one materialised 5-hop result's digest, read where it lies, is
    the count digest; k_expand_mid3 split over many launches (nonzero first tile, levels >= 3) equals the unsplit run."""
    vid, src, dst = datagen.small_graph(1_000_000, 2_500_000, 0xB16, dangling=100, dup_edges=1000)
    gg.staging_clear()
    gg.append_vertices(vid)
    gg.append_edges(src, dst)
    csr = gg.build_csr()
    try:
        exact, exact64 = exact_walk_counts(vid, src, dst, 6)
        assert exact[5] > 5 * 10 ** 7 and exact[6] > 10 ** 8
        for k_min, k_max in ((5, 5), (1, 6), (6, 6)):
            runs = {}
            for knob in (0, 1, 2, 3):
                gg.force_frontier(knob)
                runs[knob] = gg.expand_khop(csr, k_min, k_max)
                assert runs[knob]["rows"][k_min:k_max + 1] == exact64[k_min:k_max + 1], (knob, k_min, k_max)
                assert runs[knob] == runs[0], (knob, k_min, k_max)
            _, whole = launches(gg, lambda: gg.expand_khop(csr, k_min, k_max))
            gg.max_grid_tiles(7)
            split, parts = launches(gg, lambda: gg.expand_khop(csr, k_min, k_max))
            assert split == runs[3], (k_min, k_max)
            # several launches, every one after the first with a nonzero first tile
            assert parts.get("expand_front3", 0) > max(1, whole.get("expand_front3", 0)), (k_min, k_max, parts, whole)
            gg.max_grid_tiles(0)
            gg.force_frontier(0)
        res = gg.expand_khop_result(csr, 5)
        try:
            n, dig = res.digest(csr, 5)
            assert n == exact[5] and dig == gg.expand_khop(csr, 5, 5)["digest"][5]
        finally:
            res.close()
    finally:
        gg.force_frontier(0)
        gg.max_grid_tiles(0)
        csr.close()
