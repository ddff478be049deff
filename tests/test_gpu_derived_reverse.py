"""The derived reverse CSR (gg_csr_fast.hip "Derived reverse"): where EVERY row i + E/2 of the edge table is row i with
source and destination swapped, the vertex-sorted bucketed build partitions and sorts the forward entries only and
writes the reverse CSR as the forward rows rotated.  Its arrays must equal, bit for bit, a numpy stable sort of the
kept rows by destination and the arrays of a context created with GG_MIRROR_REVERSE=0 (the sorted reverse); tables
and builds the derivation does not apply to must say so (reverse_derived == 0) and give the same arrays as ever."""
import os

import numpy as np
import pytest

import duckdb_pgq_amd as pkg
from duckdb_pgq_amd import datagen, sharding
from duckdb_pgq_amd.gg import GG_CHUNK_ROWS

pytestmark = pytest.mark.gpu

TILE = 8192  # rows per tile of the densification and the partition (FB_TILE)


def _ctx_with_env(name):
    old = os.environ.get(name)
    os.environ[name] = "0"
    try:
        return pkg.GG(0)
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


@pytest.fixture(scope="module")
def gg_sorted():
    """A second context that never derives: GG_MIRROR_REVERSE=0 at its creation."""
    g = _ctx_with_env("GG_MIRROR_REVERSE")
    yield g
    g.close()


@pytest.fixture(scope="module")
def gg_unpaired():
    """A context without the pairing at all (GG_MIRROR_PAIRS=0 implies no derivation)."""
    g = _ctx_with_env("GG_MIRROR_PAIRS")
    yield g
    g.close()


# ---- tables (the shapes of tests/test_gpu_mirrored_tables.py) ----------------------------------------------------------
def _ids(kind, V, rng):
    if kind == "sparse":  # packed 8-byte dictionary slots
        return datagen.person_ids(V, 11)
    if kind == "dense":   # span < 2^20: direct-address array
        return (np.arange(V, dtype=np.int64) * 2 - 77)[rng.permutation(V)]
    if kind == "wide":    # arbitrary 64-bit ids: 16-byte slots
        ids = np.unique(rng.integers(np.iinfo(np.int64).min, np.iinfo(np.int64).max, V + V // 8, dtype=np.int64))
        return ids[rng.permutation(ids.size)][:V]
    raise AssertionError(kind)


def _half(vid, h, rng, extras=False):
    s = vid[rng.integers(0, vid.size, h)]
    d = vid[rng.integers(0, vid.size, h)]
    if extras and h >= 64:  # self loops, duplicate rows, ids that are no vertex
        s[:8] = d[:8]
        s[8:24], d[8:24] = s[24:40], d[24:40]
        bad = np.int64(int(vid.max()) + 1) if int(vid.max()) < np.iinfo(np.int64).max else np.int64(int(vid.min()) - 1)
        s[40:48] = bad
        d[48:56] = bad
        s[56:64] = d[56:64] = bad
    return s, d


def mirrored(vid, E, rng, extras=False):
    """E rows; row i + E // 2 = (dst[i], src[i]) for i < E // 2, row E - 1 of an odd E on its own."""
    h = E // 2
    s, d = _half(vid, h, rng, extras)
    src, dst = np.concatenate([s, d]), np.concatenate([d, s])
    if E % 2:
        src = np.append(src, vid[rng.integers(0, vid.size)])
        dst = np.append(dst, vid[rng.integers(0, vid.size)])
    return src.astype(np.int64), dst.astype(np.int64)


def _break(vid, src, dst, rows, rng):
    """Rows whose destination is drawn again (a different id each: the pair is certainly not mirrored any more)."""
    src, dst = src.copy(), dst.copy()
    pos = {int(x): i for i, x in enumerate(vid)}
    for r in rows:
        dst[r] = vid[(pos[int(dst[r])] + 1 + int(rng.integers(0, vid.size - 1))) % vid.size]
    return src, dst


def _shaped(vid, E, shape, rng):
    src, dst = mirrored(vid, E, rng)
    h = E // 2
    if shape == "one_per_tile":
        rows = h + np.arange(0, h, TILE) + rng.integers(0, 512, (h + TILE - 1) // TILE)
        src, dst = _break(vid, src, dst, np.minimum(rows, 2 * h - 1), rng)
    elif shape == "last_pair":
        src, dst = _break(vid, src, dst, [2 * h - 1], rng)
    elif shape == "offset_by_one":  # the second half one row late: row i + h + 1 mirrors row i
        src = np.concatenate([src[:h], vid[:1], src[h:E - 1]])
        dst = np.concatenate([dst[:h], vid[1:2], dst[h:E - 1]])
    elif shape == "permuted_half":  # the second half holds the mirror of every first-half row, in another order
        p = h + rng.permutation(h)
        src, dst = np.concatenate([src[:h], src[p]]), np.concatenate([dst[:h], dst[p]])
    elif shape == "a_tenth":  # too few pairs for the paired walk to pay
        src, dst = _break(vid, src, dst, h + np.flatnonzero(rng.random(h) < 0.9), rng)
    elif shape == "shuffled":  # no pair at all
        p = rng.permutation(src.size)
        src, dst = src[p], dst[p]
    else:
        assert shape == "full", shape
    assert src.size == E and dst.size == E
    return src, dst


# ---- reference and comparison --------------------------------------------------------------------------------------
def reverse_reference(o_vid, src, dst, by_source=False, owned_part=None):
    """numpy on the host: dense (u, v) of the kept rows in rowid order, stable sort by v, bincount.  by_source: inside
    a row the sources ascend (the order of the lazily built reverse CSR of the multi-pass build).  owned_part: (part,
    n_parts), only the rows whose destination that shard owns."""
    order = np.argsort(o_vid, kind="stable")
    sv = o_vid[order]

    def dense(ids):
        if sv.size == 0:
            return np.full(ids.size, -1, np.int64)
        p = np.minimum(np.searchsorted(sv, ids), sv.size - 1)
        return np.where(sv[p] == ids, order[p], -1).astype(np.int64)

    u, v = dense(src), dense(dst)
    keep = (u >= 0) & (v >= 0)
    if owned_part is not None:
        keep &= sharding.owner_of(dst, owned_part[1]) == owned_part[0]
    u, v = u[keep], v[keep]
    o = np.lexsort((u, v)) if by_source else np.argsort(v, kind="stable")
    roff = np.concatenate([[0], np.cumsum(np.bincount(v, minlength=o_vid.size))]).astype(np.int64)
    return roff, u[o], v[o]


def _rows(ctx, csr, h):
    res = ctx.expand_khop_result(csr, h)
    try:
        n = res.rows(h)
        parts = [res.fetch(h, o) for o in range(0, n, GG_CHUNK_ROWS)]
        return np.concatenate(parts) if parts else np.zeros((0, h + 1), np.int64)
    finally:
        res.close()


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def check(gg, gg_sorted, orc, vid, src, dst, derived, rowid=False, rank=1, legacy=False, main=None, rows=False):
    """Build on `main` (default: gg) and on the never-deriving context; everything listed in the module docstring."""
    main = gg if main is None else main
    rc, g = orc.csr_build(vid, src, dst)
    assert rc == 0
    try:
        o_arr = g.arrays()
        want_rev = reverse_reference(o_arr[3], src, dst, by_source=legacy)
        want_khop = g.khop(1, 2)
        sources = datagen.pick_sources(vid, 64, 1)
        want_dist, want_bfs = g.bfs64(g.lookup(sources), 5)
        got_rows = []
        for ctx in (main, gg_sorted):
            ctx.staging_clear()
            ctx.set_edge_rowid(rowid)
            ctx.rank_mode(rank)
            ctx.force_legacy_build(legacy)
            ctx.append_vertices(vid)
            ctx.append_edges(src, dst)
            csr = ctx.build_csr()
            try:
                tag = "main" if ctx is main else "GG_MIRROR_REVERSE=0"
                assert csr.reverse_derived == (derived if ctx is main else 0), tag
                assert (csr.V, csr.E, csr.dropped) == (g.V, g.E, g.dropped), tag
                rev = csr.export_reverse()
                for name, a, b in zip(("roff", "rnbr", "rrow"), rev, want_rev):
                    assert np.array_equal(a, b), (tag, name)
                off, nbr, eid, v2 = csr.export()
                assert _same((off, nbr, v2), (o_arr[0], o_arr[1], o_arr[3])), tag
                assert np.array_equal(eid, o_arr[2]) if rowid else np.all(eid == -1), tag
                assert ctx.expand_khop(csr, 1, 2) == want_khop, tag
                dist, st = ctx.bfs64(csr, sources, 5)
                assert np.array_equal(dist, want_dist) and st == want_bfs, tag
                if rows:
                    got_rows.append(_rows(ctx, csr, 2))
            finally:
                csr.close()
        if rows:  # the materialised 2-hop rows, row for row and in order
            assert got_rows[0].shape == got_rows[1].shape and np.array_equal(got_rows[0], got_rows[1])
            assert got_rows[0].shape[0] == want_khop["rows"][2]
    finally:
        for ctx in (main, gg_sorted):
            ctx.debug_reset()
            ctx.staging_clear()
        g.close()


# ---- must derive ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [2, 2 * TILE, 2 * TILE + 2, 2 * 3 * TILE + 2 * 1234])
def test_fully_mirrored_tables_derive(gg, gg_sorted, orc, E):
    """h = 1, h a multiple of the tile, a partial last first-half tile; the 2-hop rows in full."""
    rng = np.random.default_rng(E)
    vid = _ids("sparse", 3000, rng)
    src, dst = mirrored(vid, E, rng)
    check(gg, gg_sorted, orc, vid, src, dst, 1, rows=True)


@pytest.mark.parametrize("V,E", [(1, 2 * 700), (7, 2 * 3000), (1024, 300_000), (70_000, 600_000)])
def test_vertex_counts_and_bucket_shapes_derive(gg, gg_sorted, orc, V, E):
    """One vertex (all self-loops); fewer vertices than a group of k_vrows; one bucket per half with more chunks than
    k_vrows takes at a time and groups beyond its LDS stage (the direct stores); many buckets."""
    rng = np.random.default_rng(V + E)
    vid = _ids("sparse", V, rng)
    src, dst = mirrored(vid, E, rng)
    check(gg, gg_sorted, orc, vid, src, dst, 1)


def test_self_loops_duplicates_and_dangling_ids_derive(gg, gg_sorted, orc):
    """Rows whose ids are no vertex drop in pairs: the kept rows are still fully mirrored."""
    rng = np.random.default_rng(5)
    vid = _ids("sparse", 40_000, rng)
    src, dst = mirrored(vid, 2 * 3 * TILE + 2 * 99, rng, extras=True)
    check(gg, gg_sorted, orc, vid, src, dst, 1)


def test_star_derives(gg, gg_sorted, orc):
    """The hub is the source of every first-half row: its split is its degree, the leaves' split is 0, and the
    vertices that are no leaf have no edge at all."""
    rng = np.random.default_rng(9)
    vid = _ids("sparse", 3000, rng)
    hub, leaves = vid[17], np.delete(vid, 17)[:2500]
    d = leaves[rng.integers(0, leaves.size, 2 * TILE + 100)]
    s = np.full(d.size, hub, np.int64)
    check(gg, gg_sorted, orc, vid, np.concatenate([s, d]), np.concatenate([d, s]), 1)


@pytest.mark.parametrize("kind", ["dense", "sparse", "wide"])
def test_every_dictionary_mode_derives(gg, gg_sorted, orc, kind):
    rng = np.random.default_rng(len(kind))
    vid = _ids(kind, 40_000, rng)
    src, dst = mirrored(vid, 2 * 3 * TILE + 2 * 99, rng)
    check(gg, gg_sorted, orc, vid, src, dst, 1)


# ---- must not derive -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["last_pair", "one_per_tile", "offset_by_one", "permuted_half", "a_tenth", "shuffled"])
def test_tables_that_are_not_fully_mirrored_do_not_derive(gg, gg_sorted, orc, shape):
    rng = np.random.default_rng(len(shape))
    vid = _ids("sparse", 20_000, rng)
    src, dst = _shaped(vid, 2 * 5 * TILE + 2 * 777, shape, rng)
    check(gg, gg_sorted, orc, vid, src, dst, 0)


def test_odd_row_count_does_not_derive(gg, gg_sorted, orc):
    rng = np.random.default_rng(3)
    vid = _ids("sparse", 20_000, rng)
    src, dst = mirrored(vid, 2 * 5 * TILE + 2 * 777 + 1, rng)
    check(gg, gg_sorted, orc, vid, src, dst, 0)


@pytest.mark.parametrize("how", ["edge_rowid", "rank_mode_2", "legacy_build", "mirror_pairs_off"])
def test_builds_outside_the_vertex_sorted_form_do_not_derive(gg, gg_sorted, gg_unpaired, orc, how):
    """A fully mirrored table, built with edge rowids, with match-mask ranks, by the multi-pass build (whose reverse
    CSR is made on first use, sources ascending inside a row), and on a GG_MIRROR_PAIRS=0 context."""
    rng = np.random.default_rng(21)
    vid = _ids("sparse", 20_000, rng)
    src, dst = mirrored(vid, 2 * 5 * TILE + 2 * 777, rng)
    try:
        check(gg, gg_sorted, orc, vid, src, dst, 0, rowid=how == "edge_rowid", rank=2 if how == "rank_mode_2" else 1,
              legacy=how == "legacy_build", main=gg_unpaired if how == "mirror_pairs_off" else None)
    finally:
        gg_unpaired.debug_reset()
        gg_unpaired.staging_clear()


def test_shard_builds_do_not_derive(gg, gg_sorted, orc):
    """Shard 0 of 2 of a fully mirrored table: its reverse CSR (the rows whose destination it owns) against numpy,
    everything else against the same shard of the never-deriving context."""
    rng = np.random.default_rng(22)
    vid = _ids("sparse", 20_000, rng)
    src, dst = mirrored(vid, 2 * 5 * TILE + 2 * 777, rng)
    want_rev = reverse_reference(vid, src, dst, owned_part=(0, 2))
    got = []
    try:
        for ctx in (gg, gg_sorted):
            ctx.staging_clear()
            ctx.set_edge_rowid(False)
            ctx.rank_mode(1)
            ctx.append_vertices(vid)
            ctx.append_edges(src, dst)
            csr = ctx.build_csr_shard(0, 2)
            try:
                assert csr.reverse_derived == 0
                rev = csr.export_reverse()
                assert _same(rev, want_rev)
                got.append((csr.export(), ctx.expand_khop(csr, 1, 2)))
            finally:
                csr.close()
        assert _same(got[0][0], got[1][0]) and got[0][1] == got[1][1]
    finally:
        for ctx in (gg, gg_sorted):
            ctx.debug_reset()
            ctx.staging_clear()
