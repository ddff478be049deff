"""Edge tables whose second half mirrors the first (row i + E/2 = row i with source and destination swapped, an
undirected table loaded twice): the bucketed build densifies such pairs with one dictionary lookup (gg_csr_fast.hip,
k_densify_pairs).  Every export must equal the oracle's bit for bit, and the 2-hop counts and digests must equal
both the oracle's and those of a context created with GG_MIRROR_PAIRS=0 (no pairing), on fully, partly and not at
all mirrored tables."""
import os

import numpy as np
import pytest

import duckdb_pgq_amd as pkg
from duckdb_pgq_amd import datagen

pytestmark = pytest.mark.gpu

TILE = 8192  # rows per tile of the densification (FB_TILE)


@pytest.fixture(scope="module")
def gg_unpaired():
    """A second context, created with the pairing switched off."""
    old = os.environ.get("GG_MIRROR_PAIRS")
    os.environ["GG_MIRROR_PAIRS"] = "0"
    try:
        g = pkg.GG(0)
    finally:
        if old is None:
            del os.environ["GG_MIRROR_PAIRS"]
        else:
            os.environ["GG_MIRROR_PAIRS"] = old
    yield g
    g.close()


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


def _build(g, vid, src, dst, edge_only=False):
    g.staging_clear()
    if not edge_only:
        g.append_vertices(vid)
    g.append_edges(src, dst)
    if edge_only:
        g.vertices_from_edges()
    return g.build_csr()


def check(gg, gg_unpaired, orc, vid, src, dst, rowid=True, rank_modes=(1, 2), edge_only=False):
    if edge_only:
        vid = np.unique(np.concatenate([src, dst]))
    rc, g = orc.csr_build(vid, src, dst)
    assert rc == 0
    o_off, o_nbr, o_eid, o_vid = g.arrays()
    want = g.khop(1, 2)
    runs = [(gg, m) for m in rank_modes] + [(gg_unpaired, rank_modes[0])]
    try:
        for ctx, mode in runs:
            ctx.set_edge_rowid(rowid)
            ctx.rank_mode(mode)
            csr = _build(ctx, vid, src, dst, edge_only)
            off, nbr, eid, v2 = csr.export()
            tag = (ctx is gg, mode)
            assert csr.V == g.V and csr.E == g.E and csr.dropped == g.dropped, tag
            assert np.array_equal(v2, o_vid), tag
            assert np.array_equal(off, o_off), tag
            assert np.array_equal(nbr, o_nbr), tag
            assert np.array_equal(eid, o_eid) if rowid else np.all(eid == -1), tag
            assert ctx.expand_khop(csr, 1, 2) == want, tag
            csr.close()
    finally:
        for ctx in (gg, gg_unpaired):
            ctx.debug_reset()
            ctx.staging_clear()
        g.close()


@pytest.mark.parametrize("E", [2, 3, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, 2 * 4 * TILE, 2 * 4 * TILE + 1,
                               2 * 3 * TILE + 2 * 1234 + 1, 600_000])
@pytest.mark.parametrize("rowid", [False, True])
def test_fully_mirrored_tables(gg, gg_unpaired, orc, E, rowid):
    """h = E // 2 a multiple of the tile and not, odd E (row 2h unpaired, alone in a tile when h is a multiple)."""
    rng = np.random.default_rng(E)
    vid = _ids("sparse", 3000 if E < 100_000 else 70_000, rng)
    src, dst = mirrored(vid, E, rng)
    check(gg, gg_unpaired, orc, vid, src, dst, rowid)


def _break(vid, src, dst, rows, rng):
    src, dst = src.copy(), dst.copy()
    dst[rows] = vid[rng.integers(0, vid.size, len(rows))]
    return src, dst


def _shaped(vid, E, shape, rng):
    src, dst = mirrored(vid, E, rng)
    h = E // 2
    if shape == "one_per_tile":
        rows = h + np.arange(0, h, TILE) + rng.integers(0, 512, (h + TILE - 1) // TILE)
        src, dst = _break(vid, src, dst, np.minimum(rows, 2 * h - 1), rng)
    elif shape == "every_other":
        src, dst = _break(vid, src, dst, h + np.arange(0, h, 2), rng)
    elif shape == "last_pair":
        src, dst = _break(vid, src, dst, [2 * h - 1], rng)
    elif shape == "offset_by_one":  # the second half one row late: row i + h + 1 mirrors row i
        src = np.concatenate([src[:h], vid[:1], src[h:E - 1]])
        dst = np.concatenate([dst[:h], vid[1:2], dst[h:E - 1]])
    elif shape == "a_tenth":  # too few pairs for the paired walk to pay: the build walks the tiles one by one
        src, dst = _break(vid, src, dst, h + np.flatnonzero(rng.random(h) < 0.9), rng)
    elif shape == "shuffled":  # no pair at all
        p = rng.permutation(src.size)
        src, dst = src[p], dst[p]
    else:
        assert shape == "full", shape
    assert src.size == E and dst.size == E
    return src, dst


@pytest.mark.parametrize("shape", ["one_per_tile", "every_other", "last_pair", "offset_by_one", "a_tenth", "shuffled"])
@pytest.mark.parametrize("E", [2 * 5 * TILE + 2 * 777, 2 * 5 * TILE + 2 * 777 + 1])
def test_partly_mirrored_tables(gg, gg_unpaired, orc, shape, E):
    rng = np.random.default_rng(E + len(shape))
    vid = _ids("sparse", 20_000, rng)
    src, dst = _shaped(vid, E, shape, rng)
    check(gg, gg_unpaired, orc, vid, src, dst)


@pytest.mark.parametrize("kind", ["sparse", "dense", "wide"])
@pytest.mark.parametrize("rowid", [False, True])
def test_mirrored_pairs_with_dangling_ids_self_loops_and_duplicates(gg, gg_unpaired, orc, kind, rowid):
    """Every dictionary mode; a pair whose ids are no vertex drops both of its rows."""
    rng = np.random.default_rng(len(kind) * 7 + rowid)
    vid = _ids(kind, 40_000, rng)
    src, dst = mirrored(vid, 2 * 3 * TILE + 2 * 99 + 1, rng, extras=True)
    check(gg, gg_unpaired, orc, vid, src, dst, rowid)


@pytest.mark.parametrize("E,shape", [(3, "full"), (2 * TILE + 1, "full"), (2 * 3 * TILE + 2 * 1234, "full"),
                                     (600_000, "full"), (600_001, "every_other"), (600_000, "a_tenth"),
                                     (600_000, "shuffled")])
def test_mirrored_tables_on_the_edge_only_path(gg, gg_unpaired, orc, E, shape):
    """Vertex table := distinct endpoints (gg_vertices_from_edges: its set insert pairs rows too), then the build."""
    rng = np.random.default_rng(E + 5)
    vid = _ids("sparse", 50_000, rng)
    src, dst = _shaped(vid, E, shape, rng)
    check(gg, gg_unpaired, orc, vid, src, dst, rank_modes=(1,), edge_only=True)
    gg.staging_clear()
    gg.append_edges(src, dst)
    assert gg.vertices_from_edges() == np.unique(np.concatenate([src, dst])).size
    gg.staging_clear()


def test_ldbc_shaped_table_is_mirrored():
    """datagen.ldbc_knows builds the benchmark's table the way the reference loads it: knows twice, the second time with
    the id columns swapped, so the pairing applies to the benchmark's build."""
    _, src, dst = datagen.ldbc_knows(2000, 50_000, 7)
    h = src.size // 2
    assert np.array_equal(src[h:2 * h], dst[:h]) and np.array_equal(dst[h:2 * h], src[:h])
