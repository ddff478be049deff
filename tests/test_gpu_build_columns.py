"""The bucketed CSR build where its small kernels decide a position (gg_csr_fast.hip).

Column kernels: a tile is 8192 rows, a group 16 tiles, a supergroup 16 groups (256 tiles).  k_col_apply starts a
column of a group from the bucket start + the sums of the supergroups before its own + the partial sums of the earlier
groups of its own supergroup, so the tables below have 1, 16, 17, 256, 257 and 513 tiles: one group, a full group, a
second group of one tile, a full supergroup, a second supergroup of one tile, and a third supergroup behind two full
ones.  The build halves a whole table of E >= 2 rows at h = E // 2 (first-half and second-half tiles), so it uses
ceil(h / 8192) + ceil((E - h) / 8192) tiles: an even number for every even E, and 2 k + 1 for E = 2 * 8192 k + 1.
The odd totals are therefore met by tables of an odd number of rows and by shards (not halved); the forms that need an
even table (fully mirrored, mirrored with one pair broken) take the next even total, 18 and 258 -- still a last
group of two tiles behind a full group, or behind a full supergroup.  tiles_of() restates the count and every case
asserts that its table has the total it names.  With 513 tiles (4.2 M rows, the largest a quick test affords) a group
has at most two supergroups before it: the batch of 16 supergroup rows that k_col_apply takes from the 257th group
on (4 097 tiles, 33 M rows) is reached by no case here, only by bench.py at SF100 (304 groups) and its parity fields.

Rows step of the vertex-sorted form: a wave of k_vrows takes where its group of 16 vertices starts from the offset
words it loads (bucket start + the chunks' entries before the group); no kernel computes group starts, and the launch
"sub_totals" is the sub-bucket form's alone.

Every comparison is exact: offsets, neighbours, rowids and vertex ids against oracle_lib's csr_build of the same
tables, the reverse CSR against csr_build of the same rows with source and destination exchanged (rows in rowid order
inside a vertex: the stable order of either build)."""
import numpy as np
import pytest

from duckdb_pgq_amd import datagen, sharding
from tests.test_gpu_build_forms import launched
from tests.test_gpu_derived_reverse import TILE, _break, mirrored

pytestmark = pytest.mark.gpu

GROUP = 16   # tiles per group of the column kernels
SUPER = 16   # groups per supergroup
VG = 16      # vertices per wave of k_vrows (GG_FB_VG)
VCAP = 1536  # entries of a wave's stage in k_vrows (GG_FB_VCAP)
FORMS = ["directed", "mirrored", "one_broken", "shard", "rowid"]


def tiles_of(E, halved=True):
    h = E // 2 if halved and E >= 2 else 0
    return (h + TILE - 1) // TILE + (E - h + TILE - 1) // TILE


def rows_for(form, tiles):
    """(E, the tile total the build uses) of `form` at `tiles`"""
    if form == "shard":  # not halved: a partial last tile
        E = tiles * TILE - 5
        return E, tiles_of(E, halved=False)
    if form in ("mirrored", "one_broken"):  # an even table: the next even total, partial last tiles in both halves
        tiles += tiles % 2
        E = tiles * TILE - 2 * 7
    elif tiles % 2:  # h full tiles, then h + 1 rows
        E = (tiles - 1) * TILE + 1
    else:
        E = tiles * TILE
    return E, tiles_of(E)


def _vid(V):
    return datagen.person_ids(V, 11)


def _with_dangling(vid, src, dst):
    """a few rows whose ids are no vertex, where the table has rows to spare"""
    if src.size >= 64:
        bad = np.int64(int(vid.max()) + 1)
        src[3], dst[5], src[7], dst[7] = bad, bad, bad, bad
    return src, dst


def table(orc, form, tiles, V):
    """(vid, src, dst, part, reference) of one case; reference = (off, nbr, eid, roff, rnbr)"""
    E, total = rows_for(form, tiles)
    assert total == tiles + (tiles % 2 if form in ("mirrored", "one_broken") else 0), (form, tiles, E, total)
    rng = np.random.default_rng(E + V)
    vid = _vid(V)
    if form in ("mirrored", "one_broken"):
        src, dst = mirrored(vid, E, rng, extras=True)
        if form == "one_broken":
            src, dst = _break(vid, src, dst, [E - 1 - E // 4], rng)
    else:
        src, dst = _with_dangling(vid, vid[rng.integers(0, V, E)], vid[rng.integers(0, V, E)])
    part = (1, 2) if form == "shard" else None
    return vid, src, dst, part, reference(orc, vid, src, dst, part)


def reference(orc, vid, src, dst, part=None):
    """The oracle's CSR of the table and of the table with its columns exchanged.  A shard keeps a row in its forward
    CSR where it owns the source and in its reverse CSR where it owns the destination."""
    fwd = np.ones(src.size, bool) if part is None else sharding.owner_of(src, part[1]) == part[0]
    rev = np.ones(src.size, bool) if part is None else sharding.owner_of(dst, part[1]) == part[0]
    out = []
    for a, b in ((src[fwd], dst[fwd]), (dst[rev], src[rev])):
        rc, g = orc.csr_build(vid, a, b)
        assert rc == 0
        try:
            off, nbr, eid, o_vid = g.arrays()
            assert np.array_equal(o_vid, vid)
            out += [off.copy(), nbr.copy(), eid.copy()]
        finally:
            g.close()
    return out[0], out[1], out[2], out[3], out[4]


def build_and_compare(gg, vid, src, dst, want, part=None, rowid=False, derived=None):
    """Build (vertex-sorted unless rowids are kept), compare everything with the reference; the launched names."""
    off, nbr, eid, roff, rnbr = want
    gg.debug_reset()
    gg.set_edge_rowid(rowid)
    gg.rank_mode(1)
    gg.staging_clear()
    gg.append_vertices(vid)
    gg.append_edges(src, dst)
    csr, names = launched(gg, (lambda: gg.build_csr_shard(*part)) if part else gg.build_csr)
    try:
        assert "partition_dual" in names and ("leaf_rows" in names or "leaf_rows_plain" in names), names
        if derived is not None:
            assert csr.reverse_derived == derived
        g_off, g_nbr, g_eid, g_vid = csr.export()
        assert np.array_equal(g_vid, vid)
        assert np.array_equal(g_off, off), "off"
        assert np.array_equal(g_nbr, nbr), "nbr"
        assert np.array_equal(g_eid, eid) if rowid else bool(np.all(g_eid == -1)), "eid"
        g_roff, g_rnbr, g_rrow = csr.export_reverse()
        assert np.array_equal(g_roff, roff), "roff"
        assert np.array_equal(g_rnbr, rnbr), "rnbr"
        assert np.array_equal(g_rrow, np.repeat(np.arange(vid.size, dtype=np.int64), np.diff(roff))), "rrow"
    finally:
        csr.close()
    return names


# ---- prefix boundaries -------------------------------------------------------------------------------------------------
def _boundary_cases():
    out = []
    for V in (1500, 70_000):  # 2 buckets; 128 buckets (256 columns)
        for form in FORMS:
            for tiles in ((1, 16, 17, 256, 257, 513) if form == "directed" else (17, 257)):
                out.append(pytest.param(form, tiles, V, id=f"{form}-{rows_for(form, tiles)[1]}-{V}"))  # (the total built)
    return out


@pytest.mark.parametrize("form,tiles,V", _boundary_cases())
def test_tile_totals_at_group_and_supergroup_boundaries(gg, orc, form, tiles, V):
    """directed: random rows, an odd number of them for the odd totals (unpaired densification, nothing derived);
    mirrored: every row i + E/2 mirrors row i (paired densification, derived reverse, the two column sets are the two
    halves' forward counts); one_broken: the same with one pair broken (paired densification, plain rows); shard: shard
    1 of 2; rowid: edge rowids kept, so the sub-bucket form, which still launches sub_totals."""
    vid, src, dst, part, want = table(orc, form, tiles, V)
    derived = {"mirrored": 1, "one_broken": 0, "directed": 0, "shard": 0}.get(form)
    names = build_and_compare(gg, vid, src, dst, want, part=part, rowid=form == "rowid", derived=derived)
    assert {"col_partial", "col_scan", "col_apply", "sub_sort"} <= names, names
    assert ("sub_totals" in names) == (form == "rowid"), names


# ---- group starts ------------------------------------------------------------------------------------------------------
def _positions(shape, rng):
    """(V, allowed: the positions that may have an edge, hub or None)"""
    if shape == "second_bucket_of_one":
        V = 1025
        return V, np.arange(V), None
    if shape == "ends_one_into_a_group":
        V = VG * 70 + 1
        return V, np.arange(V), None
    if shape == "ends_one_short_of_a_group":
        V = VG * 70 + 15
        return V, np.arange(V), None
    if shape == "empty_bucket":  # bucket 1 of 4 has no entry in either direction: no chunks
        V = 3 * 1024 + 100
        p = np.arange(V)
        return V, p[(p < 1024) | (p >= 2048)], None
    if shape == "above_the_stage":  # one vertex with more entries than a wave stages; its group stores directly
        return 3000, np.arange(3000), 1029
    if shape == "isolated_group_ends":  # the first and the last vertex of every group have no edge
        V = 3000
        p = np.arange(V)
        return V, p[(p % VG != 0) & (p % VG != VG - 1)], None
    raise AssertionError(shape)


GROUP_SHAPES = ["second_bucket_of_one", "ends_one_into_a_group", "ends_one_short_of_a_group", "empty_bucket",
                "above_the_stage", "isolated_group_ends"]


@pytest.mark.parametrize("mirror", [False, True], ids=["plain", "mirrored"])
@pytest.mark.parametrize("shape", GROUP_SHAPES)
def test_group_starts_from_the_offset_rows(gg, orc, shape, mirror):
    """Three chunks a bucket and direction at least (so a group's start is a sum over several offset rows), plain (an
    odd number of random rows) and mirrored (derived reverse: the sum runs over both half-buckets)."""
    rng = np.random.default_rng(sum(map(ord, shape)) + mirror)
    V, allowed, hub = _positions(shape, rng)
    vid = _vid(V)
    half = 12 * TILE + 321
    s, d = allowed[rng.integers(0, allowed.size, half)], allowed[rng.integers(0, allowed.size, half)]
    if hub is not None:
        s[: VCAP + 500] = hub
        assert np.count_nonzero(s == hub) > VCAP
    if shape == "second_bucket_of_one":  # the lone vertex of bucket 1 has entries in both directions
        s[-40:-20], d[-20:] = 1024, 1024
    if mirror:
        src, dst = np.concatenate([s, d]), np.concatenate([d, s])
    else:
        src, dst = np.concatenate([s, d, s[:1]]), np.concatenate([d, s[::-1], d[1:2]])
        assert src.size % 2 == 1
    src, dst = vid[src], vid[dst]
    want = reference(orc, vid, src, dst)
    off, roff = want[0], want[3]
    if shape == "empty_bucket":
        assert off[1024] == off[2048] and roff[1024] == roff[2048]
    if shape == "isolated_group_ends":
        deg = np.diff(off) + np.diff(roff)
        assert not deg[::VG].any() and not deg[VG - 1::VG].any() and deg.any()
    if hub is not None:
        assert off[hub + 1] - off[hub] > VCAP
    names = build_and_compare(gg, vid, src, dst, want, derived=1 if mirror else 0)
    assert "sub_totals" not in names, names


# ---- launches ----------------------------------------------------------------------------------------------------------
def test_the_vertex_sorted_build_launches_no_group_sums(gg, orc):
    vid, src, dst = datagen.ldbc_knows(2000, 50_000, 7)
    names = build_and_compare(gg, vid, src, dst, reference(orc, vid, src, dst))
    assert "sub_totals" not in names, names
    assert {"col_partial", "col_scan", "col_apply", "sub_sort", "leaf_rows"} <= names, names
