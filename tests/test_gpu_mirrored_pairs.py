"""A mirrored pair is stored once (gg_csr_fast.hip, FB_PARTNER): where row i + h of the edge table is row i swapped, the
paired densification marks row i's dense pair instead of storing the partner's, the derived partition reads first-half
tiles only, and the plain partition makes a second-half row's pair from its partner's marked pair or loads the row's
own.  Every table here is a seeded first half of h rows plus its swapped copy, then changed per case; every build is
compared bit for bit (off, nbr, roff, rnbr, rrow, vertex ids) with a numpy stable counting sort of the kept rows, with
a GG_MIRROR_PAIRS=0 context and with a GG_MIRROR_REVERSE=0 context, its 1..2-hop rows and digests with the C oracle's,
and each case states which form must have run (reverse_derived and the profile's kernel names; where both forms of a
kernel are launched, the one that returns at once must be the quicker of the two)."""
import numpy as np
import pytest

import duckdb_pgq_amd as pkg
from tests.test_gpu_derived_reverse import _ctx_with_env

pytestmark = pytest.mark.gpu

TILE = 8192       # rows per tile of the densification and the partition (FB_TILE)
H0 = TILE + 37    # two first-half tiles, the last one partial


@pytest.fixture(scope="module")
def gg_sorted():
    g = _ctx_with_env("GG_MIRROR_REVERSE")
    yield g
    g.close()


@pytest.fixture(scope="module")
def gg_unpaired():
    g = _ctx_with_env("GG_MIRROR_PAIRS")
    yield g
    g.close()


# ---- tables ----------------------------------------------------------------------------------------------------------
def _vid(V):
    return pkg.datagen.person_ids(V, 11)


def _bad(vid):
    return np.int64(int(vid.max()) + 1)


def _half(vid, h, seed):
    rng = np.random.default_rng(seed)
    return vid[rng.integers(0, vid.size, h)].astype(np.int64), vid[rng.integers(0, vid.size, h)].astype(np.int64)


def _table(s, d):
    return np.concatenate([s, d]), np.concatenate([d, s])


def _other(vid, src, dst, row, seed):
    """Row `row` becomes another valid row, certainly not what it was."""
    rng = np.random.default_rng(seed)
    pos = int(np.flatnonzero(vid == dst[row])[0]) if dst[row] in vid else 0
    src[row] = vid[int(rng.integers(0, vid.size))]
    dst[row] = vid[(pos + 1 + int(rng.integers(0, vid.size - 1))) % vid.size]


def make(case, V=3000):
    """(vid, src, dst, derived, paired): what the default context must report for the table."""
    vid = _vid(V)
    bad = _bad(vid)
    if case.startswith("full_h"):
        h = {"full_h_partial": H0, "full_h_2tiles": 2 * TILE, "full_h_100": 100, "full_h_1": 1}[case]
        return (vid, *_table(*_half(vid, h, h)), 1, True)
    s, d = _half(vid, H0, 7)
    h = H0
    if case == "odd":
        src, dst = _table(s, d)
        return vid, np.append(src, vid[5]), np.append(dst, vid[1234]), 0, True
    if case in ("replace_row_h", "replace_last", "replace_middle", "replace_quarter"):
        src, dst = _table(s, d)
        rows = {"replace_row_h": [h], "replace_last": [2 * h - 1], "replace_middle": [h + TILE // 2 + 11],
                "replace_quarter": (h + np.flatnonzero(np.random.default_rng(3).random(h) < 0.25)).tolist()}[case]
        for r in rows:
            _other(vid, src, dst, r, r)
        return vid, src, dst, 0, True
    if case == "bad_source_mirrored":  # both rows of the pair drop: the kept rows are still fully mirrored
        s[4000] = bad
        return (vid, *_table(s, d), 1, True)
    if case == "bad_source_mirrored_first_and_last":
        s[0] = bad
        d[h - 1] = bad
        return (vid, *_table(s, d), 1, True)
    if case == "bad_destination_partner_replaced":  # only the partner stays
        d[4000] = bad
        src, dst = _table(s, d)
        _other(vid, src, dst, h + 4000, 1)
        return vid, src, dst, 0, True
    if case == "partner_replaced_by_bad":  # only the first-half row stays
        src, dst = _table(s, d)
        src[h + 4000] = bad
        return vid, src, dst, 0, True
    if case == "bad_first_and_last_partner_replaced":
        d[0] = bad  # the very first row: bad destination, partner replaced by a valid row
        src, dst = _table(s, d)
        _other(vid, src, dst, h, 2)
        dst[2 * h - 1] = bad  # the very last row of the first half: valid, its partner replaced by a row with a bad id
        return vid, src, dst, 0, True
    if case == "self_loops_and_duplicates":
        s[:8] = d[:8]
        s[8:24], d[8:24] = s[24:40], d[24:40]
        s[h - 1] = d[h - 1]
        return (vid, *_table(s, d), 1, True)
    if case in ("sorted_full", "sorted_replaced"):
        o = np.argsort(s, kind="stable")
        src, dst = _table(s[o], d[o])
        if case == "sorted_replaced":
            _other(vid, src, dst, h + 5000, 4)
        return vid, src, dst, int(case == "sorted_full"), True
    raise AssertionError(case)


# ---- reference -------------------------------------------------------------------------------------------------------
def counting_sort_reference(o_vid, src, dst):
    """off, nbr, roff, rnbr, rrow of the kept rows: dense indices are positions in o_vid, both sorts stable."""
    order = np.argsort(o_vid, kind="stable")
    sv = o_vid[order]

    def dense(ids):
        p = np.minimum(np.searchsorted(sv, ids), sv.size - 1)
        return np.where(sv[p] == ids, order[p], -1).astype(np.int64)

    u, v = dense(src), dense(dst)
    keep = (u >= 0) & (v >= 0)
    u, v = u[keep], v[keep]
    fo, ro = np.argsort(u, kind="stable"), np.argsort(v, kind="stable")
    off = np.concatenate([[0], np.cumsum(np.bincount(u, minlength=o_vid.size))]).astype(np.int64)
    roff = np.concatenate([[0], np.cumsum(np.bincount(v, minlength=o_vid.size))]).astype(np.int64)
    return off, v[fo], roff, u[ro], v[ro]


def build(ctx, vid, src, dst, rank=0, rowid=False):
    """One profiled build: (arrays, reverse_derived, profile, 1..2-hop statistics)."""
    ctx.staging_clear()
    ctx.set_edge_rowid(rowid)  # (with edge rowids the build is not the vertex-sorted form)
    if rank:
        ctx.rank_mode(rank)
    ctx.append_vertices(vid)
    ctx.append_edges(src, dst)
    ctx.profile_reset()
    ctx.profile_select(None)
    ctx.profile(True)
    try:
        csr = ctx.build_csr()
    finally:
        ctx.profile(False)
    try:
        prof = ctx.profile_get()
        off, nbr, _, v2 = csr.export()
        roff, rnbr, rrow = csr.export_reverse()
        return (off, nbr, roff, rnbr, rrow, v2), int(csr.reverse_derived), prof, ctx.expand_khop(csr, 1, 2)
    finally:
        csr.close()
        ctx.debug_reset()
        ctx.staging_clear()


NAMES = ("off", "nbr", "roff", "rnbr", "rrow", "vertex ids")


def check(gg, gg_unpaired, gg_sorted, orc, case, V=3000, rank=0, rowid=False):
    vid, src, dst, derived, _ = make(case, V)
    if rank == 2 or rowid:
        derived = 0  # match-mask ranks, edge rowids: the sub-bucket form, which never derives
    h = src.size // 2
    rc, g = orc.csr_build(vid, src, dst)
    assert rc == 0
    try:
        o_off, o_nbr, _, o_vid = g.arrays()
        want_khop = g.khop(1, 2)
    finally:
        g.close()
    want = (*counting_sort_reference(o_vid, src, dst), o_vid)
    assert np.array_equal(want[0], o_off) and np.array_equal(want[1], o_nbr)  # (the reference agrees with the oracle)

    got, rd, prof, khop = build(gg, vid, src, dst, rank, rowid)
    for name, a, b in zip(NAMES, got, want):
        assert np.array_equal(a, b), ("default", name)
    assert khop == want_khop
    # which form ran
    us = {k: round(v[1] * 1e3 / max(v[0], 1), 1) for k, v in prof.items() if k.startswith(("densify", "partition"))}
    print(case, V, rank, "reverse_derived", rd, us)
    assert rd == derived
    assert prof["densify_pairs"][0] == 1 and prof["densify_unpaired"][0] == 1  # the paired form was launched ...
    even_vsort = src.size % 2 == 0 and rank != 2 and not rowid
    assert ("partition_dual_plain" in prof) == even_vsort and prof["partition_dual"][0] == 1
    if not derived and h >= TILE:  # ... and did the work (a derived build says so itself: only the paired form can raise it)
        assert prof["densify_pairs"][1] > prof["densify_unpaired"][1], us
        if even_vsort:
            assert prof["partition_dual_plain"][1] > prof["partition_dual"][1], us

    # the same table without the pairing, and paired without the derivation
    for tag, ctx in (("GG_MIRROR_PAIRS=0", gg_unpaired), ("GG_MIRROR_REVERSE=0", gg_sorted)):
        got2, rd2, prof2, khop2 = build(ctx, vid, src, dst)
        assert rd2 == 0, tag
        for name, a, b in zip(NAMES, got2, got):
            assert np.array_equal(a, b), (tag, name)
        assert khop2 == want_khop, tag
        assert ("densify_unpaired" in prof2) == (ctx is gg_sorted), tag
        assert "partition_dual_plain" not in prof2 and prof2["partition_dual"][0] == 1, tag


FULL = ["full_h_partial", "full_h_2tiles", "full_h_100", "full_h_1"]
PAIRED_NOT_DERIVED = ["odd", "replace_row_h", "replace_last", "replace_middle", "replace_quarter"]
BAD_IDS = ["bad_source_mirrored", "bad_source_mirrored_first_and_last", "bad_destination_partner_replaced",
           "partner_replaced_by_bad", "bad_first_and_last_partner_replaced"]
OTHERS = ["self_loops_and_duplicates", "sorted_full", "sorted_replaced"]


@pytest.mark.parametrize("case", FULL + PAIRED_NOT_DERIVED + BAD_IDS + OTHERS)
def test_tables(gg, gg_unpaired, gg_sorted, orc, case):
    check(gg, gg_unpaired, gg_sorted, orc, case)


@pytest.mark.parametrize("case", ["full_h_partial", "replace_middle"])
def test_many_buckets(gg, gg_unpaired, gg_sorted, orc, case):
    """V = 70 000: more than 6 bucket bits, more buckets than a wave has lanes."""
    check(gg, gg_unpaired, gg_sorted, orc, case, V=70_000)


@pytest.mark.parametrize("case", ["full_h_partial", "replace_middle"])
def test_match_mask_ranks(gg, gg_unpaired, gg_sorted, orc, case):
    """gg_debug_rank_mode(ctx, 2): the paired densification followed by the sub-bucket form's partition."""
    check(gg, gg_unpaired, gg_sorted, orc, case, rank=2)


@pytest.mark.parametrize("case", ["full_h_partial", "replace_middle"])
def test_edge_rowids(gg, gg_unpaired, gg_sorted, orc, case):
    """Edge rowids kept: the paired densification followed by the partition that carries edge positions."""
    check(gg, gg_unpaired, gg_sorted, orc, case, rowid=True)
