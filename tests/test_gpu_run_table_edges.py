"""The run table of k_expand_mid2 and the fold it shares with k_expand_front and k_expand_mid3 (gg_khop.hip:
mid_stage_offsets, mid_stage, mid_fold_tile) at the sizes where the fold takes another path.  The comb puts one hub per
case between dedicated leaves, so that every in-run length around the i-split threshold (128) and the tile (768) meets
out-degrees around a lane row (64), a J-block (512) and several of them; its mirrored form derives its reverse CSR
(roff == off), its one-directional form has separate reverse rows.  Written for the changes to that staging and fold
of DESIGN.md 4.2 "Round 26" (profiles/r26_expand_mid2_ab.json): the variants that were measured and not kept and the
state loop as it is now all passed here, and any later change to either has to.  Everything is integer: every
comparison is exact, against the C oracle."""
import numpy as np
import pytest

from tests import offset_runs as R
from tests.test_gpu_deep_walks import launches

pytestmark = pytest.mark.gpu

OUT_DEGREES = (0, 1, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 2049)
IN_RUNS = (1, 127, 128, 129, 767, 768, 769)


# ---- the tables ------------------------------------------------------------------------------------------------------
def _directed_cases():
    """(in-run length, out-degree) per hub: every value of both lists, the thresholds of one against those of the other,
    about 2.9 M walks in all."""
    cases = [(1, d) for d in OUT_DEGREES]
    cases += [(n, d) for n in (127, 128, 129) for d in (0, 1, 63, 64, 65, 511, 512, 513, 1025)]
    cases += [(n, d) for n in (767, 768, 769) for d in (1, 65, 513)]
    cases += [(128, 2049), (129, 1023), (127, 1024)]
    assert {n for n, _ in cases} == set(IN_RUNS) and {d for _, d in cases} == set(OUT_DEGREES)
    assert sum(n * d for n, d in cases) < 5_000_000
    return cases


MIRRORED_DEGREES = (1, 63, 64, 65, 127, 128, 129, 511, 512, 513, 767, 768, 769, 1025)  # in-run == out-degree: 3.7 M walks


def comb(mirror):
    """vid, src, dst.  One-directional: hub i has IN dedicated vertices with a row into it and OUT dedicated vertices it has
    a row to.  Mirrored: hub i has DEG dedicated neighbours, the table is those rows and then the same rows swapped."""
    src, dst, nxt = [], [], 0

    def fresh(n):
        nonlocal nxt
        out = np.arange(nxt, nxt + n, dtype=np.int64)
        nxt += n
        return out

    if mirror:
        for deg in MIRRORED_DEGREES:
            hub, leaves = fresh(1), fresh(deg)
            src.append(np.repeat(hub, deg)), dst.append(leaves)
    else:
        for n_in, n_out in _directed_cases():
            ins, hub, outs = fresh(n_in), fresh(1), fresh(n_out)  # (the in-leaves before the hub, the out-leaves behind it)
            src += [ins, np.repeat(hub, n_out)]
            dst += [np.repeat(hub, n_in), outs]
    s, d = np.concatenate(src), np.concatenate(dst)
    vid = np.arange(nxt, dtype=np.int64) * 3 + 5  # ascending: the dense index of a vertex is its position
    s, d = vid[s], vid[d]
    if mirror:
        return vid, np.concatenate([s, d]), np.concatenate([d, s])
    return vid, s, d


_OFFSET_RUNS = R.tables()
TABLES = {"comb_mirrored": lambda: comb(True), "comb_plain": lambda: comb(False),
          "mirrored_4618": lambda: _OFFSET_RUNS["mirrored_4618"], "gaps_plain": lambda: _OFFSET_RUNS["gaps_plain"]}


@pytest.fixture(scope="module")
def refs(orc):
    """name -> the table and the oracle's figures: computed once, shared, never changed."""
    out = {}
    for name, make in TABLES.items():
        vid, src, dst = make()
        rc, g = orc.csr_build(vid, src, dst)
        assert rc == 0
        try:
            sources = vid[::7]
            dense = g.lookup(sources).astype(np.uint32)
            out[name] = {"vid": vid, "src": src, "dst": dst, "V": g.V, "E": g.E, "sources": sources,
                         "khop12": g.khop(1, 2), "khop13": g.khop(1, 3), "khop13_sources": g.khop(1, 3, sources_dense=dense),
                         "khop12_sources": g.khop(1, 2, sources_dense=dense)}
        finally:
            g.close()
    return out


def _build(ctx, r, shard=None):
    ctx.staging_clear()
    ctx.set_edge_rowid(False)
    ctx.rank_mode(1)  # (the vertex-sorted build: a fully mirrored table derives its reverse CSR)
    ctx.append_vertices(r["vid"])
    ctx.append_edges(r["src"], r["dst"])
    return ctx.build_csr() if shard is None else ctx.build_csr_shard(*shard)


def _figures(st):
    return st["rows"][1], st["rows"][2], st["digest"][1], st["digest"][2]


# ---- the run table's edges ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["comb_mirrored", "comb_plain"])
def test_comb(gg, refs, name):
    r = refs[name]
    walks = (sum(d * d for d in MIRRORED_DEGREES) + sum(MIRRORED_DEGREES) if name == "comb_mirrored"
             else sum(n * d for n, d in _directed_cases()))
    assert r["khop12"]["rows"][2] == walks < 5_000_000
    c = _build(gg, r)
    try:
        assert (c.V, c.E) == (r["V"], r["E"])
        assert c.reverse_derived == (name == "comb_mirrored")
        st, counts = launches(gg, lambda: gg.expand_khop(c, 1, 2))
        assert counts.get("expand_mid2") == 1 and counts.get("mid_tile_rows") == 1
        assert st == r["khop12"]
        assert gg.expand_khop(c, 2, 2)["digest"][2] == r["khop12"]["digest"][2]
        cut = r["V"] // 3
        mids = [gg.expand_khop_mid(c, 0, cut), gg.expand_khop_mid(c, cut, r["V"])]
        for h in (1, 2):
            assert sum(m["rows"][h] for m in mids) == r["khop12"]["rows"][h]
            assert sum(m["digest"][h] for m in mids) & R.M32 == r["khop12"]["digest"][h]
    finally:
        c.close()


# ---- the kernels that share the fold -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(TABLES))
def test_shared_fold_forms(gg, refs, name):
    """k_max = 3 from every vertex (k_expand_mid3) and a source list under the forced frontier forms 1, 2 and 3
    (k_expand_fused2, k_expand_front, k_expand_mid3 over the sorted frontier)."""
    r = refs[name]
    c = _build(gg, r)
    try:
        assert gg.expand_khop(c, 1, 3) == r["khop13"]
        for knob in (1, 2, 3):
            gg.force_frontier(knob)
            assert gg.expand_khop(c, 1, 3, sources=r["sources"]) == r["khop13_sources"], knob
            assert gg.expand_khop(c, 1, 2, sources=r["sources"]) == r["khop12_sources"], knob
        gg.force_frontier(0)
        assert gg.expand_khop(c, 1, 2) == r["khop12"]  # (and the product kernel behind them)
    finally:
        gg.force_frontier(0)
        c.close()


# ---- shards: foreign rows, entries that are indices of the whole vertex table -----------------------------------------
def test_shards(gg, refs):
    r = refs["comb_plain"]
    total = [0, 0, 0, 0]
    for part in (0, 1):
        c = _build(gg, r, shard=(part, 2))
        try:
            got = _figures(gg.expand_khop(c, 1, 2))
            off, nbr = c.export()[:2]
            roff, rnbr, _ = c.export_reverse()
            assert int(rnbr.max()) < c.V == r["V"]
            assert got == R.khop12(off, nbr, roff, rnbr, c.V), part
            total = [a + b for a, b in zip(total, got)]
        finally:
            c.close()
    want = _figures(r["khop12"])
    assert tuple(total[:2]) == want[:2] and (total[2] & R.M32, total[3] & R.M32) == want[2:]


# ---- the same CSR again and again ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["comb_mirrored", "gaps_plain"])
def test_repeats_are_identical(gg, refs, name):
    r = refs[name]
    c = _build(gg, r)
    try:
        runs = [gg.expand_khop(c, 1, 2) for _ in range(3)]
        assert runs[0] == runs[1] == runs[2] == r["khop12"]
    finally:
        c.close()
