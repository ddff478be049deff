"""k_expand_mid2 stages its tiles from the reverse offsets and reads no row index (gg_khop.hip: mid_stage_offsets); a
derived build therefore writes none, and the first call that reads the COO column has it expanded from the offsets
(gg_csr.hip: ensure_reverse_index).  The tables are the smallest at which each part of the indexing can go wrong
(tests/offset_runs.py, whose numpy model of the staging tests/test_offset_runs_cpu.py pins to the oracle): edge counts
around one, two and three tiles of 768 entries, a hub row that holds whole tiles, and stretches of isolated vertices
longer than two window chunks.  Everything is integer: every comparison is exact."""
import numpy as np
import pytest

from duckdb_pgq_amd.gg import GG_CHUNK_ROWS
from tests import offset_runs as R
from tests.test_gpu_build_forms import FORMS, KINDS, _build as build_knobs, build_table, cases, tables  # noqa: F401
from tests.test_gpu_deep_walks import launched
from tests.test_gpu_derived_reverse import _ctx_with_env, reverse_reference

pytestmark = pytest.mark.gpu

TABLES = R.tables()
DERIVES = sorted(n for n in TABLES if n == "star" or n == "gaps_mirrored" or
                 (n.startswith("mirrored_") and int(n.split("_")[1]) % 2 == 0))


@pytest.fixture(scope="module")
def _gg_sorted_module():
    """A second context that never derives: GG_MIRROR_REVERSE=0 at its creation."""
    g = _ctx_with_env("GG_MIRROR_REVERSE")
    yield g
    g.close()


@pytest.fixture
def gg_sorted(_gg_sorted_module):
    g = _gg_sorted_module
    g.debug_reset()
    yield g
    g.debug_reset()
    g.profile(False)
    g.staging_clear()


@pytest.fixture(scope="module")
def refs(orc):
    """name -> the table, the oracle's CSR and khop(1, 2), the reverse CSR by numpy: computed once, shared, never changed."""
    out = {}
    for name, (vid, src, dst) in TABLES.items():
        rc, g = orc.csr_build(vid, src, dst)
        assert rc == 0
        try:
            off, nbr, _, o_vid = g.arrays()
            roff, rnbr, rrow = reverse_reference(o_vid, src, dst)
            out[name] = {"vid": vid, "src": src, "dst": dst, "V": g.V, "E": g.E, "off": off.astype(np.int64), "nbr": nbr,
                         "roff": roff, "rnbr": rnbr, "rrow": rrow, "khop12": g.khop(1, 2), "khop13": g.khop(1, 3)}
        finally:
            g.close()
    return out


def _build(ctx, r, shard=None):
    ctx.staging_clear()
    ctx.set_edge_rowid(False)
    ctx.rank_mode(1)
    ctx.append_vertices(r["vid"])
    ctx.append_edges(r["src"], r["dst"])
    return ctx.build_csr() if shard is None else ctx.build_csr_shard(*shard)


def _figures(st):
    return st["rows"][1], st["rows"][2], st["digest"][1], st["digest"][2]


@pytest.mark.parametrize("name", sorted(TABLES))
def test_counts_and_digests(gg, gg_sorted, refs, name):
    r = refs[name]
    c, s = _build(gg, r), _build(gg_sorted, r)
    try:
        assert (c.V, c.E) == (r["V"], r["E"]) == (s.V, s.E)
        assert s.reverse_derived == 0
        if r["E"] >= 767:  # (whether a table of one or two rows derives is the build's business)
            assert c.reverse_derived == (name in DERIVES)
        got, names = launched(gg, lambda: gg.expand_khop(c, 1, 2))
        assert "expand_mid2" in names and "row_index" not in names
        assert got == r["khop12"] == gg_sorted.expand_khop(s, 1, 2)
        assert gg.expand_khop(c, 2, 2)["digest"][2] == r["khop12"]["digest"][2]
        assert gg.khop_count(c, 1, 2)[1:3] == r["khop12"]["rows"][1:3]
        if name in DERIVES:
            assert not c.reverse_index_ready and not c.reverse_rows_ready
    finally:
        c.close()
        s.close()


def _ranges(gg, csr, r):
    V, roff = r["V"], r["roff"]
    out = []
    for n_parts in (2, 3, 4, 5):
        b = gg.khop_partition_mid(csr, n_parts)
        assert b[0] == 0 and b[-1] == V and list(b) == sorted(b)
        out += list(zip(b, b[1:]))
    live = np.flatnonzero(np.diff(roff))
    empty = np.flatnonzero(np.diff(roff) == 0)
    inside = int(live[np.flatnonzero(roff[live] % R.MT)[len(live) // 3]]) if np.any(roff[live] % R.MT) else int(live[0])
    out += [(inside, V), (0, inside), (inside, min(inside + 3, V))]  # begins inside a tile; ends at V
    if empty.size:
        e = int(empty[empty.size // 2])
        out += [(e, V), (int(empty[0]), e), (e, e + 1)]              # begins on an empty row; a range without entries
    return sorted(set((int(a), int(b)) for a, b in out if a < b))


@pytest.mark.parametrize("name", ["plain_2309", "mirrored_4618", "star", "gaps_plain", "gaps_mirrored"])
def test_middle_ranges(gg, gg_sorted, refs, name):
    """Per-range values against the numpy restatement: a range starts at reverse entry roff[lo], anywhere in a tile."""
    r = refs[name]
    c, s = _build(gg, r), _build(gg_sorted, r)
    try:
        ranges = _ranges(gg, c, r)
        assert not c.reverse_index_ready or name not in DERIVES  # (the partition reads the two offset arrays only)
        for lo, hi in ranges:
            want = R.khop12(r["off"], r["nbr"], r["roff"], r["rnbr"], r["V"], lo, hi)
            assert _figures(gg.expand_khop_mid(c, lo, hi)) == want, (lo, hi)
            assert _figures(gg_sorted.expand_khop_mid(s, lo, hi)) == want, (lo, hi)
        if name in DERIVES:
            assert not c.reverse_index_ready
    finally:
        c.close()
        s.close()


@pytest.mark.parametrize("n_parts", [2, 8])
@pytest.mark.parametrize("name", ["plain_2309", "gaps_plain", "star"])
def test_shards(gg, refs, name, n_parts):
    """A shard keeps the reverse entries whose destination it owns: every other row of its reverse CSR is empty.  Its
    figures are the model's over its own arrays, and the shards' figures add up to the oracle's."""
    r = refs[name]
    total = [0, 0, 0, 0]
    for part in range(n_parts):
        c = _build(gg, r, shard=(part, n_parts))
        try:
            got = _figures(gg.expand_khop(c, 1, 2))
            off, nbr = c.export()[:2]
            roff, rnbr, rrow = c.export_reverse()
            assert np.array_equal(rrow, np.repeat(np.arange(c.V), np.diff(roff)))
            assert got == R.khop12(off, nbr, roff, rnbr, c.V), part
            assert _figures(gg.expand_khop(c, 1, 2)) == got
            total = [a + b for a, b in zip(total, got)]
        finally:
            c.close()
    want = _figures(r["khop12"])
    assert tuple(total[:2]) == want[:2] and (total[2] & R.M32, total[3] & R.M32) == want[2:]


@pytest.mark.parametrize("form,kind,name", cases("ac"))
def test_every_build_route(gg, gg_sorted, tables, form, kind, name):  # noqa: F811
    """Every route of gg_csr_build under every id dictionary: the counting expansion's figures are the oracle's, and those
    of a context that never derives."""
    t = tables(name)
    ctx, csr, vid, idmap = build_table(gg, gg_sorted, form, t, kind)
    try:
        want = t.khop(1, 2)
        assert ctx.expand_khop(csr, 1, 2) == want
        cut = t.V // 3
        mids = [ctx.expand_khop_mid(csr, 0, cut), ctx.expand_khop_mid(csr, cut, t.V)]
        for h in (1, 2):
            assert sum(m["rows"][h] for m in mids) == want["rows"][h]
            assert sum(m["digest"][h] for m in mids) & R.M32 == want["digest"][h]
    finally:
        csr.close()
    if ctx is not gg_sorted:
        s, _ = build_knobs(gg_sorted, form, vid, idmap[t.src], idmap[t.dst], None)
        try:
            assert s.reverse_derived == 0 and gg_sorted.expand_khop(s, 1, 2) == want
        finally:
            s.close()


# ---- the row index on first use ----------------------------------------------------------------------------------------
def _mid_rows(ctx, csr, r):
    res = ctx.expand_khop_mid_result(csr, 0, r["V"], k_min=1)
    try:
        return [np.concatenate([res.fetch(h, o) for o in range(0, res.rows(h), GG_CHUNK_ROWS)]).tolist() for h in (1, 2)]
    finally:
        res.close()


def _components(ctx, csr, r):
    out = ctx.components(csr)
    return {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in out.items()}


def _frontier3(ctx, csr, r):
    ctx.force_frontier(3)  # the product form of an explicit frontier's last two hops, whatever the frontier's size
    try:
        return ctx.expand_khop(csr, 1, 3, sources=r["vid"][::7])
    finally:
        ctx.force_frontier(0)


CONSUMERS = {
    "mid_result_rows": _mid_rows,                                   # khop_materialise_mid2 / k_mat_mid2
    "khop_1_3": lambda ctx, csr, r: ctx.expand_khop(csr, 1, 3),     # khop_count_mid3 / k_mid3_prepare
    "khop_1_3_sources": _frontier3,                                 # the frontier forms
    "components": _components,                                      # gg_components
    "export_index": lambda ctx, csr, r: csr.export_reverse_index().tolist(),
    "export_reverse": lambda ctx, csr, r: [a.tolist() for a in csr.export_reverse()],
}
FIRST_USE = ["mirrored_1536", "mirrored_4618", "gaps_mirrored"]  # (the star's 10^7 2-hop rows are for the counting tests)


@pytest.mark.parametrize("consumer", sorted(CONSUMERS))
@pytest.mark.parametrize("name", FIRST_USE)
def test_index_is_built_by_the_first_consumer(gg, gg_sorted, refs, name, consumer):
    r = refs[name]
    c, s = _build(gg, r), _build(gg_sorted, r)
    try:
        assert c.reverse_derived == 1 and not c.reverse_index_ready and s.reverse_index_ready
        gg.expand_khop(c, 1, 2)
        gg.khop_count(c, 1, 2)
        gg.khop_partition_mid(c, 3)
        gg.expand_khop_mid(c, 1, r["V"])
        assert not c.reverse_index_ready and not c.reverse_rows_ready  # none of the counting calls asks for it
        got, names = launched(gg, lambda: CONSUMERS[consumer](gg, c, r))
        assert "row_index" in names and c.reverse_index_ready
        if consumer in ("components", "export_index"):
            assert not c.reverse_rows_ready and "rotate_rows" not in names  # the index level stops short of the rows
        assert got == CONSUMERS[consumer](gg_sorted, s, r)
        if consumer == "khop_1_3":
            assert got == r["khop13"]
        again, names = launched(gg, lambda: CONSUMERS[consumer](gg, c, r))
        assert again == got and "row_index" not in names  # built once
        assert np.array_equal(c.export_reverse_index(), np.repeat(np.arange(r["V"]), np.diff(r["roff"])))
        assert gg.expand_khop(c, 1, 2) == r["khop12"]  # the same figures with the index in place
    finally:
        c.close()
        s.close()


def test_closing_returns_every_block(gg, refs):
    r = refs["mirrored_1536"]

    def one(touch):
        csr = _build(gg, r)
        try:
            assert csr.reverse_derived == 1
            gg.expand_khop(csr, 1, 2)
            if touch == 1:
                csr.export_reverse_index()
            elif touch == 2:
                csr.export_reverse()
            assert csr.reverse_index_ready == (touch > 0) and csr.reverse_rows_ready == (touch == 2)
        finally:
            csr.close()

    for touch in (0, 1, 2, 0, 1, 2):  # the pool reaches its steady set of blocks
        one(touch)
    before = gg.pool()
    for i in range(30):
        one(i % 3)
    assert gg.pool() == before  # (blocks held, blocks handed out): no leak, no block returned twice
    gg.staging_clear()
