"""A derived build (fully mirrored edge table) writes no reverse rows: it keeps roff == off, rrow and one rotation count
per vertex, the counting 1- and 2-hop calls read the forward rows in place of the in-rows, and the first call that
needs the rows themselves has them rotated into place (gg_csr.hip: ensure_reverse).  Every table is built on the
default context and on one created with GG_MIRROR_REVERSE=0, which sorts its reverse rows during the build as ever:
the two must agree on every figure and every row, and with the oracle and numpy where those have the answer."""
import os

import numpy as np
import pytest

import duckdb_pgq_amd as pkg
from duckdb_pgq_amd import datagen
from duckdb_pgq_amd.gg import GG_CHUNK_ROWS
from tests import lazy_reverse_tables as T
from tests.test_gpu_derived_reverse import mirrored, reverse_reference

pytestmark = pytest.mark.gpu

M32 = 0xFFFFFFFF


@pytest.fixture(scope="module")
def gg_sorted():
    """A second context that never derives: GG_MIRROR_REVERSE=0 at its creation."""
    old = os.environ.get("GG_MIRROR_REVERSE")
    os.environ["GG_MIRROR_REVERSE"] = "0"
    try:
        g = pkg.GG(0)
    finally:
        if old is None:
            del os.environ["GG_MIRROR_REVERSE"]
        else:
            os.environ["GG_MIRROR_REVERSE"] = old
    yield g
    g.close()


def _mid_window(off, roff, most=250_000, enough=20_000):
    """[lo, hi): a few middle vertices with between `enough` and `most` 2-hop rows through them (fetched 1 024 at a time)."""
    prod = np.diff(roff) * np.diff(off)
    lo = 0
    while True:
        total, hi = 0, lo
        while hi < prod.size and total < enough and total + prod[hi] <= most:
            total += int(prod[hi])
            hi += 1
        if total:
            return lo, hi
        lo = hi + 1  # (a vertex with more rows than `most` on its own: start behind it)
        assert lo < prod.size


@pytest.fixture(scope="module")
def refs(orc):
    """name -> the table and what the oracle and numpy say about it: computed once, shared, never changed."""
    out = {}
    for name in T.SHAPES:
        vid, src, dst = T.table(name)
        rc, g = orc.csr_build(vid, src, dst)
        assert rc == 0
        try:
            off, _, _, o_vid = g.arrays()
            rev = reverse_reference(o_vid, src, dst)
            out[name] = {"vid": vid, "src": src, "dst": dst, "V": g.V, "E": g.E, "khop12": g.khop(1, 2),
                         "khop22": g.khop(2, 2), "rev": rev, "window": _mid_window(off, rev[0]),
                         "sources": datagen.pick_sources(vid, 64, 1)}
        finally:
            g.close()
    return out


def _build(ctx, vid, src, dst):
    ctx.staging_clear()
    ctx.set_edge_rowid(False)
    ctx.rank_mode(1)
    ctx.append_vertices(vid)
    ctx.append_edges(src, dst)
    return ctx.build_csr()


@pytest.fixture
def both(gg, gg_sorted):
    """Builds (deriving csr, sorted csr) of a table; closes what it built and resets both contexts afterwards."""
    made = []

    def build(r, derived=1):
        pair = []
        for ctx in (gg, gg_sorted):
            csr = _build(ctx, r["vid"], r["src"], r["dst"])
            made.append(csr)
            pair.append(csr)
        assert pair[0].reverse_derived == derived and pair[1].reverse_derived == 0
        assert pair[0].reverse_rows_ready == (not derived) and pair[1].reverse_rows_ready
        return pair

    yield build
    for csr in made:
        csr.close()
    for ctx in (gg, gg_sorted):
        ctx.debug_reset()
        ctx.staging_clear()


def _counting(ctx, csr, V):
    cut = max(1, V // 3)
    return {"khop12": ctx.expand_khop(csr, 1, 2), "khop22": ctx.expand_khop(csr, 2, 2),
            "mid": [ctx.expand_khop_mid(csr, 0, cut), ctx.expand_khop_mid(csr, cut, V)],  # two proper sub-ranges
            "count": ctx.khop_count(csr, 1, 2)}


def _check_counting(got, r):
    assert got["khop12"] == r["khop12"] and got["khop22"] == r["khop22"]
    for h in (1, 2):  # the sub-ranges cut the middle vertices in two: their figures add up to the oracle's
        assert sum(m["rows"][h] for m in got["mid"]) == r["khop12"]["rows"][h]
        assert (got["mid"][0]["digest"][h] + got["mid"][1]["digest"][h]) & M32 == r["khop12"]["digest"][h]
    assert got["count"][1:3] == r["khop12"]["rows"][1:3]


@pytest.mark.parametrize("name", T.SHAPES)
def test_counting_calls_leave_the_rows_unwritten_and_the_export_writes_them(gg, gg_sorted, both, refs, name):
    r = refs[name]
    c, s = both(r)
    assert (c.V, c.E) == (r["V"], r["E"]) == (s.V, s.E)
    got = _counting(gg, c, r["V"])
    assert not c.reverse_rows_ready  # 1- and 2-hop counting, whole and by middle range, never touched them
    _check_counting(got, r)
    assert got == _counting(gg_sorted, s, r["V"])
    rev = c.export_reverse()
    assert c.reverse_rows_ready
    for label, a, b, w in zip(("roff", "rnbr", "rrow"), rev, s.export_reverse(), r["rev"]):
        assert np.array_equal(a, w) and np.array_equal(b, w), label
    assert _counting(gg, c, r["V"]) == got  # the same values with the rows in place
    assert c.reverse_rows_ready


def _mid_rows(ctx, csr, r):
    res = ctx.expand_khop_mid_result(csr, *r["window"])
    try:
        n = res.rows(2)
        assert 0 < n <= 250_000
        return np.concatenate([res.fetch(2, o) for o in range(0, n, GG_CHUNK_ROWS)])
    finally:
        res.close()


def _aggregate(ctx, csr, r):
    a = ctx.khop_aggregate(csr, 1, 2, group_by="end")
    try:
        return a.stats["groups"], a.stats["walks"], [[list(map(int, col)) for col in a.fetch(h)] for h in (1, 2)]
    finally:
        a.close()


def _pair_counts(ctx, csr, r):
    p = ctx.khop_pair_counts(csr, 1, 2, sources=r["sources"])
    try:
        return p.stats["pairs"], p.stats["walks"], [[col.tolist() for col in p.fetch(h)] for h in (1, 2)]
    finally:
        p.close()


def _bfs(ctx, csr, r):
    dist, st = ctx.bfs64(csr, r["sources"], 5)
    return dist.tolist(), st


CONSUMERS = {
    "mid_result_rows": lambda ctx, csr, r: _mid_rows(ctx, csr, r).tolist(),  # row for row, in order
    "khop_1_3": lambda ctx, csr, r: ctx.expand_khop(csr, 1, 3),
    "khop_count_1_3": lambda ctx, csr, r: ctx.khop_count(csr, 1, 3),
    "bfs64": _bfs,
    "aggregate_by_end": _aggregate,
    "pair_counts": _pair_counts,
}


@pytest.mark.parametrize("consumer", sorted(CONSUMERS))
@pytest.mark.parametrize("name", T.SHAPES)
def test_first_touch_by_each_consumer(gg, gg_sorted, both, refs, name, consumer):
    """A fresh build each, so that the rotation is this consumer's own first touch."""
    r = refs[name]
    c, s = both(r)
    got = CONSUMERS[consumer](gg, c, r)
    want = CONSUMERS[consumer](gg_sorted, s, r)
    assert got == want
    if consumer != "bfs64":  # (five levels give the BFS its chance to pull; whether it does is the frontier's business)
        assert c.reverse_rows_ready  # each of the others reads the rows themselves
    assert np.array_equal(c.export_reverse()[1], r["rev"][1])


def test_closing_with_and_without_the_rows_returns_every_block(gg, refs):
    r = refs["a_packed"]

    def one(rotate):
        csr = _build(gg, r["vid"], r["src"], r["dst"])
        try:
            assert csr.reverse_derived == 1
            if rotate:
                csr.export_reverse()
            assert csr.reverse_rows_ready == rotate
        finally:
            csr.close()

    for rotate in (False, True, False, True):  # the pool reaches its steady set of blocks
        one(rotate)
    before = gg.pool()
    for i in range(50):
        one(i % 2 == 1)
    assert gg.pool() == before  # (blocks held, blocks handed out): no leak, no block returned twice
    gg.staging_clear()


@pytest.mark.parametrize("how", ["odd", "one_broken_pair", "shuffled"])
def test_tables_that_do_not_derive_have_their_rows_from_the_build(gg, gg_sorted, both, orc, how):
    rng = np.random.default_rng(len(how))
    vid = T.ids("packed", 5000, rng)
    src, dst = mirrored(vid, 40_001 if how == "odd" else 40_000, rng)
    if how == "one_broken_pair":
        dst = dst.copy()
        dst[-1] = vid[(int(np.flatnonzero(vid == dst[-1])[0]) + 1) % vid.size]
    elif how == "shuffled":
        p = rng.permutation(src.size)
        src, dst = src[p], dst[p]
    rc, g = orc.csr_build(vid, src, dst)
    assert rc == 0
    try:
        want, rev = g.khop(1, 2), reverse_reference(g.arrays()[3], src, dst)
    finally:
        g.close()
    c, s = both({"vid": vid, "src": src, "dst": dst}, derived=0)
    for ctx, csr in ((gg, c), (gg_sorted, s)):
        assert ctx.expand_khop(csr, 1, 2) == want
        assert all(np.array_equal(a, b) for a, b in zip(csr.export_reverse(), rev))
        assert csr.reverse_rows_ready
