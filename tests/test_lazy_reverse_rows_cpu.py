"""A numpy model of the derived build without its reverse rows (no GPU): on a fully mirrored edge table the build keeps
off == roff, rrow and rot = |A| per vertex; ensure_reverse rotates the forward rows into rnbr on first use, and the
counting 2-hop expansion reads the forward rows in place of the in-rows.  Three facts carry that:
  1. the multiset of every forward row equals the multiset of the reverse row of the same vertex,
  2. the rotation by rot reproduces a stable sort by destination bit for bit,
  3. the khop(1, 2) digests of the C oracle do not change when the in-rows are replaced by the forward rows."""
import numpy as np
import pytest

from tests import lazy_reverse_tables as T
from tests.test_gpu_derived_reverse import reverse_reference


@pytest.fixture(scope="module")
def models(orc):
    """name -> (oracle khop(1, 2), model arrays, sorted reverse): computed once, read by every test, never changed."""
    out = {}
    for name in T.SHAPES + tuple(n for n in T.SMALL if n not in T.SHAPES):
        vid, src, dst = T.table(name)
        rc, g = orc.csr_build(vid, src, dst)
        assert rc == 0
        try:
            o_off, o_nbr, _, o_vid = g.arrays()
            want = g.khop(1, 2) if name in T.SMALL else None
        finally:
            g.close()
        m = T.derived_model(o_vid, src, dst)
        assert np.array_equal(m[0], o_off) and np.array_equal(m[1], o_nbr), name  # the model's forward CSR is the oracle's
        out[name] = (want, m, reverse_reference(o_vid, src, dst))
    return out


ALL = T.SHAPES + ("star_small_out", "star_small_in")


@pytest.mark.parametrize("name", ALL)
def test_offsets_and_coo_column_are_shared(models, name):
    _, (off, nbr, rrow, rot), (roff, rnbr, rrow_sorted) = models[name]
    assert np.array_equal(off, roff) and np.array_equal(rrow, rrow_sorted)
    assert np.all(rot >= 0) and np.all(rot <= np.diff(off))


@pytest.mark.parametrize("name", ALL)
def test_forward_row_is_the_reverse_row_as_a_multiset(models, name):
    _, (off, nbr, rrow, rot), (roff, rnbr, _) = models[name]
    # sorting inside the rows (by row, then value) leaves equal arrays exactly when every pair of rows is one multiset
    assert np.array_equal(nbr[np.lexsort((nbr, rrow))], rnbr[np.lexsort((rnbr, rrow))])


@pytest.mark.parametrize("name", ALL)
def test_rotation_reproduces_the_stable_sort(models, name):
    _, (off, nbr, rrow, rot), (_, rnbr, _) = models[name]
    assert np.array_equal(T.rotate(off, nbr, rrow, rot), rnbr)


def test_tables_cover_the_edge_cases(models):
    """Self-loops, duplicate rows and dropped ids in the `a` tables; vertices with |A| = 0 or |B| = 0 and rows > 0."""
    vid, src, dst = T.table("a_packed")
    off, nbr, rrow, rot = models["a_packed"][1]
    assert np.any(nbr == rrow)                                     # self-loops
    assert nbr.size < src.size and (src.size - nbr.size) % 2 == 0  # ids that are no vertex, dropped in pairs
    pairs = rrow * vid.size + nbr
    assert np.unique(pairs).size < pairs.size                      # duplicate rows
    for name, hub_rot_is_deg in (("star_out", True), ("star_in", False)):
        off, nbr, rrow, rot = models[name][1]
        deg = np.diff(off)
        hub = int(np.argmax(deg))
        assert deg[hub] >= 2000 and rot[hub] == (deg[hub] if hub_rot_is_deg else 0)
        assert np.any((deg > 0) & (rot == 0)) and np.any((deg > 0) & (rot == deg))


def _digests(orc, off, nbr, rrow, in_rows):
    """khop(1, 2) from every vertex the way k_expand_mid2 walks it: entry p of the in-rows is the 1-hop row u -> x with
    x = rrow[p], u = in_rows[p], and every w of x's forward row ends a 2-hop row u -> x -> w."""
    rows2, d1, d2 = 0, 0, 0
    for p in range(in_rows.size):
        u, x = int(in_rows[p]), int(rrow[p])
        d1 = (d1 + (orc.row_hash([u, x]) & 0xFFFFFFFF)) & 0xFFFFFFFF
        for w in nbr[off[x]:off[x + 1]]:
            d2 = (d2 + (orc.row_hash([u, x, int(w)]) & 0xFFFFFFFF)) & 0xFFFFFFFF
            rows2 += 1
    return in_rows.size, rows2, d1, d2


@pytest.mark.parametrize("name", T.SMALL)
def test_oracle_digests_do_not_change_with_forward_rows_as_in_rows(orc, models, name):
    want, (off, nbr, rrow, rot), (_, rnbr, _) = models[name]
    expect = (want["rows"][1], want["rows"][2], want["digest"][1], want["digest"][2])
    assert _digests(orc, off, nbr, rrow, rnbr) == expect  # the walk itself: the oracle's figures from the in-rows
    assert _digests(orc, off, nbr, rrow, nbr) == expect   # and from the forward rows in their place
