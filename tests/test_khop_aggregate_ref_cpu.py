"""The grouped-aggregate restatement (tests/khop_aggregate_ref.py) pinned against a brute-force group-by over the walk rows
of tests/edge_filter_ref.walks and, where the compiled reference is present, against the reference's own hash-aggregate
plan read as HUGEINT text.  One test needs the built library but no GPU: the C-ABI exports the four entry points."""
import ctypes as C

import numpy as np
import pytest

from oracle import ref_duckdb as R
from tests import edge_filter_ref as F
from tests import khop_aggregate_ref as K
from tests import triangles_ref as T


def weights_of(V, seed=0xA66):
    """random int64 weights with the extremes in front: sums of a few of them leave the int64 range in both directions"""
    rng = np.random.RandomState(seed)
    w = rng.randint(-(1 << 62), 1 << 62, size=V, dtype=np.int64) * 2 + rng.randint(0, 2, size=V)
    w[:4] = [-(1 << 63), (1 << 63) - 1, -1, 0]
    return w


@pytest.fixture(scope="module")
def hard():
    vid, src, dst = T.hard_graph(V=300, rows=3000, seed=0x51, hub_fan=120)
    g = T.TriangleGraph(vid, src, dst)
    return vid, src, dst, g, weights_of(g.V)


def listed(g):
    """a list with a duplicate and an id that is no vertex"""
    hub = int(np.bincount(g.dv, minlength=g.V).argmax())
    return np.concatenate([g.vid[[hub, 3, hub, 17]], [-123456789]])


@pytest.mark.parametrize("group_by", K.GROUPS)
@pytest.mark.parametrize("which", ["all", "list"])
def test_restatement_equals_the_group_by_over_the_walk_rows(hard, group_by, which):
    vid, src, dst, g, w = hard
    S = None if which == "all" else listed(g)
    got = K.aggregate(g, 3, group_by, S, w)
    counts = K.aggregate(g, 3, group_by, S, None)
    for h in (1, 2, 3):
        rows = F.walks(g, S, h)
        assert rows.shape[0] > 0
        assert K.same(got[h], K.group_rows(g, rows, group_by, w))
        assert sum(got[h][1]) == rows.shape[0]
        # without weights the total is the count
        assert K.same(counts[h], K.group_rows(g, rows, group_by, None)) and counts[h][1] == counts[h][2]
    if which == "list":  # the duplicate doubles its group when grouping by the start
        once = K.aggregate(g, 1, "start", np.unique(S), w)[1]
        twice = K.aggregate(g, 1, "start", S, w)[1]
        hub = int(S[0])
        i, j = once[0].tolist().index(hub), twice[0].tolist().index(hub)
        assert twice[1][j] == 2 * once[1][i] and twice[2][j] == K.wrap128(2 * once[2][i])


def test_totals_leave_the_int64_range_and_wrap_only_at_128_bits(hard):
    vid, src, dst, g, w = hard
    got = K.aggregate(g, 2, "start", None, w)
    assert any(abs(t) >= 1 << 63 for t in got[2][2])
    assert K.wrap128((1 << 127) + 5) == -(1 << 127) + 5 and K.wrap128(-1) == -1 and K.wrap128(1 << 128) == 0


def test_the_library_exports_the_entry_points_and_the_binding_has_the_methods():
    import duckdb_pgq_amd as pkg
    from duckdb_pgq_amd import gg as binding

    lib = C.CDLL(binding.LIB_PATH)
    for name in ("gg_khop_aggregate", "gg_khop_aggregate_rows", "gg_khop_aggregate_fetch", "gg_debug_aggregate_long_row"):
        assert hasattr(lib, name) and name in binding.SYMBOLS
    assert callable(getattr(pkg.GG, "khop_aggregate", None)) and callable(getattr(pkg.GG, "debug_aggregate_long_row", None))


needs_reference = pytest.mark.skipif(not R.available(), reason="reference build not present")


@pytest.fixture(scope="module")
def ref(hard):
    vid, src, dst, g, w = hard
    d = R.RefDuckDB(threads=4)
    d.load_table("person", {"p_personid": vid, "p_score": w})
    d.load_table("knows", {"k_person1id": src, "k_person2id": dst})
    yield d
    d.close()


@needs_reference
@pytest.mark.parametrize("group_by", K.GROUPS)
@pytest.mark.parametrize("h", [1, 2])
def test_against_the_reference_hash_aggregate_plan(hard, ref, h, group_by):
    vid, src, dst, g, w = hard
    want = K.aggregate(g, h, group_by, None, w)[h]
    assert any(abs(t) >= 1 << 63 for t in want[2])  # the HUGEINT column is needed
    got = sorted((int(a), int(b), int(c)) for a, b, c in ref.query_text(K.sql_khop_aggregate(h, group_by)))
    assert got == sorted(zip(want[0].tolist(), want[1], want[2]))
