"""The top-n restatement (tests/khop_aggregate_top_ref.py) pinned against a brute-force ordering of the group-by over the
walk rows and, where the compiled reference is present, against the reference's own TopN-above-hash-aggregate plan read as
text in result order.  One test needs the built library but no GPU: the C-ABI exports the new entry points."""
import ctypes as C

import numpy as np
import pytest

from oracle import ref_duckdb as R
from tests import edge_filter_ref as F
from tests import khop_aggregate_ref as K
from tests import khop_aggregate_top_ref as KT
from tests import triangles_ref as T


@pytest.fixture(scope="module")
def hard():
    """weights and biases below 2^40: no bias + sum leaves 128 bits (the reference raises there where the library wraps),
    yet the sums collide often enough that the id decides some places (weights of a few values only)"""
    vid, src, dst = T.hard_graph(V=300, rows=3000, seed=0x51, hub_fan=120)
    g = T.TriangleGraph(vid, src, dst)
    rng = np.random.RandomState(0x70B)
    w = rng.choice(np.array([-(1 << 40), -3, 0, 1, 1, 2, 1 << 40], np.int64), size=g.V)
    bias = rng.choice(np.array([-(1 << 41), -1, 0, 0, 5, 1 << 41], np.int64), size=g.V)
    return vid, src, dst, g, w, bias


def brute_force(g, rows, group_by, w, n, order_by, descending, bias):
    """order the groups of the walk rows one comparison at a time (a selection sort over python tuples)"""
    ids, walks, totals = K.group_rows(g, rows, group_by, w)
    left = [(int(i), int(c), int(t)) for i, c, t in zip(ids.tolist(), walks, totals)]
    out = []
    while left and len(out) < n:
        best = left[0]
        for r in left[1:]:
            kr = r[1] if order_by == "walks" else K.wrap128(r[2] + (bias[g.index[r[0]]] if bias is not None else 0))
            kb = best[1] if order_by == "walks" else K.wrap128(best[2] + (bias[g.index[best[0]]] if bias is not None else 0))
            better = kr > kb if descending else kr < kb
            if better or (kr == kb and r[0] < best[0]):
                best = r
        out.append(best)
        left.remove(best)
    return (np.array([r[0] for r in out], np.int64), [r[1] for r in out], [r[2] for r in out])


@pytest.mark.parametrize("group_by", K.GROUPS)
@pytest.mark.parametrize("h", [1, 2])
def test_restatement_equals_a_brute_force_ordering_of_the_group_by(hard, h, group_by):
    vid, src, dst, g, w, bias = hard
    level = K.aggregate(g, h, group_by, None, w)[h]
    rows = F.walks(g, None, h)
    groups = len(level[1])
    b = [int(x) for x in bias.tolist()]
    ties = 0
    for order_by, biased in (("total", False), ("total", True), ("walks", False)):
        for descending in (True, False):
            for n in (0, 1, 7, groups, groups + 5):
                got = KT.top(level, n, order_by, descending, KT.bias_by_id(g, bias) if biased else None)
                assert K.same(got, brute_force(g, rows, group_by, w, n, order_by, descending, b if biased else None))
                assert len(got[1]) == min(n, groups)
            ties += groups - len(set(level[1] if order_by == "walks" else level[2]))
    assert ties > 0  # equal keys exist: the id decided some places


def test_keys_wrap_and_walks_compare_unsigned():
    level = (np.array([5, -7, 9, 2], np.int64), [1 << 63, 3, (1 << 64) - 1, 3], [(1 << 127) - 1, -(1 << 127), 0, -1])
    assert KT.top(level, 4, "walks", True)[0].tolist() == [9, 5, -7, 2]   # 2^64 - 1 and 2^63 are large, not negative
    assert KT.top(level, 4, "walks", False)[0].tolist() == [-7, 2, 5, 9]  # the tie keeps the smaller id first
    assert KT.top(level, 4, "total", True)[0].tolist() == [5, 9, 2, -7]
    # + 1 carries the largest total over the top: it wraps to the smallest key; the rows keep their unbiased totals
    got = KT.top(level, 2, "total", True, {5: 1, -7: 0, 9: 0, 2: 0})
    assert got[0].tolist() == [9, 2] and got[2] == [0, -1]
    assert KT.top(level, 4, "total", False, {5: 1, -7: 1, 9: 0, 2: 0})[0].tolist() == [5, -7, 2, 9]


def test_the_library_exports_the_entry_points_and_the_binding_has_the_methods():
    import duckdb_pgq_amd as pkg
    from duckdb_pgq_amd import gg as binding

    lib = C.CDLL(binding.LIB_PATH)
    for name in ("gg_khop_aggregate_top", "gg_debug_aggregate_top", "gg_debug_aggregate_top_listed"):
        assert hasattr(lib, name) and name in binding.SYMBOLS
    assert callable(getattr(pkg.GG, "khop_aggregate_top", None)) and callable(getattr(pkg.GG, "debug_aggregate_top", None))
    assert callable(getattr(pkg.GG, "debug_aggregate_top_listed", None))
    assert C.sizeof(binding.TopStats) == 24 and binding.TOP_BY == {"total": 0, "walks": 1}


needs_reference = pytest.mark.skipif(not R.available(), reason="reference build not present")


@pytest.fixture(scope="module")
def ref(hard):
    vid, src, dst, g, w, bias = hard
    d = R.RefDuckDB(threads=4)
    d.load_table("person", {"p_personid": vid, "p_score": w, "p_bias": bias})
    d.load_table("knows", {"k_person1id": src, "k_person2id": dst})
    yield d
    d.close()


@needs_reference
def test_bigint_plus_hugeint_binds_in_the_reference(ref):
    """the ORDER BY expression p_bias + sum(p_score) needs no CAST in this vintage"""
    rows = ref.query_text("SELECT p_personid, p_bias + sum(p_score) FROM person GROUP BY p_personid, p_bias "
                          "ORDER BY p_bias + sum(p_score) DESC, p_personid LIMIT 3")
    assert len(rows) == 3


@needs_reference
@pytest.mark.parametrize("group_by", K.GROUPS)
@pytest.mark.parametrize("h", [1, 2])
def test_against_the_reference_top_n_above_its_hash_aggregate(hard, ref, h, group_by):
    vid, src, dst, g, w, bias = hard
    level = K.aggregate(g, h, group_by, None, w)[h]
    groups = len(level[1])
    assert groups > 7
    for order_by, biased in (("total", False), ("total", True), ("walks", False)):
        for descending in (True, False):
            for n in (1, 7, groups, groups + 5):
                want = KT.top(level, n, order_by, descending, KT.bias_by_id(g, bias) if biased else None)
                sql = KT.sql_khop_aggregate_top(h, group_by, n, order_by, descending, biased=biased)
                got = [tuple(int(x) for x in r[:3]) for r in ref.query_text(sql)]  # in result order, not re-sorted
                assert got == list(zip(want[0].tolist(), want[1], want[2])), (order_by, biased, descending, n)
