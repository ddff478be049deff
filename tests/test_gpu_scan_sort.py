"""The shared exclusive scan (scan_exclusive_u32 / _u64, gg_runtime.hip) and the shared stable radix sort
(radix_sort_stable behind sort_pairs_by_key / sort_triples_by_key, gg_csr.hip) on their own, through gg_debug_scan and
gg_debug_sort_pairs, against numpy: cumsum in uint64 and argsort(kind="stable").  Every comparison is exact.

The sizes are the ones at which the code takes another path: the scan's tiles of 4096 are chained by a look-back over 64
predecessors at a time, so 64, 65, 66 and 130 tiles give it one, two and three trips; the sort has tiles of 4096 and at
most 8 bits a pass, so the key widths give one to four passes with even and uneven last passes.

Every 64-bit sum here stays below 2^62: the scan's status word keeps its flag in the top two bits (gg_internal.h), and
what a larger sum does is not defined."""
import numpy as np
import pytest

from duckdb_pgq_amd.gg import SORT_PREFILL, GGError

pytestmark = pytest.mark.gpu

TILE = 4096
SCAN_N = [0, 1, 63, 64, 65, 4095, 4096, 4097, 64 * TILE, 64 * TILE + 1, 65 * TILE + 1, 129 * TILE + 5]
SORT_N = [n for n in SCAN_N if n <= 65 * TILE + 1]
KEY_BITS = [1, 7, 8, 9, 16, 17, 24, 25, 31]
INVALID = 0xFFFFFFFF


# ---- scan ------------------------------------------------------------------------------------------------------------
def _scan_inputs(n, dtype):
    """name -> values; every sum below 2^62 (width 8) and, for width 4, some above 2^32"""
    rng = np.random.default_rng(0x5CA0 + n)
    big = np.uint64(1) << np.uint64(61) if dtype == np.uint64 else np.uint64(0xFFFFFFFF)
    tiles = (n + TILE - 1) // TILE
    out = {"zeros": np.zeros(n, dtype), "ones": np.ones(n, dtype)}
    if n:
        for name, at in (("big_first", 0), ("big_last", n - 1), ("big_middle", min(n - 1, (tiles // 2) * TILE + 17))):
            a = np.ones(n, dtype)
            a[at] = big
            out[name] = a
    # random: below 2^40 in 64 bits (530 k of them stay below 2^60); the whole 32-bit range in 32 bits, so the sum of
    # any two tiles of them passes 2^32
    out["random"] = rng.integers(0, 1 << 40 if dtype == np.uint64 else 1 << 32, n, dtype=np.uint64).astype(dtype)
    if dtype == np.uint32:
        out["all_max"] = np.full(n, 0xFFFFFFFF, dtype)  # the sum passes 2^32 from the second element on
    return out


def _scan_ref(a):
    wide = a.astype(np.uint64)
    incl = np.cumsum(wide, dtype=np.uint64)
    total = int(incl[-1]) if a.size else 0
    assert total < 1 << 62
    excl = np.zeros(a.size, np.uint64)
    excl[1:] = incl[:-1]
    return excl.astype(a.dtype), total  # (uint32: the prefix mod 2^32)


@pytest.mark.parametrize("width", [4, 8])
@pytest.mark.parametrize("n", SCAN_N)
def test_scan_matches_cumsum(gg, n, width):
    dtype = np.uint32 if width == 4 else np.uint64
    inputs = _scan_inputs(n, dtype)
    passed_2_32 = False
    for name, a in inputs.items():
        want, want_total = _scan_ref(a)
        passed_2_32 |= want_total >= 1 << 32
        for in_place in (False, True):
            before = a.copy()
            got, total = gg.debug_scan(a, in_place=in_place)
            assert np.array_equal(a, before), (name, in_place)
            assert total == want_total, (name, in_place, total, want_total)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (name, in_place, "first wrong prefix at", int(bad[0]), "tile", int(bad[0]) // TILE,
                                   int(got[bad[0]]), int(want[bad[0]]))
    if width == 4 and n >= 2:
        assert passed_2_32  # the wrap of the 32-bit prefix was exercised


def test_scan_u32_prefix_wraps_and_total_does_not(gg):
    """pinned: out holds the prefix mod 2^32, total the exact sum"""
    a = np.full(3 * TILE + 1, 0xFFFFFFFF, np.uint32)
    got, total = gg.debug_scan(a)
    assert total == a.size * 0xFFFFFFFF and total > 1 << 32
    i = np.arange(a.size, dtype=np.uint64)
    assert np.array_equal(got, ((i * np.uint64(0xFFFFFFFF)) & np.uint64(0xFFFFFFFF)).astype(np.uint32))
    assert got[1] == 0xFFFFFFFF and got[2] == 0xFFFFFFFE


def test_scan_refuses_other_widths(gg):
    import ctypes as C

    a = np.zeros(4, np.uint32)
    total = C.c_uint64()
    assert gg.lib.gg_debug_scan(gg.ctx, a.ctypes.data, 4, 2, a.ctypes.data, C.byref(total)) != 0
    assert gg.debug_scan(np.ones(5, np.uint32))[1] == 5


# ---- sort ------------------------------------------------------------------------------------------------------------
def _sort_keys(n, key_bits):
    rng = np.random.default_rng(0x50B7 * 64 + key_bits + n)
    top = (1 << key_bits) - 1
    rnd = rng.integers(0, top + 1, n, dtype=np.uint64).astype(np.uint32)
    out = {
        "equal": np.full(n, top // 3, np.uint32),  # stability is the whole answer
        "sorted": np.sort(rnd),
        "reversed": np.sort(rnd)[::-1].copy(),
        "two_values": np.where(rng.integers(0, 2, n) == 1, top, 0).astype(np.uint32),
        "random": rnd,
    }
    if key_bits == 31 and n:
        a = rnd.copy()
        a[rng.integers(0, n, max(1, n // 5))] = (1 << 31) - 1  # the largest key a caller may pass
        a[n // 2] = (1 << 31) - 1
        out["with_2_31_minus_1"] = a
    return out


def _check_sort(gg, key, key_bits, triples, label):
    n = key.size
    pos = np.arange(n, dtype=np.uint32)  # the payload is the position: stability is visible
    b = (pos * np.uint32(2654435761)) if triples else None
    k_out, a_out, b_out, n_valid = gg.debug_sort_pairs(key, pos, b, key_bits)
    valid = key != INVALID
    nv = int(valid.sum())
    assert n_valid == nv, (label, n_valid, nv)
    order = np.argsort(key[valid], kind="stable")
    assert np.array_equal(k_out[:nv], key[valid][order]), label
    assert np.array_equal(a_out[:nv], pos[valid][order]), label
    assert (k_out[nv:] == SORT_PREFILL).all() and (a_out[nv:] == SORT_PREFILL).all(), label
    if triples:
        assert np.array_equal(b_out[:nv], b[valid][order]), label
        assert (b_out[nv:] == SORT_PREFILL).all(), label
    else:
        assert b_out is None


@pytest.mark.parametrize("key_bits", KEY_BITS)
@pytest.mark.parametrize("n", SORT_N)
def test_sort_matches_stable_argsort(gg, n, key_bits):
    for name, key in _sort_keys(n, key_bits).items():
        assert key.size == 0 or int(key.max()) < 1 << key_bits
        for triples in (False, True):
            _check_sort(gg, key, key_bits, triples, (name, triples))


@pytest.mark.parametrize("key_bits", KEY_BITS)
@pytest.mark.parametrize("n", SORT_N)
def test_sort_drops_the_no_element_key(gg, n, key_bits):
    """The contract the builds rely on: a key of 0xFFFFFFFF (out of range for every key_bits a caller may pass) is no
    element — it is not counted, the others are sorted stably in front, and the slots behind them are not written."""
    rng = np.random.default_rng(0xD20 + 64 * n + key_bits)
    base = _sort_keys(n, key_bits)
    cases = {}
    for name in ("random", "two_values"):
        key = base[name].copy()
        key[rng.random(n) < 0.125] = INVALID
        if n >= 2:
            key[0] = key[-1] = INVALID
        if n > TILE:
            key[TILE:2 * TILE] = INVALID  # a whole tile without an element
        cases[name + "_sprinkled"] = key
    cases["none_left"] = np.full(n, INVALID, np.uint32)
    for name, key in cases.items():
        for triples in (False, True):
            _check_sort(gg, key, key_bits, triples, (name, triples))


@pytest.mark.parametrize("key_bits", [32, 33, 64])
def test_sort_refuses_whole_word_keys(gg, key_bits):
    key = np.arange(100, dtype=np.uint32)[::-1].copy()
    with pytest.raises(GGError) as e:
        gg.debug_sort_pairs(key, key, None, key_bits)
    assert "internal:" in str(e.value)
    _check_sort(gg, key, 7, True, "after the refusal")  # the context still works
    assert gg.debug_scan(np.ones(TILE + 1, np.uint32))[1] == TILE + 1
