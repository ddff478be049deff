"""The numpy restatement of gg_result_filter_value / gg_result_top_rows (tests/value_rows_ref.py) against its python-loop
twin on random small tables, and against hand-written cases: INT64_MIN and INT64_MAX as values and as bounds, lo > hi,
lo == hi, ties straddling n.  No GPU."""
import numpy as np
import pytest

from tests import value_rows_ref as R

LO, HI = R.I64_MIN, R.I64_MAX


def same(a, b):
    assert np.array_equal(a[0], b[0]) and a[2] == b[2]
    assert (a[1] is None and b[1] is None) or np.array_equal(a[1], b[1])


@pytest.mark.parametrize("seed", range(6))
def test_random_small_tables_equal_the_loops(seed):
    rng = np.random.RandomState(seed)
    V, N, width = 40, 150, 3
    ids = rng.permutation(200)[:V].astype(np.int64) - 100
    values = rng.randint(-3, 4, V).astype(np.int64)
    values[:4] = [LO, HI, -1, 0]
    bits = rng.rand(V) > 0.2
    table = rng.randint(-100, 100, (N, width)).astype(np.int64)
    edges = rng.randint(0, 1000, (N, width - 1)).astype(np.int64)
    for valid in (None, R.pack_valid(bits), R.pack_valid(np.zeros(V, bool))):
        for col in range(width):
            for lo, hi in ((-1, 2), (LO, HI), (2, -1), (0, 0), (LO, LO), (HI, HI), (LO, -1), (1, HI)):
                for mode in ("in", "not_in"):
                    a = R.filter_rows(table, edges, col, ids, values, valid, lo, hi, mode)
                    same(a, R.filter_rows_loop(table, edges, col, ids, values, valid, lo, hi, mode))
                    for desc in (False, True):
                        for tie in (None, 0, width - 1):
                            for n in (0, 1, 7, a[2]["rows_out"], a[2]["rows_out"] + 3):
                                same(R.top_rows(table, edges, col, ids, values, valid, lo, hi, mode, desc, tie, n),
                                     R.top_rows_loop(table, edges, col, ids, values, valid, lo, hi, mode, desc, tie, n))


def test_valid_bits_round_trip():
    rng = np.random.RandomState(3)
    for V in (1, 63, 64, 65, 200):
        bits = rng.rand(V) > 0.5
        assert np.array_equal(R.valid_bits(R.pack_valid(bits), V), bits)
    assert R.valid_bits(None, 5).all()


IDS = np.array([10, 20, 30, 40, 50], np.int64)
VALUES = np.array([LO, HI, 0, -1, 7], np.int64)
TABLE = np.array([[10, 1], [20, 2], [30, 3], [40, 4], [50, 5], [60, 6], [30, 0], [30, 3]], np.int64)  # 60: no vertex


def test_hand_written_filter_cases():
    f = lambda lo, hi, mode, valid=None: R.filter_rows(TABLE, None, 0, IDS, VALUES, valid, lo, hi, mode)
    rows, e, st = f(LO, HI, "in")
    assert e is None and st == {"rows_in": 8, "rows_valued": 7, "rows_out": 7} and rows[:, 1].tolist() == [1, 2, 3, 4, 5, 0, 3]
    assert f(LO, HI, "not_in")[2]["rows_out"] == 0                      # nothing lies outside everything
    assert f(LO, LO, "in")[0].tolist() == [[10, 1]]                     # INT64_MIN as value and bound
    assert f(HI, HI, "in")[0].tolist() == [[20, 2]]
    assert f(LO + 1, HI - 1, "not_in")[0][:, 0].tolist() == [10, 20]
    assert f(1, 0, "in")[2]["rows_out"] == 0                            # lo > hi: IN keeps nothing
    assert f(1, 0, "not_in")[2]["rows_out"] == 7                        # ... NOT_IN every valued row, never the unvalued one
    assert f(0, 0, "not_in")[0][:, 0].tolist() == [10, 20, 40, 50]      # <>
    assert f(0, 0, "in")[0][:, 1].tolist() == [3, 0, 3]
    no30 = R.pack_valid(IDS != 30)
    assert f(LO, HI, "in", no30)[2] == {"rows_in": 8, "rows_valued": 4, "rows_out": 4}   # a NULL passes nothing
    assert f(0, 0, "not_in", no30)[0][:, 0].tolist() == [10, 20, 40, 50]
    assert f(1, 0, "not_in", R.pack_valid(np.zeros(5, bool)))[2] == {"rows_in": 8, "rows_valued": 0, "rows_out": 0}
    # the second column's cells are no vertices at all
    assert R.filter_rows(TABLE, None, 1, IDS, VALUES, None, LO, HI, "in")[2]["rows_valued"] == 0


def test_hand_written_top_cases():
    t = lambda desc, tie, n, lo=LO, hi=HI, mode="in": R.top_rows(TABLE, TABLE[:, 1:] * 10, 0, IDS, VALUES, None, lo, hi, mode,
                                                                   desc, tie, n)
    rows, e, st = t(True, None, 100)
    assert rows[:, 0].tolist() == [20, 50, 30, 30, 30, 40, 10]           # INT64_MAX first, INT64_MIN last
    assert rows[:, 1].tolist() == [2, 5, 3, 0, 3, 4, 1]                  # ties by input row
    assert np.array_equal(e, rows[:, 1:] * 10)
    assert st == {"rows_in": 8, "rows_valued": 7, "candidates": 7, "rows_out": 7}
    assert t(False, None, 100)[0][:, 0].tolist() == [10, 40, 30, 30, 30, 50, 20]
    assert t(True, 1, 100)[0][:, 1].tolist() == [2, 5, 0, 3, 3, 4, 1]    # ties by id ascending, in both directions
    assert t(False, 1, 100)[0][:, 1].tolist() == [1, 4, 0, 3, 3, 5, 2]
    # n cuts the tie group of value 0 (three rows): by id, then by row
    assert t(True, 1, 3)[0].tolist() == [[20, 2], [50, 5], [30, 0]]
    assert t(True, 1, 4)[0].tolist() == [[20, 2], [50, 5], [30, 0], [30, 3]]
    assert t(True, None, 3)[0].tolist() == [[20, 2], [50, 5], [30, 3]]
    assert t(True, None, 0)[0].shape == (0, 2) and t(True, None, 0)[2]["candidates"] == 7
    assert t(True, None, 5, 1, 0)[2] == {"rows_in": 8, "rows_valued": 7, "candidates": 0, "rows_out": 0}
    assert t(True, None, 5, 0, 0, "not_in")[0][:, 0].tolist() == [20, 50, 40, 10]
