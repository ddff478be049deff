"""The numpy restatement of gg_result_distinct (tests/distinct_ref.py) against its python-loop twin, and the facts about
the shared tables (tests/distinct_tables.py) that the device tests rest on.  No GPU."""
import itertools

import numpy as np

from tests import distinct_ref as D
from tests.distinct_tables import hard_tables

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def test_restatement_equals_the_python_loop_on_random_tables():
    rng = np.random.RandomState(0xD157)
    for n, width, values in ((0, 3, 4), (1, 1, 1), (7, 2, 2), (200, 3, 3), (500, 4, 2), (300, 9, 2)):
        rows = rng.randint(0, values, size=(n, width)).astype(np.int64)
        for k in range(1, min(width, 3) + 1):
            for cols in itertools.permutations(range(width), k):
                if width > 4 and cols[0] > 1:
                    continue
                got = D.distinct_rows(rows, cols)
                assert same(got, D.distinct_rows_brute(rows, cols)), (n, width, cols)
                assert got[0].shape == (got[2]["rows_out"], k)
        assert same(D.distinct_rows(rows, range(width)), D.distinct_rows_brute(rows, range(width)))


def test_restatement_on_extreme_cells_and_orders():
    rows = np.array([[1, 2], [2, 1], [1, 2], [I64_MIN, -1], [-1, I64_MIN], [I64_MAX, 0], [I64_MIN, -1],
                     [1 << 32, 0], [0, 0], [0, 1 << 63 - 1], [0, 0]], np.int64)
    for cols in ([0], [1], [0, 1], [1, 0]):
        assert same(D.distinct_rows(rows, cols), D.distinct_rows_brute(rows, cols))
    out, at, st = D.distinct_rows(rows, [1, 0])
    assert at.tolist() == [0, 1, 3, 4, 5, 7, 8, 9] and out[0].tolist() == [2, 1] and st == {"rows_in": 11, "rows_out": 8}
    # the first occurrence is kept, in input order — not the sorted order np.unique works in
    out, at, _ = D.distinct_rows(np.array([[5], [3], [5], [4], [3]], np.int64), [0])
    assert out[:, 0].tolist() == [5, 3, 4] and at.tolist() == [0, 1, 3]


def test_the_shared_tables_hold_what_the_device_tests_need():
    hard = hard_tables()
    big, mid, small = (hard["rows"][k] for k in ("big", "mid", "small"))
    assert [t.shape for t in (big, mid, small)] == [(172_475, 4), (25_146, 4), (10, 3)]
    msgs, per_msg = np.unique(big[:, 3], return_counts=True)
    assert msgs.size == 2937 and per_msg.max() == 839
    assert D.distinct_rows(big, [3])[2]["rows_out"] == 2937
    # exact duplicate whole rows: the source list names the hub twice
    assert np.count_nonzero(hard["S"] == hard["ext"][3]["hub"]) == 2
    assert D.distinct_rows(big, range(4))[2]["rows_out"] < big.shape[0]
    # an end vertex of the 2-hop table reached over two different middle vertices
    two = hard["walks"][2]
    ends = D.distinct_rows(two, [0, 2])[2]["rows_out"]
    whole = D.distinct_rows(two, [0, 1, 2])[2]["rows_out"]
    assert ends < whole
    # the start column of every table has far fewer values than rows: at most the four distinct sources
    for t in (big, mid, small, hard["walks"][1], two):
        assert 1 <= D.distinct_rows(t, [0])[2]["rows_out"] <= 4 < t.shape[0]
