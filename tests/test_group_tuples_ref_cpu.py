"""The numpy restatement of gg_result_group_tuples (tests/group_tuples_ref.py) against its python-loop twin on the tables
the device tests use (tests/distinct_tables.hard_tables()), and the facts about the restatement those tests lean on.  No GPU."""
import numpy as np
import pytest

from tests import distinct_ref as D
from tests import group_tuples_ref as T
from tests import value_rows_ref as R
from tests.distinct_tables import hard_tables

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def column_sets(width: int):
    sets = [[c] for c in range(width)] + [[0, width - 1], [width - 1, 0], list(range(width))]
    return [s for i, s in enumerate(sets) if s not in sets[:i]]


def extreme_values(ids) -> np.ndarray:
    """a value per id: mostly small, of both signs, with the extremes mixed in"""
    ids = np.asarray(ids, np.int64)
    v = (ids % 2001 - 1000).astype(np.int64)
    v[::5] = I64_MAX
    v[1::7] = I64_MIN
    v[2::11] = -1
    return v


@pytest.mark.parametrize("name", ["small", "mid", "walk1", "walk2"])
def test_restatement_equals_the_dict_loop(name):
    hard = hard_tables()
    rows = hard["walks"][int(name[-1])] if name.startswith("walk") else hard["rows"][name]
    ids = np.unique(np.concatenate([hard["vid"], hard["ext"][0], hard["ext"][1]]))
    values = extreme_values(ids)
    valid = R.pack_valid(np.arange(ids.size) % 3 != 0)
    for cols in column_sets(rows.shape[1]):
        a, ast = T.group_tuples(rows, cols)
        b, bst = T.group_tuples_brute(rows, cols)
        assert ast == bst and T.same(a, b)
        assert not a["valued"].any() and not any(a["sum"]) and not a["min"].any() and not a["max"].any()
        assert np.array_equal(a["keys"], D.distinct_rows(rows, cols)[0])  # DISTINCT's rows in DISTINCT's order
        assert int(a["rows"].sum()) == rows.shape[0]
        for vc in (0, rows.shape[1] - 1):
            for bits in (None, valid):
                a, ast = T.group_tuples(rows, cols, vc, ids, values, bits)
                b, bst = T.group_tuples_brute(rows, cols, vc, ids, values, bits)
                assert ast == bst and T.same(a, b)
                assert ast["rows_valued"] == int(a["valued"].sum()) == int(R.row_values(rows, vc, ids, values, bits)[0].sum())


def test_sums_wrap_mod_2_128_and_split_in_twos_complement():
    assert T.split128(0) == (0, 0) and T.split128(-1) == ((1 << 64) - 1, -1)
    assert T.split128(3 * I64_MAX) == ((3 * I64_MAX) & ((1 << 64) - 1), 1)
    assert T.split128(I64_MIN - 1) == (I64_MAX, -1)
    assert T.split128(1 << 127) == (0, I64_MIN) and T.split128((1 << 128) + 5) == (5, 0)
    rows = np.array([[1, 9], [1, 9], [1, 9], [2, 8], [2, 9], [3, 7]], np.int64)
    ids, values = np.array([9, 8], np.int64), np.array([I64_MAX, I64_MIN], np.int64)
    out, st = T.group_tuples(rows, [0], 1, ids, values)
    assert out["keys"][:, 0].tolist() == [1, 2, 3] and out["rows"].tolist() == [3, 2, 1] and out["valued"].tolist() == [3, 2, 0]
    assert [int(s) for s in out["sum"]] == [3 * I64_MAX, -1, 0]
    assert out["lo"].tolist() == [(3 * I64_MAX) & ((1 << 64) - 1), (1 << 64) - 1, 0] and out["hi"].tolist() == [1, -1, 0]
    assert out["min"].tolist() == [I64_MAX, I64_MIN, 0] and out["max"].tolist() == [I64_MAX, I64_MAX, 0]
    assert st == {"rows_in": 6, "rows_valued": 5, "groups": 3}


def test_empty_input_and_column_order():
    out, st = T.group_tuples(np.empty((0, 3), np.int64), [2, 0])
    assert out["keys"].shape == (0, 2) and st == {"rows_in": 0, "rows_valued": 0, "groups": 0}
    rows = np.array([[1, 2], [2, 1], [1, 2]], np.int64)
    a, _ = T.group_tuples(rows, [0, 1])
    b, _ = T.group_tuples(rows, [1, 0])
    assert a["keys"].tolist() == [[1, 2], [2, 1]] and b["keys"].tolist() == [[2, 1], [1, 2]]  # (a, b) is not (b, a)
    assert a["rows"].tolist() == b["rows"].tolist() == [2, 1]
