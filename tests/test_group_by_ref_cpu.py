"""tests/group_by_ref.py against its own brute force on small tables, and the properties of the shared fixtures that
tests/test_gpu_group_by.py relies on.  No GPU."""
import numpy as np
import pytest

from tests import edge_filter_ref as F
from tests import extend_ref as X
from tests import group_by_ref as R
from tests import khop_aggregate_ref as K
from tests import triangles_ref as T


@pytest.fixture(scope="module")
def hard():
    vid, src, dst = T.hard_graph()
    g = T.TriangleGraph(vid, src, dst)
    es, ed, er, info = X.ext_table(g)
    light = int(es[(es != info["hub"]) & np.isin(es, g.vid)][0])
    S = np.array([info["hub"], info["z"], info["hub"], light, int(g.vid[3])], np.int64)
    return g, (es, ed, er, info), S


def ext_ids(vid, es, ed):
    """the vertex table of the joined table's CSR: the persons, then the other endpoints ascending"""
    rest = np.setdiff1d(np.concatenate([es, ed]), vid)
    return np.concatenate([np.asarray(vid, np.int64), rest])


def test_restatement_equals_brute_force_on_small_tables():
    rng = np.random.RandomState(5)
    key_ids = np.array([7, -3, 100, 42, np.iinfo(np.int64).min, 9], np.int64)
    weight_ids = np.array([42, 7, 1000, -3], np.int64)
    weights = np.array([np.iinfo(np.int64).max, np.iinfo(np.int64).min, 5, -np.iinfo(np.int64).max], np.int64)
    pool = np.concatenate([key_ids, [1000, 555]])
    for n in (0, 1, 5, 200):
        table = pool[rng.randint(0, pool.size, (n, 3))].reshape(n, 3)
        for kc in range(3):
            assert_same(R.group_by(table, kc, key_ids), R.group_by_brute(table, kc, key_ids))
            for wc in range(3):
                a = R.group_by(table, kc, key_ids, wc, weight_ids, weights)
                b = R.group_by_brute(table, kc, key_ids, wc, weight_ids, weights)
                assert_same(a, b)
                assert a[1]["rows_grouped"] == sum(a[0][1]) <= n
    level, st = R.group_by(np.zeros((0, 2), np.int64), 1, key_ids)
    assert st == {"rows_in": 0, "rows_grouped": 0, "groups": 0} and level[0].size == 0
    level, st = R.group_by(np.array([[7, 7]], np.int64), 0, np.empty(0, np.int64))  # a key table without vertices
    assert st == {"rows_in": 1, "rows_grouped": 0, "groups": 0}


def assert_same(a, b):
    assert K.same(a[0], b[0]) and a[1] == b[1]


def test_groups_ascend_by_position_in_the_key_table_and_unknown_keys_form_none():
    key_ids = np.array([30, 10, 20], np.int64)
    table = np.array([[10, 1], [30, 2], [99, 3], [10, 4], [20, 5]], np.int64)
    level, st = R.group_by(table, 0, key_ids)
    assert level[0].tolist() == [30, 10, 20] and level[1] == [1, 2, 1] and level[2] == [1, 2, 1]
    assert st == {"rows_in": 5, "rows_grouped": 4, "groups": 3}
    level, _ = R.group_by(table, 0, key_ids, 0, None, [1 << 62, -5, 7])  # weights by the key itself
    assert level[2] == [1 << 62, -10, 7]


def test_the_fixtures_have_what_the_gpu_tests_rely_on(hard):
    g, (es, ed, er, info), S = hard
    ids = ext_ids(g.vid, es, ed)
    assert X.NOT_A_PERSON in es and X.NOT_A_PERSON not in g.vid and -4242 in ed and -4242 not in g.vid
    w_person = R.hub_weights(g.vid, info["hub"])
    saw_big = saw_negative = False
    for hops in (1, 2):
        walks = g.vid[F.walks(g, S, hops)]
        # grouped by the extended-from column, the hub key arrives as a run of HUB_ROWS consecutive rows or more (from
        # column 0 always: the hub is a source; from the later columns wherever a walk comes back to it)
        longest = {}
        for fc in range(hops + 1):
            key = X.extend_rows(walks, es, ed, er, fc)[0][:, fc]
            change = np.flatnonzero(np.diff(key) != 0)
            runs = np.diff(np.concatenate([[-1], change, [key.size - 1]]))
            starts = np.concatenate([[0], change + 1])
            hub_runs = runs[key[starts] == info["hub"]]
            longest[fc] = int(hub_runs.max()) if hub_runs.size else 0
        assert longest[0] >= X.HUB_ROWS, longest
        rows, _, st = X.extend_rows(walks, es, ed, er, hops)
        # keys that are no vertex of the key's table occur: w against the persons
        level, stw = R.group_by(rows, hops + 1, g.vid)
        assert 0 < stw["rows_grouped"] < stw["rows_in"]
        # the weighted sums leave 64 bits and go negative
        level, _ = R.group_by(rows, hops, ids, hops, g.vid, w_person)
        saw_big |= any(abs(t) > 1 << 64 for t in level[2])
        saw_negative |= any(t < 0 for t in level[2])
        level, _ = R.group_by(rows, 0, g.vid, hops, g.vid, w_person)
        saw_big |= any(abs(t) > 1 << 64 for t in level[2])
    assert saw_big and saw_negative
    # the joined table read as a walk table of its own: its keys NOT_A_PERSON and the creator of -4242 give rows whose
    # cells are no person, in column 0 and in column 1
    own = np.stack([es, ed], axis=1)[np.isin(es, [X.NOT_A_PERSON, int(es[3])])]
    level, st = R.group_by(own, 0, g.vid)
    assert st["rows_in"] - st["rows_grouped"] == 3 and int(es[3]) in level[0]
    level, st = R.group_by(own, 1, ids)
    assert -4242 in level[0] and st["rows_grouped"] == st["rows_in"]
    # the source list has a duplicate and the hub
    assert np.unique(S).size < S.size and info["hub"] in S
    # message -> tag: 50 tags, some messages without any
    ts, td, tr = X.tag_table(ed)
    assert np.unique(td).size == 50 and np.setdiff1d(ed, ts).size > 0
