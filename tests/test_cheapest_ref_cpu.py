"""tests/cheapest_ref.py against itself: the rounds at the fixpoint equal an independent heap Dijkstra, unit weights turn
cost and hops into the BFS distances of tests/bfs_levels_ref.py, and tiny cases worked out by hand.  No GPU."""
import numpy as np

from tests import bfs_levels_ref as B
from tests import cheapest_ref as R
from tests import triangles_ref as T

INT64_MAX = R.INT64_MAX


def rows_of(res):
    return list(zip(res["rows"][0].tolist(), res["rows"][1].tolist(), res["rows"][2], res["rows"][3]))


def small():
    vid, src, dst = T.hard_graph(V=300, rows=3000, seed=0x51, hub_fan=120)
    return vid, src, dst


def test_rounds_at_the_fixpoint_equal_dijkstra():
    vid, src, dst = small()
    g = R.WeightedGraph(vid, src, dst, R.hashed_weights(src.size))
    S = np.concatenate([vid[:20], [-123456789], vid[5:6]])
    res = R.cheapest(g, S)
    got = {}
    for i, v, c, h in rows_of(res):
        got.setdefault(i, {})[g.index[v]] = (c, h)
    for i, s in enumerate(S.tolist()):
        assert got.get(i, {}) == R.dijkstra(g, s), i
    assert res["reached_pairs"] == len(res["rows"][2]) > 20 * 250
    assert res["entries_pulled"] == res["rounds"] * g.E and 0 < res["rows_gathered"] < res["entries_pulled"]
    assert res["cells_lowered"] >= res["reached_pairs"] - 21  # every reached cell but a seed was lowered at least once


def test_unit_weights_are_the_bfs_distances():
    vid, src, dst = small()
    g = R.WeightedGraph(vid, src, dst, np.ones(src.size, np.int64))
    S = vid[:64]
    dense = lambda ids: np.array([g.index.get(int(x), -1) for x in np.asarray(ids).tolist()], np.int64)
    for max_hops in (-1, 0, 1, 3):
        res = R.cheapest(g, S, max_hops)
        lv = B.bfs_levels(g.V, dense(src), dense(dst), dense(S).tolist(), max_hops)
        want = [(lane, int(vid[v]), int(lv.dist[lane, v]), int(lv.dist[lane, v]))
                for lane in range(64) for v in range(g.V) if lv.dist[lane, v] >= 0]
        assert rows_of(res) == want
        # a round per BFS level, the last empty one included
        assert res["rounds"] == lv.levels and res["cells_lowered"] == sum(lv.reached[1:])


def tiny(edges, vid=(1, 2, 3, 4)):
    src, dst, w = zip(*edges) if edges else ((), (), ())
    return R.WeightedGraph(np.array(vid, np.int64), np.array(src, np.int64), np.array(dst, np.int64), list(w))


def test_the_bound_changes_the_answer():
    g = tiny([(1, 3, 10), (1, 2, 1), (2, 3, 2)])  # a direct edge of weight 10 beside a 2-edge detour of weight 3
    assert rows_of(R.cheapest(g, [1], 1)) == [(0, 1, 0, 0), (0, 2, 1, 1), (0, 3, 10, 1)]
    assert rows_of(R.cheapest(g, [1], 2)) == [(0, 1, 0, 0), (0, 2, 1, 1), (0, 3, 3, 2)]
    res = R.cheapest(g, [1], -1)
    assert rows_of(res) == [(0, 1, 0, 0), (0, 2, 1, 1), (0, 3, 3, 2)]  # vertex 4 is unreachable: no row
    assert (res["rounds"], res["cells_lowered"], res["reached_pairs"], res["entries_pulled"]) == (3, 3, 3, 9)
    assert res["rows_gathered"] == 2 + 1 + 0  # round 1: the rows out of 1; round 2: out of 2 and 3; round 3: out of 3
    assert rows_of(R.cheapest(g, [1], 0)) == [(0, 1, 0, 0)]


def test_parallel_rows_self_loops_and_zero_weights():
    g = tiny([(1, 2, 7), (1, 2, 4), (1, 2, 9), (2, 2, 0), (1, 1, 3)])
    assert rows_of(R.cheapest(g, [1])) == [(0, 1, 0, 0), (0, 2, 4, 1)]
    # a zero-weight 2-cycle 2 <-> 3 behind 1, and a zero-weight tie: 1 -> 4 directly (5) and through 2 (5 + 0)
    g = tiny([(1, 2, 5), (2, 3, 0), (3, 2, 0), (1, 4, 5), (2, 4, 0)])
    res = R.cheapest(g, [1, 3])
    assert rows_of(res) == [(0, 1, 0, 0), (0, 2, 5, 1), (0, 3, 5, 2), (0, 4, 5, 1),
                            (1, 2, 0, 1), (1, 3, 0, 0), (1, 4, 0, 2)]
    assert res["rounds"] == 3  # it terminates: a tie lowers nothing


def test_saturation_and_targets_and_batches():
    g = tiny([(1, 2, 1 << 62), (2, 3, 1 << 62), (3, 4, 1 << 62)])
    assert rows_of(R.cheapest(g, [1])) == [(0, 1, 0, 0), (0, 2, 1 << 62, 1), (0, 3, INT64_MAX, 2), (0, 4, INT64_MAX, 3)]
    g = tiny([(1, 2, INT64_MAX), (2, 3, 1)])
    assert rows_of(R.cheapest(g, [1])) == [(0, 1, 0, 0), (0, 2, INT64_MAX, 1), (0, 3, INT64_MAX, 2)]
    g = tiny([(1, 2, 1), (2, 3, 1), (9, 1, 1), (3, 8, 1)])  # two dangling rows
    assert g.E == 2 and g.kept == [0, 1] and g.entry_weights().tolist() == [1, 1]
    assert rows_of(R.cheapest(g, [1, 1, 77], -1, [3, 3, 99, 1])) == [(0, 1, 0, 0), (0, 3, 2, 2), (1, 1, 0, 0), (1, 3, 2, 2)]
    assert rows_of(R.cheapest(g, [1], -1, [])) == []
    many = R.cheapest(g, [1] * 65 + [2])  # two batches: the source index runs on, the statistics add
    assert many["rows"][0].tolist()[-3:] == [64, 65, 65] and many["rounds"] == 3 + 3
    assert R.id_rows(R.cheapest(g, [2, 1])["rows"], [2, 1])[0] == (1, 1, 0, 0)
    empty = tiny([])
    assert rows_of(R.cheapest(empty, [2])) == [(0, 2, 0, 0)] and R.cheapest(empty, [2])["rounds"] == 0
