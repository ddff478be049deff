"""tests/cheapest_paths_ref.py, the restatement of gg_cheapest64_paths, against a second and independent statement of the
same relation on graphs of at most 7 vertices: every walk of at most V - 1 kept rows from the source is enumerated, those
to the target with the least cost and then the fewest edges are kept, and one is chosen from the target backwards by
(dense index of the row's source, append order) of the last row, then of the row before it, and so on.  Then the bounded
counter-example of include/gg.h and the relation's invariants on a few hundred random graphs.  No GPU."""
import numpy as np
import pytest

from tests import cheapest_paths_ref as PR
from tests import cheapest_ref as CR


def random_graph(rng, V, rows, weights=(0, 0, 1, 2, 5), dangling=True):
    vid = (rng.permutation(V) * 5 + 2).astype(np.int64)
    pool = np.concatenate([vid, [-9]]) if dangling else vid  # -9 is no vertex: such rows are dropped
    src, dst = pool[rng.randint(0, pool.size, rows)], pool[rng.randint(0, pool.size, rows)]
    wt = np.array(weights, np.int64)[rng.randint(0, len(weights), rows)]
    return vid, src, dst, wt


def enumerated(g, s, t):
    """the chosen walk s -> t as kept-row indices in walk order (None: t is not reached from s; []: s == t)"""
    out_rows = [[] for _ in range(g.V)]
    for k in range(g.E):
        out_rows[g.su[k]].append(k)
    found = []  # (cost, edges, key from the target backwards, rows)

    def walk(x, rows, cost):
        if x == t:
            found.append((cost, len(rows), [(g.su[k], k) for k in reversed(rows)], list(rows)))
        if len(rows) == g.V - 1:
            return
        for k in out_rows[x]:
            rows.append(k)
            walk(g.dv[k], rows, cost + g.wk[k])
            rows.pop()

    walk(s, [], 0)
    return min(found)[3] if found else None


@pytest.mark.parametrize("seed", range(40))
def test_the_restatement_equals_the_enumeration(seed):
    rng = np.random.RandomState(seed)
    V = int(rng.randint(2, 8))
    vid, src, dst, wt = random_graph(rng, V, int(rng.randint(1, 13)))
    g = CR.WeightedGraph(vid, src, dst, wt)
    S = vid[:min(V, 3)]
    lanes = np.repeat(np.arange(S.size), V)
    targets = np.tile(vid, S.size)
    got = PR.paths(g, S, lanes, targets)
    pair, step, vertex, edge, cost = got["rows"]
    at = 0
    listed = dict(zip(got["pairs"][0].tolist(), zip(got["pairs"][1], got["pairs"][2].tolist(), got["pairs"][3].tolist())))
    for p, (lane, t) in enumerate(zip(lanes.tolist(), targets.tolist())):
        rows = enumerated(g, g.index[int(S[lane])], g.index[int(t)])
        if rows is None:
            assert p not in listed
            continue
        walk_cost = sum(g.wk[k] for k in rows)
        assert listed[p] == (walk_cost, len(rows), 1)
        n = len(rows) + 1
        assert pair[at:at + n].tolist() == [p] * n and step[at:at + n].tolist() == list(range(n))
        assert vertex[at:at + n].tolist() == [int(S[lane])] + [int(g.vid[g.dv[k]]) for k in rows]
        assert edge[at:at + n].tolist() == [-1] + [g.kept[k] for k in rows]  # the append position of the row
        assert cost[at:at + n] == [sum(g.wk[k] for k in rows[:i]) for i in range(n)]
        at += n
    assert at == pair.size == got["n_rows"] and got["pairs_saturated"] == 0


def test_the_bounded_state_of_the_counter_example_cannot_be_traced():
    vid = np.arange(5, dtype=np.int64)
    src, dst, wt = np.array([0, 0, 1, 2, 3]), np.array([3, 1, 2, 3, 4]), np.array([10, 1, 1, 1, 1])
    g = CR.WeightedGraph(vid, src, dst, wt)
    bounded = CR.cheapest(g, [0], 3)
    assert PR.cells_of(bounded)[(0, 4)] == (11, 2)  # derived from cost_1(3) = 10, which round 3 overwrote with 3
    with pytest.raises(PR.LostTrace):
        PR.paths(g, [0], [0], [4], max_hops=3)
    got = PR.paths(g, [0], [0], [4])  # the fixpoint: the walk of 4 rows and cost 4
    assert PR.same_rows(got["rows"], ([0] * 5, [0, 1, 2, 3, 4], [0, 1, 2, 3, 4], [-1, 1, 2, 3, 4], [0, 1, 2, 3, 4]))
    assert PR.same_rows(got["pairs"], ([0], [4], [4], [1])) and got["entries_scanned"] == 1 + 2 + 1 + 1


def test_a_saturated_pair_is_listed_and_not_traced():
    vid = np.array([1, 2, 3], np.int64)
    g = CR.WeightedGraph(vid, [1, 2], [2, 3], [CR.INT64_MAX - 1, 5])
    got = PR.paths(g, [1], [0, 0, 0], [3, 2, 1])
    assert PR.same_rows(got["pairs"], ([0, 1, 2], [CR.INT64_MAX, CR.INT64_MAX - 1, 0], [2, 1, 0], [0, 1, 1]))
    assert PR.same_rows(got["rows"], ([1, 1, 2], [0, 1, 0], [1, 2, 1], [-1, 0, -1], [0, CR.INT64_MAX - 1, 0]))
    assert got["pairs_saturated"] == 1 and got["pairs_reached"] == 3


def test_the_invariants_on_random_graphs():
    traced = 0
    for seed in range(300):
        rng = np.random.RandomState(1000 + seed)
        V = int(rng.randint(2, 25))
        vid, src, dst, wt = random_graph(rng, V, int(rng.randint(1, 4 * V)))
        rowid = rng.permutation(src.size).astype(np.int64) + 100
        g = CR.WeightedGraph(vid, src, dst, wt)
        S = vid[:min(V, 4)]
        lanes, targets = np.repeat(np.arange(S.size), V), np.tile(vid, S.size)
        state = CR.cheapest(g, S)
        got = PR.paths(g, S, lanes, targets, rowid, state=state)
        cells = PR.cells_of(state)
        pair, step, vertex, edge, cost = got["rows"]
        weight_of = dict(zip(rowid.tolist(), zip(src.tolist(), dst.tolist(), wt.tolist())))
        assert got["pairs_reached"] == sum((int(l), int(t)) in cells for l, t in zip(lanes, targets))
        start = 0
        for p, c, h, was_traced in zip(*[list(col) for col in got["pairs"]]):
            assert was_traced == 1 and (c, h) == cells[(int(lanes[p]), int(targets[p]))]
            n = h + 1  # rows equal hops + 1
            assert pair[start:start + n].tolist() == [p] * n and step[start:start + n].tolist() == list(range(n))
            assert vertex[start] == S[lanes[p]] and vertex[start + n - 1] == targets[p]
            assert cost[start] == 0 and edge[start] == -1 and cost[start + n - 1] == c  # the last cost is cheapest()'s
            for i in range(start + 1, start + n):
                a, b, w = weight_of[int(edge[i])]  # each step's edge row joins the two vertices and weighs the difference
                assert (a, b) == (vertex[i - 1], vertex[i]) and cost[i] - cost[i - 1] == w >= 0
            start += n
            traced += 1
        assert start == pair.size
    assert traced > 3000
