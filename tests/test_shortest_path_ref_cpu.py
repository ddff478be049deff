"""The numpy restatement of the shortest-path relation (tests/shortest_path_ref.py) against the oracle's BFS, the
compiled reference's friends_shortest goldens and the edge table itself; and the C-ABI's three path entry points are
declared and exported.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import duckdb_pgq_amd.gg as ggmod
from tests import shortest_path_ref as ref
from tests.test_golden import NAMES, bfs_cases, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["gg_bfs64_paths", "gg_bfs64_paths_rows", "gg_bfs64_paths_fetch"]


def test_reverse_rows_are_ascending_by_source_then_position():
    off = np.array([0, 3, 4, 6])
    nbr = np.array([1, 2, 1, 1, 0, 1])
    roff, rnbr = ref.reverse_rows(off, nbr)
    assert roff.tolist() == [0, 1, 5, 6]
    assert rnbr.tolist() == [2, 0, 0, 1, 2, 0]


def test_parallel_edges_self_loops_and_the_bound():
    # 0 -> 1 twice (rowids 7, 5 in CSR order), 1 -> 1, 1 -> 2, 0 -> 2 absent; 3 isolated
    off, nbr, eid, vid = np.array([0, 2, 4, 4, 4]), np.array([1, 1, 1, 2]), np.array([7, 5, 9, 11]), np.array([10, 11, 12, 13])
    pair, step, vtx, edge = ref.shortest_paths(off, nbr, eid, vid, [10, 10, 11, 10, 99, 10], [12, 10, 11, 13, 12, 12], 2)
    assert pair.tolist() == [0, 0, 0, 1, 2, 5, 5, 5]
    assert step.tolist() == [0, 1, 2, 0, 0, 0, 1, 2]
    assert vtx.tolist() == [10, 11, 12, 10, 11, 10, 11, 12]
    assert edge.tolist() == [-1, 7, 11, -1, -1, -1, 7, 11]  # the first CSR entry wins among parallel edges
    assert ref.shortest_paths(off, nbr, eid, vid, [10], [12], 1)[0].size == 0  # cut by max_hops


@pytest.mark.parametrize("name", NAMES)
def test_paths_on_the_goldens(orc, name):
    g = load(name)
    vid, src, dst = g["vid"], g["src"], g["dst"]
    rc, c = orc.csr_build(vid, src, dst)
    assert rc == 0
    off, nbr, eid, v2 = c.arrays()
    cases = 0
    for sources, max_hops, rel in bfs_cases(g):
        dense = c.lookup(sources)
        o_dist, _ = c.bfs64(dense, max_hops)
        lane_of = {int(s): i for i, s in enumerate(sources)}
        rows = rel  # every golden friends_shortest row (source, friend, hopCount) is a pair
        pair, step, vtx, edge = ref.shortest_paths(off, nbr, eid, v2, rows[:, 0], rows[:, 1], max_hops)
        starts = np.flatnonzero(step == 0)
        assert np.array_equal(pair[starts], np.arange(rows.shape[0]))  # every golden pair has a path
        ends = np.append(starts[1:], pair.size) - 1
        dense_of = {int(v): i for i, v in enumerate(v2)}
        for p, (a, b) in enumerate(zip(starts, ends)):
            s_id, t_id, hops = (int(x) for x in rows[p])
            assert step[a:b + 1].tolist() == list(range(b - a + 1))
            assert b - a == hops == int(o_dist[lane_of[s_id], dense_of[t_id]])
            assert vtx[a] == s_id and vtx[b] == t_id and edge[a] == -1
            e = edge[a + 1:b + 1]  # no rowids were passed: the rowid is the row's position in the edge table
            assert np.array_equal(src[e], vtx[a:b]) and np.array_equal(dst[e], vtx[a + 1:b + 1])
        cases += 1
    assert cases
    c.close()


def test_header_declares_and_library_exports_the_path_entry_points():
    text = open(os.path.join(ROOT, "include", "gg.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", text))
    lib = ctypes.CDLL(ggmod.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in ggmod.SYMBOLS
