"""The CPU side of the full-width walk-row tests (tests/test_wide_rows_ref_cpu.py, tests/test_gpu_wide_rows.py): the small
shapes of tests/deep_graphs.py as triangles_ref.TriangleGraph, their source lists, their walk rows of 1 to 8 hops by
edge_filter_ref.walks and their second edge table, each computed once and never changed."""
import functools

import numpy as np

from tests import deep_graphs as D
from tests import edge_filter_ref as F
from tests import triangles_ref as T

# rows of the walk tables of deep_graphs.sources_of at 1..8 hops
ROWS = {
    "multigraph": [176, 298, 475, 724, 1155, 1935, 3299, 5504],
    "cycle_chords": [184, 197, 219, 240, 271, 334, 442, 640],
    "hub": [140, 3526, 7268, 9983, 9652, 8774, 7074, 5980],
    "dying": [96, 64, 29, 0, 0, 0, 0, 0],
}
KEPT_EDGE_ROWS = {"multigraph": 520, "cycle_chords": 542, "hub": 590, "dying": 297}


@functools.lru_cache(maxsize=None)
def world(name):
    """(vid, src, dst, TriangleGraph, source list) of a small shape"""
    vid, src, dst = D.shape(name)
    return vid, src, dst, T.TriangleGraph(vid, src, dst), D.sources_of(name, vid)


@functools.lru_cache(maxsize=None)
def walk_rows(name, hops: int) -> np.ndarray:
    """id rows [N, hops + 1] of the shape's source list, in the order of the expansion"""
    vid, _, _, g, S = world(name)
    rows = g.vid[F.walks(g, S, hops)].reshape(-1, hops + 1)
    rows.setflags(write=False)
    return rows


def column_pairs(hops: int):
    """every (from, to) over the columns {0, 1, hops - 1, hops}, from == to included"""
    cols = sorted({0, 1, hops - 1, hops})
    return [(a, b) for a in cols for b in cols]
