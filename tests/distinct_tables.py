"""The tables the DISTINCT tests share, built exactly as tests/test_gpu_value_rows.py's `hard` fixture builds them (the
walks of tests/test_gpu_extend.py's source list over triangles_ref.hard_graph(), extended over extend_ref.ext_table), once
per process and read-only.  The keys tests/test_gpu_value_rows.World reads are all here, so a World can be made of it."""
import functools

import numpy as np

from tests import edge_filter_ref as F
from tests import extend_ref as X
from tests import triangles_ref as T

SHAPE = {"big": (2, 0), "mid": (2, 2), "small": (1, 1)}  # name -> (hops of the walk table, from_col)


@functools.lru_cache(maxsize=None)
def hard_tables() -> dict:
    vid, src, dst = T.hard_graph()
    g = T.TriangleGraph(vid, src, dst)
    es, ed, er, info = X.ext_table(g)
    light = int(es[(es != info["hub"]) & np.isin(es, g.vid)][0])
    S = np.array([info["hub"], info["z"], info["hub"], light, int(g.vid[3])], np.int64)
    walks = {h: g.vid[F.walks(g, S, h)] for h in (1, 2)}
    rows = {name: X.extend_rows(walks[h], es, ed, er, fc)[0] for name, (h, fc) in SHAPE.items()}
    for a in (vid, src, dst, es, ed, er, S, *walks.values(), *rows.values()):
        a.setflags(write=False)
    return {"vid": vid, "src": src, "dst": dst, "g": g, "ext": (es, ed, er, info), "S": S, "walks": walks, "shape": SHAPE,
            "rows": rows}
