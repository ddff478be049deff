"""gg_bfs64_all_paths and its three readers are declared, bound and exported, and refuse NULL arguments before they touch
a device.  No GPU."""
import ctypes as C
import os
import re

import duckdb_pgq_amd.gg as ggmod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["gg_bfs64_all_paths", "gg_bfs64_all_paths_rows", "gg_bfs64_all_paths_fetch_pairs",
                "gg_bfs64_all_paths_fetch"]
GG_ERR_INVALID_ARG = -1


def test_header_declares_and_library_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "gg.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", text))
    lib = C.CDLL(ggmod.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in ggmod.SYMBOLS


def test_stats_struct_matches_the_header():
    text = open(os.path.join(ROOT, "include", "gg.h")).read()
    body = re.search(r"typedef struct gg_all_paths_stats \{(.*?)\} gg_all_paths_stats;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(\w+)\s*;", body)
    assert fields == [f[0] for f in ggmod.AllPathsStats._fields_]
    assert C.sizeof(ggmod.AllPathsStats) == C.sizeof(ggmod.BfsStats) + 6 * 8


def test_null_arguments_are_refused_without_a_device():
    lib = ggmod.load_library()
    st, res, n, got = ggmod.AllPathsStats(), C.c_void_p(), C.c_uint64(), C.c_uint32()
    assert lib.gg_bfs64_all_paths(None, None, None, 0, -1, None, None, 0, 0, 1, 1, C.byref(st), C.byref(res)) == GG_ERR_INVALID_ARG
    assert res.value is None
    assert lib.gg_bfs64_all_paths(None, None, None, 0, -1, None, None, 0, 0, 0, 0, None, None) == GG_ERR_INVALID_ARG
    assert lib.gg_bfs64_all_paths_rows(None, 0, C.byref(n)) == GG_ERR_INVALID_ARG
    assert lib.gg_bfs64_all_paths_fetch_pairs(None, 0, 1, None, None, None, None, C.byref(got)) == GG_ERR_INVALID_ARG
    assert lib.gg_bfs64_all_paths_fetch(None, 0, 1, None, None, None, None, None, C.byref(got)) == GG_ERR_INVALID_ARG
