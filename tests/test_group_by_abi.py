"""gg_result_group_by and gg_debug_group are declared, bound and exported, gg_group_stats matches its ctypes mirror, and NULL
arguments are refused before a device is touched.  No GPU."""
import ctypes as C
import os
import re

import duckdb_pgq_amd.gg as ggmod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["gg_result_group_by", "gg_debug_group"]
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
    body = re.search(r"typedef struct gg_group_stats \{(.*?)\} gg_group_stats;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(\w+)\s*;", body)
    assert fields == [f[0] for f in ggmod.GroupStats._fields_] == ["rows_in", "rows_grouped", "groups", "route"]
    assert C.sizeof(ggmod.GroupStats) == 32  # three u64, a u32 and its padding
    assert ggmod.GroupStats.route.offset == 24


def test_null_arguments_are_refused_without_a_device():
    lib = ggmod.load_library()
    st, res = ggmod.GroupStats(), C.c_void_p(1)
    assert lib.gg_result_group_by(None, None, 1, 0, None, -1, None, None, C.byref(st), C.byref(res)) == GG_ERR_INVALID_ARG
    assert res.value is None  # the out pointer is cleared first
    assert lib.gg_result_group_by(None, None, 1, 0, None, -1, None, None, None, None) == GG_ERR_INVALID_ARG
    assert lib.gg_debug_group(None, 0, 0) == GG_ERR_INVALID_ARG
