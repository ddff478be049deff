"""gg_result_filter_value, gg_result_top_rows and gg_debug_value_top are declared, bound and exported, their stats structs
match the ctypes mirrors, and NULL arguments are refused before a device is touched.  No GPU."""
import ctypes as C
import os
import re

import duckdb_pgq_amd.gg as ggmod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["gg_result_filter_value", "gg_result_top_rows", "gg_debug_value_top"]
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
    assert re.search(r"#define GG_VALUE_IN\s+0\b", text) and re.search(r"#define GG_VALUE_NOT_IN\s+1\b", text)
    assert ggmod.VALUE_MODES == {"in": 0, "not_in": 1}


def header_fields(struct: str):
    text = open(os.path.join(ROOT, "include", "gg.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]


def test_stats_structs_match_the_header():
    assert header_fields("gg_value_filter_stats") == [f[0] for f in ggmod.ValueFilterStats._fields_] == [
        "rows_in", "rows_valued", "rows_out"]
    assert C.sizeof(ggmod.ValueFilterStats) == 24
    assert header_fields("gg_value_top_stats") == [f[0] for f in ggmod.ValueTopStats._fields_] == [
        "rows_in", "rows_valued", "candidates", "rows_out", "select_passes", "sort_route"]
    assert C.sizeof(ggmod.ValueTopStats) == 40  # four u64 and two u32
    assert ggmod.ValueTopStats.select_passes.offset == 32 and ggmod.ValueTopStats.sort_route.offset == 36


def test_null_arguments_are_refused_without_a_device():
    lib = ggmod.load_library()
    fs, ts = ggmod.ValueFilterStats(), ggmod.ValueTopStats()
    res = C.c_void_p(1)
    assert lib.gg_result_filter_value(None, None, 1, 0, None, None, None, 0, 0, 0, 1, C.byref(fs), C.byref(res)) == GG_ERR_INVALID_ARG
    assert res.value is None  # the out pointer is cleared first
    assert lib.gg_result_filter_value(None, None, 1, 0, None, None, None, 0, 0, 0, 0, None, None) == GG_ERR_INVALID_ARG
    res = C.c_void_p(1)
    assert lib.gg_result_top_rows(None, None, 1, 0, None, None, None, 0, 0, 0, 1, -1, 5, C.byref(ts), C.byref(res)) == GG_ERR_INVALID_ARG
    assert res.value is None
    assert lib.gg_result_top_rows(None, None, 1, 0, None, None, None, 0, 0, 0, 1, -1, 5, None, None) == GG_ERR_INVALID_ARG
    assert lib.gg_debug_value_top(None, 0, 0) == GG_ERR_INVALID_ARG
