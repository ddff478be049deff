"""gg_result_group_tuples, its two readers and gg_debug_group_tuples are declared, bound and exported,
gg_group_tuples_stats matches its ctypes mirror, and NULL arguments are refused before a device is touched.  No GPU."""
import ctypes as C
import os
import re

import duckdb_pgq_amd.gg as ggmod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["gg_result_group_tuples", "gg_tuple_groups_rows", "gg_tuple_groups_fetch", "gg_debug_group_tuples"]
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


def header_fields(struct: str):
    text = open(os.path.join(ROOT, "include", "gg.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]


def test_stats_struct_matches_the_header():
    fields = ggmod.GroupTuplesStats._fields_
    assert header_fields("gg_group_tuples_stats") == [f[0] for f in fields] == [
        "rows_in", "rows_valued", "groups", "slots", "probe_steps", "route"]
    assert [f[1] for f in fields] == [C.c_uint64] * 5 + [C.c_uint32]  # five u64 and one u32
    assert C.sizeof(ggmod.GroupTuplesStats) == 48


def test_null_arguments_are_refused_without_a_device():
    lib = ggmod.load_library()
    st = ggmod.GroupTuplesStats()
    cols = (C.c_int * 1)(0)
    res = C.c_void_p(1)
    assert lib.gg_result_group_tuples(None, None, 1, cols, 1, -1, None, None, None, C.byref(st), C.byref(res)) == GG_ERR_INVALID_ARG
    assert res.value is None  # the out pointer is cleared first
    assert lib.gg_result_group_tuples(None, None, 1, None, 1, -1, None, None, None, None, None) == GG_ERR_INVALID_ARG
    n, k, got = C.c_uint64(), C.c_int(), C.c_uint32()
    assert lib.gg_tuple_groups_rows(None, C.byref(n), C.byref(k)) == GG_ERR_INVALID_ARG
    assert lib.gg_tuple_groups_fetch(None, 0, 8, None, None, None, None, None, None, None, C.byref(got)) == GG_ERR_INVALID_ARG
    assert lib.gg_debug_group_tuples(None, 0, 0) == GG_ERR_INVALID_ARG
