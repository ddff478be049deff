"""gg_edge_weights_create / _destroy, gg_cheapest64 and its two readers and gg_debug_cheapest are declared, bound and
exported, gg_cheapest_stats matches its ctypes mirror, and NULL arguments are refused before a device is touched.  No GPU."""
import ctypes as C
import os
import re

import duckdb_pgq_amd.gg as ggmod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["gg_edge_weights_create", "gg_edge_weights_destroy", "gg_cheapest64", "gg_cheapest64_rows",
                "gg_cheapest64_fetch", "gg_debug_cheapest"]
GG_ERR_INVALID_ARG = -1


def test_header_declares_and_library_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "gg.h")).read()
    assert "#define GG_WEIGHTS_BY_ROWID 0" in text and "#define GG_WEIGHTS_BY_ENTRY 1" in text
    assert ggmod.WEIGHTS_BY == {"rowid": 0, "entry": 1}
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(gg_[a-z0-9_]+)\s*\(", text))
    lib = C.CDLL(ggmod.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in ggmod.SYMBOLS
    for method in ("edge_weights", "cheapest64", "cheapest_path_lengths", "debug_cheapest"):
        assert callable(getattr(ggmod.GG, method))


def test_stats_struct_matches_the_header():
    text = open(os.path.join(ROOT, "include", "gg.h")).read()
    body = re.search(r"typedef struct gg_cheapest_stats \{(.*?)\} gg_cheapest_stats;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(\w+)\s*;", body)
    assert fields == [f[0] for f in ggmod.CheapestStats._fields_] == [
        "rounds", "reached_pairs", "cells_lowered", "entries_pulled", "rows_gathered"]
    assert C.sizeof(ggmod.CheapestStats) == 40  # five u64
    assert ggmod.CheapestStats.rows_gathered.offset == 32


def test_null_arguments_are_refused_without_a_device():
    lib = ggmod.load_library()
    one = (C.c_int64 * 1)(7)
    w = C.c_void_p(1)
    assert lib.gg_edge_weights_create(None, None, one, 1, 0, C.byref(w)) == GG_ERR_INVALID_ARG
    assert w.value is None  # the out pointer is cleared first
    assert lib.gg_edge_weights_create(None, None, None, 0, 0, None) == GG_ERR_INVALID_ARG
    lib.gg_edge_weights_destroy(None)  # a NULL is ignored
    st, res = ggmod.CheapestStats(), C.c_void_p(1)
    st.rounds = 9
    assert lib.gg_cheapest64(None, None, None, one, 1, -1, None, 0, C.byref(st), C.byref(res)) == GG_ERR_INVALID_ARG
    assert res.value is None and st.rounds == 0  # both outputs are cleared first
    assert lib.gg_cheapest64(None, None, None, None, 1, -1, None, 0, None, None) == GG_ERR_INVALID_ARG
    n, got = C.c_uint64(5), C.c_uint32(5)
    assert lib.gg_cheapest64_rows(None, C.byref(n)) == GG_ERR_INVALID_ARG
    assert lib.gg_cheapest64_fetch(None, 0, 8, None, None, None, None, C.byref(got)) == GG_ERR_INVALID_ARG
    assert lib.gg_debug_cheapest(None, 0, 0) == GG_ERR_INVALID_ARG
