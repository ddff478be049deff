"""gg_cheapest64_paths and its three readers are declared, bound and exported, with the two python calls above them;
gg_cheapest_paths_stats matches its ctypes mirror; and NULL arguments are refused before a device is touched, outputs
cleared.  No GPU."""
import ctypes as C
import os
import re

import duckdb_pgq_amd.gg as ggmod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["gg_cheapest64_paths", "gg_cheapest64_paths_rows", "gg_cheapest64_paths_fetch_pairs",
                "gg_cheapest64_paths_fetch"]
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
    bound = ggmod.load_library()
    assert len(bound.gg_cheapest64_paths.argtypes) == 11 and len(bound.gg_cheapest64_paths_rows.argtypes) == 3
    assert len(bound.gg_cheapest64_paths_fetch_pairs.argtypes) == 8 and len(bound.gg_cheapest64_paths_fetch.argtypes) == 9
    for method in ("cheapest64_paths", "cheapest_paths"):
        assert callable(getattr(ggmod.GG, method))


def test_stats_struct_matches_the_header():
    text = open(os.path.join(ROOT, "include", "gg.h")).read()
    body = re.search(r"typedef struct gg_cheapest_paths_stats \{(.*?)\} gg_cheapest_paths_stats;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(\w+)\s*;", body)
    assert fields == [f[0] for f in ggmod.CheapestPathsStats._fields_] == [
        "search", "pairs_reached", "pairs_saturated", "rows", "entries_scanned"]
    assert "gg_cheapest_stats search" in body and ggmod.CheapestPathsStats._fields_[0][1] is ggmod.CheapestStats
    assert C.sizeof(ggmod.CheapestPathsStats) == 72  # nine u64
    assert ggmod.CheapestPathsStats.pairs_reached.offset == 40 and ggmod.CheapestPathsStats.entries_scanned.offset == 64


def test_null_arguments_are_refused_without_a_device():
    lib = ggmod.load_library()
    one = (C.c_int64 * 1)(7)
    lane = (C.c_uint32 * 1)(0)
    st, res = ggmod.CheapestPathsStats(), C.c_void_p(1)
    st.rows, st.search.rounds = 9, 9
    assert lib.gg_cheapest64_paths(None, None, None, one, 1, lane, one, 1, 1, C.byref(st), C.byref(res)) == GG_ERR_INVALID_ARG
    assert res.value is None and st.rows == 0 and st.search.rounds == 0  # both outputs are cleared first
    assert lib.gg_cheapest64_paths(None, None, None, None, 1, None, None, 0, 0, None, None) == GG_ERR_INVALID_ARG
    n, got = C.c_uint64(5), C.c_uint32(5)
    assert lib.gg_cheapest64_paths_rows(None, 0, C.byref(n)) == GG_ERR_INVALID_ARG
    assert lib.gg_cheapest64_paths_fetch_pairs(None, 0, 8, None, None, None, None, C.byref(got)) == GG_ERR_INVALID_ARG
    assert lib.gg_cheapest64_paths_fetch(None, 0, 8, one, None, one, None, None, C.byref(got)) == GG_ERR_INVALID_ARG
