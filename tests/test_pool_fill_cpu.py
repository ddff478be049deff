"""gg_debug_pool_fill as an entry point, and the lock that keeps tests/test_gpu_pool_fill.py complete (no GPU).

Every symbol of gg.SYMBOLS is either run under the pool fills (COVERED there names the test) or written out below as
exempt: a symbol that allocates no scratch of its own -- the context, the staging, the readers of a finished result (rows,
fetch, levels), close, the profiler, the debug knobs and read-outs.  A device operation added to the C ABI later fails
here until it is run under the fills."""
import ctypes
import inspect

import duckdb_pgq_amd.gg as ggmod
from tests import test_gpu_pool_fill as filled
from tests.test_abi import _header_functions

GG_ERR_INVALID_ARG = -1

EXEMPT = [
    # the library and the context
    "gg_version", "gg_last_error", "gg_device_count", "gg_ctx_create", "gg_ctx_destroy", "gg_ctx_set_edge_rowid",
    "gg_stream_wait", "gg_host_alloc", "gg_host_free",
    # staging
    "gg_vertices_append", "gg_edges_append", "gg_staging_sync", "gg_staging_counts", "gg_staging_clear",
    "gg_staging_clear_edges",
    # rows, levels and fetches of a finished result; info of a CSR
    "gg_csr_info", "gg_result_rows", "gg_result_fetch", "gg_result_fetch_edges", "gg_triangles_fetch_edges",
    "gg_walk_closure_levels", "gg_walk_closure_fetch", "gg_reach_closure_levels", "gg_reach_closure_fetch",
    "gg_level_sets_levels", "gg_level_sets_fetch", "gg_bfs64_paths_rows", "gg_bfs64_paths_fetch",
    "gg_bfs64_all_paths_rows", "gg_bfs64_all_paths_fetch_pairs", "gg_bfs64_all_paths_fetch",
    "gg_khop_aggregate_rows", "gg_khop_aggregate_fetch", "gg_khop_pair_counts_rows", "gg_khop_pair_counts_fetch",
    "gg_cheapest64_rows", "gg_cheapest64_fetch", "gg_cheapest64_paths_rows", "gg_cheapest64_paths_fetch_pairs",
    "gg_cheapest64_paths_fetch", "gg_components_rows", "gg_components_fetch", "gg_components_fetch_sizes",
    "gg_tuple_groups_rows", "gg_tuple_groups_fetch",
    # close
    "gg_csr_destroy", "gg_result_destroy", "gg_edge_weights_destroy", "gg_bfs_sharded_end",
    # the profiler
    "gg_profile_enable", "gg_profile_select", "gg_profile_reset", "gg_profile_count", "gg_profile_get",
    # debug knobs and read-outs
    "gg_debug_force_frontier", "gg_debug_force_legacy_build", "gg_debug_scan_fault", "gg_debug_rank_mode",
    "gg_debug_csr_reverse_ready", "gg_debug_csr_reverse_index_ready", "gg_debug_max_grid_tiles", "gg_debug_reset",
    "gg_debug_placement", "gg_debug_pool", "gg_debug_pool_fill", "gg_debug_reach_visited", "gg_debug_level_sets",
    "gg_debug_bfs_steps", "gg_debug_triangle_tile", "gg_debug_aggregate_long_row", "gg_debug_aggregate_top",
    "gg_debug_aggregate_top_listed", "gg_debug_pair_counts", "gg_debug_cheapest", "gg_debug_components", "gg_debug_extend",
    "gg_debug_group", "gg_debug_value_top", "gg_debug_distinct", "gg_debug_group_tuples",
]

# the operations the fills were built for: none of them may ever be moved to EXEMPT
OPERATIONS = [
    "gg_csr_build", "gg_vertices_from_edges", "gg_csr_export", "gg_debug_csr_reverse",
    "gg_khop_count", "gg_expand_khop", "gg_expand_khop_result", "gg_expand_khop_edges", "gg_expand_khop_range",
    "gg_expand_khop_mid", "gg_expand_khop_mid_result", "gg_result_filter_common_neighbour",
    "gg_bfs64", "gg_bfs64_pairs", "gg_bfs64_paths", "gg_bfs64_all_paths",
    "gg_walk_closure", "gg_reach_closure", "gg_level_sets",
    "gg_triangles", "gg_triangles_edges",
    "gg_khop_aggregate", "gg_khop_aggregate_top", "gg_khop_pair_counts", "gg_cheapest64", "gg_cheapest64_paths",
    "gg_components",
    "gg_result_filter_edge", "gg_result_extend_edge", "gg_result_group_by", "gg_result_filter_value", "gg_result_top_rows",
    "gg_result_distinct", "gg_result_group_tuples",
    "gg_debug_scan", "gg_debug_sort_pairs",
]


def test_the_header_declares_the_library_exports_and_the_binding_names_the_entry_point():
    assert "gg_debug_pool_fill" in _header_functions()
    assert hasattr(ctypes.CDLL(ggmod.LIB_PATH), "gg_debug_pool_fill")
    assert "gg_debug_pool_fill" in ggmod.SYMBOLS
    assert callable(ggmod.GG.pool_fill)


def test_a_null_context_is_refused():
    lib = ggmod.load_library()
    fill, blocks, nbytes = ctypes.c_int(7), ctypes.c_uint64(7), ctypes.c_uint64(7)
    rc = lib.gg_debug_pool_fill(None, ctypes.byref(fill), ctypes.byref(blocks), ctypes.byref(nbytes))
    assert rc == GG_ERR_INVALID_ARG
    assert (fill.value, blocks.value, nbytes.value) == (7, 7, 7)  # nothing is written
    assert lib.gg_debug_pool_fill(None, None, None, None) == GG_ERR_INVALID_ARG


def test_every_symbol_is_run_under_the_fills_or_exempt_by_name():
    assert len(EXEMPT) == len(set(EXEMPT))
    assert not set(EXEMPT) & set(filled.COVERED), sorted(set(EXEMPT) & set(filled.COVERED))
    listed = set(EXEMPT) | set(filled.COVERED)
    assert listed <= set(ggmod.SYMBOLS), sorted(listed - set(ggmod.SYMBOLS))
    missing = [s for s in ggmod.SYMBOLS if s not in listed]
    assert not missing, f"neither run in tests/test_gpu_pool_fill.py nor exempt: {missing}"


def test_every_covering_test_exists():
    for symbol, name in filled.COVERED.items():
        fn = getattr(filled, name, None)
        assert name.startswith("test_") and inspect.isfunction(fn), (symbol, name)
        assert "filled" in inspect.signature(fn).parameters, (symbol, name)  # it runs on the filled contexts


def test_no_operation_is_exempt():
    for symbol in OPERATIONS:
        assert symbol in filled.COVERED and symbol not in EXEMPT, symbol
