"""ctypes binding of include/gg.h (test/bench harness; the C-ABI itself is the product boundary)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libgg.so")

GG_MAX_HOPS = 8
GG_BFS_LANES = 64
GG_CHUNK_ROWS = 1024
SORT_PREFILL = 0xA5A5A5A5  # GG_DEBUG_SORT_PREFILL

# every symbol include/gg.h declares (tests/test_abi.py checks the library exports exactly these)
SYMBOLS = [
    "gg_version", "gg_last_error", "gg_device_count", "gg_ctx_create", "gg_ctx_destroy",
    "gg_vertices_append", "gg_edges_append", "gg_staging_sync", "gg_staging_counts", "gg_staging_clear",
    "gg_ctx_set_edge_rowid", "gg_csr_build", "gg_csr_build_shard", "gg_csr_destroy", "gg_csr_info", "gg_csr_export",
    "gg_expand_khop", "gg_expand_khop_range", "gg_khop_count", "gg_expand_khop_dev", "gg_stream_wait", "gg_join_probe", "gg_khop_partition", "gg_expand_khop_mid", "gg_khop_partition_mid", "gg_expand_khop_mid_result",
    "gg_debug_force_frontier", "gg_debug_force_legacy_build", "gg_debug_scan_fault", "gg_debug_rank_mode",
    "gg_debug_csr_reverse", "gg_debug_csr_reverse_ready", "gg_debug_csr_reverse_index_ready", "gg_debug_scan", "gg_debug_sort_pairs",
    "gg_debug_max_grid_tiles", "gg_debug_reset", "gg_debug_placement", "gg_debug_pool", "gg_debug_pool_fill", "gg_debug_reach_visited",
    "gg_debug_level_sets", "gg_level_sets", "gg_level_sets_levels", "gg_level_sets_fetch",
    "gg_result_rows", "gg_result_fetch", "gg_result_destroy", "gg_expand_khop_result", "gg_result_digest",
    "gg_expand_khop_edges", "gg_result_fetch_edges",
    "gg_result_filter_common_neighbour", "gg_result_filter_edge", "gg_staging_clear_edges", "gg_vertices_from_edges",
    "gg_bfs64", "gg_bfs64_pairs", "gg_bfs64_pairs_packed", "gg_bfs64_paths", "gg_bfs64_paths_rows", "gg_bfs64_paths_fetch",
    "gg_bfs64_all_paths", "gg_bfs64_all_paths_rows", "gg_bfs64_all_paths_fetch_pairs", "gg_bfs64_all_paths_fetch",
    "gg_debug_bfs_steps",
    "gg_walk_endpoints", "gg_walk_closure", "gg_walk_closure_levels",
    "gg_walk_closure_fetch", "gg_reach_closure", "gg_reach_closure_levels", "gg_reach_closure_fetch", "gg_host_alloc", "gg_host_free", "gg_csr_lookup",
    "gg_bfs_sharded_begin", "gg_bfs_sharded_expand", "gg_bfs_sharded_words", "gg_bfs_sharded_commit",
    "gg_bfs_sharded_pairs", "gg_bfs_sharded_end", "gg_bfs_sharded_levels",
    "gg_triangles", "gg_triangles_edges", "gg_triangles_fetch_edges", "gg_debug_triangle_tile",
    "gg_khop_aggregate", "gg_khop_aggregate_rows", "gg_khop_aggregate_fetch", "gg_debug_aggregate_long_row",
    "gg_khop_aggregate_top", "gg_debug_aggregate_top", "gg_debug_aggregate_top_listed",
    "gg_khop_pair_counts", "gg_khop_pair_counts_rows", "gg_khop_pair_counts_fetch", "gg_debug_pair_counts",
    "gg_edge_weights_create", "gg_edge_weights_destroy", "gg_cheapest64", "gg_cheapest64_rows", "gg_cheapest64_fetch",
    "gg_debug_cheapest",
    "gg_cheapest64_paths", "gg_cheapest64_paths_rows", "gg_cheapest64_paths_fetch_pairs", "gg_cheapest64_paths_fetch",
    "gg_components", "gg_components_rows", "gg_components_fetch", "gg_components_fetch_sizes", "gg_debug_components",
    "gg_result_extend_edge", "gg_debug_extend",
    "gg_result_group_by", "gg_debug_group",
    "gg_result_filter_value", "gg_result_top_rows", "gg_debug_value_top",
    "gg_result_distinct", "gg_debug_distinct",
    "gg_result_group_tuples", "gg_tuple_groups_rows", "gg_tuple_groups_fetch", "gg_debug_group_tuples",
    "gg_profile_enable", "gg_profile_select", "gg_profile_reset", "gg_profile_count", "gg_profile_get",
]


class GGError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"gg error {code}: {msg}")
        self.code = code


class KhopStats(C.Structure):
    _fields_ = [
        ("rows", C.c_uint64 * (GG_MAX_HOPS + 1)),
        ("digest", C.c_uint64 * (GG_MAX_HOPS + 1)),
        ("traversed_edges", C.c_uint64),
        ("frontier_entries", C.c_uint64),
    ]


class BfsStats(C.Structure):
    _fields_ = [
        ("levels", C.c_uint32),
        ("traversed_edges", C.c_uint64),
        ("active_vertices", C.c_uint64),
        ("reached_pairs", C.c_uint64),
    ]


class AllPathsStats(C.Structure):
    _fields_ = [
        ("bfs", BfsStats),
        ("pairs_reached", C.c_uint64),
        ("paths", C.c_uint64),
        ("paths_kept", C.c_uint64),
        ("rows", C.c_uint64),
        ("sigma_entries", C.c_uint64),
        ("sigma_gathered", C.c_uint64),
    ]


class TriStats(C.Structure):
    _fields_ = [("rows", C.c_uint64), ("digest", C.c_uint64), ("wedges", C.c_uint64)]


class EdgeFilterStats(C.Structure):
    _fields_ = [("rows_in", C.c_uint64), ("rows_out", C.c_uint64), ("matches", C.c_uint64)]


class ExtendStats(C.Structure):
    _fields_ = [("rows_in", C.c_uint64), ("rows_out", C.c_uint64), ("rows_matched", C.c_uint64)]


class GroupStats(C.Structure):
    _fields_ = [("rows_in", C.c_uint64), ("rows_grouped", C.c_uint64), ("groups", C.c_uint64), ("route", C.c_uint32)]


class ValueFilterStats(C.Structure):
    _fields_ = [("rows_in", C.c_uint64), ("rows_valued", C.c_uint64), ("rows_out", C.c_uint64)]


class ValueTopStats(C.Structure):
    _fields_ = [("rows_in", C.c_uint64), ("rows_valued", C.c_uint64), ("candidates", C.c_uint64), ("rows_out", C.c_uint64),
                ("select_passes", C.c_uint32), ("sort_route", C.c_uint32)]


class DistinctStats(C.Structure):
    _fields_ = [("rows_in", C.c_uint64), ("rows_out", C.c_uint64), ("slots", C.c_uint64), ("probe_steps", C.c_uint64)]


class GroupTuplesStats(C.Structure):
    _fields_ = [("rows_in", C.c_uint64), ("rows_valued", C.c_uint64), ("groups", C.c_uint64), ("slots", C.c_uint64),
                ("probe_steps", C.c_uint64), ("route", C.c_uint32)]


class AggStats(C.Structure):
    _fields_ = [
        ("groups", C.c_uint64 * (GG_MAX_HOPS + 1)),
        ("walks", C.c_uint64 * (GG_MAX_HOPS + 1)),
        ("entries_pulled", C.c_uint64),
    ]


class PairStats(C.Structure):
    _fields_ = [
        ("pairs", C.c_uint64 * (GG_MAX_HOPS + 1)),
        ("walks", C.c_uint64 * (GG_MAX_HOPS + 1)),
        ("entries_pulled", C.c_uint64),
        ("rows_gathered", C.c_uint64),
    ]


class CheapestStats(C.Structure):
    _fields_ = [
        ("rounds", C.c_uint64),
        ("reached_pairs", C.c_uint64),
        ("cells_lowered", C.c_uint64),
        ("entries_pulled", C.c_uint64),
        ("rows_gathered", C.c_uint64),
    ]


class CheapestPathsStats(C.Structure):
    _fields_ = [
        ("search", CheapestStats),
        ("pairs_reached", C.c_uint64),
        ("pairs_saturated", C.c_uint64),
        ("rows", C.c_uint64),
        ("entries_scanned", C.c_uint64),
    ]


class CcStats(C.Structure):
    _fields_ = [
        ("vertices", C.c_uint64),
        ("components", C.c_uint64),
        ("largest", C.c_uint64),
        ("singletons", C.c_uint64),
        ("entries_read", C.c_uint64),
        ("hooks", C.c_uint64),
        ("jump_launches", C.c_uint32),
    ]


class TopStats(C.Structure):
    _fields_ = [("rows_in", C.c_uint64), ("rows_out", C.c_uint64), ("select_passes", C.c_uint32),
                ("sort_route", C.c_uint32)]


GROUP_BY = {"start": 0, "end": 1}  # GG_GROUP_START / GG_GROUP_END
TOP_BY = {"total": 0, "walks": 1}  # GG_TOP_BY_TOTAL / GG_TOP_BY_WALKS
EDGE_MODES = {"inner": 0, "semi": 1, "anti": 2}  # GG_EDGE_INNER / GG_EDGE_SEMI / GG_EDGE_ANTI
WEIGHTS_BY = {"rowid": 0, "entry": 1}  # GG_WEIGHTS_BY_ROWID / GG_WEIGHTS_BY_ENTRY
VALUE_MODES = {"in": 0, "not_in": 1}  # GG_VALUE_IN / GG_VALUE_NOT_IN
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1

_lib = None


def load_library(path: str | None = None):
    """Load libgg.so; raises (loudly) if the HIP extension has not been built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise ImportError(
            f"{p} not found: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()'). "
            "There is no CPU fallback for the gg hot path."
        )
    lib = C.CDLL(p)
    P, u64, i64p = C.c_void_p, C.c_uint64, C.POINTER(C.c_int64)
    lib.gg_version.restype = C.c_char_p
    lib.gg_last_error.restype = C.c_char_p
    lib.gg_device_count.argtypes = [C.POINTER(C.c_int)]
    lib.gg_ctx_create.argtypes = [C.c_int, C.POINTER(P)]
    lib.gg_ctx_destroy.argtypes = [P]
    lib.gg_ctx_destroy.restype = None
    lib.gg_vertices_append.argtypes = [P, i64p, u64]
    lib.gg_edges_append.argtypes = [P, i64p, i64p, i64p, u64]
    lib.gg_staging_sync.argtypes = [P]
    lib.gg_staging_counts.argtypes = [P, C.POINTER(u64), C.POINTER(u64)]
    lib.gg_staging_clear.argtypes = [P]
    lib.gg_csr_build.argtypes = [P, C.POINTER(P)]
    lib.gg_csr_build_shard.argtypes = [P, C.c_int, C.c_int, C.POINTER(P)]
    lib.gg_ctx_set_edge_rowid.argtypes = [P, C.c_int]
    lib.gg_csr_destroy.argtypes = [P]
    lib.gg_csr_destroy.restype = None
    lib.gg_csr_info.argtypes = [P, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    lib.gg_csr_export.argtypes = [P, i64p, i64p, i64p, i64p]
    lib.gg_expand_khop.argtypes = [P, P, i64p, u64, C.c_int, C.c_int, C.c_int, C.POINTER(KhopStats), C.POINTER(P)]
    lib.gg_expand_khop_range.argtypes = [P, P, u64, u64, C.c_int, C.c_int, C.c_int, C.POINTER(KhopStats), C.POINTER(P)]
    lib.gg_khop_partition.argtypes = [P, P, C.c_int, C.POINTER(u64)]
    lib.gg_khop_count.argtypes = [P, P, i64p, u64, C.c_int, C.c_int, C.POINTER(u64)]
    lib.gg_expand_khop_dev.argtypes = [P, P, C.c_int, C.POINTER(C.c_void_p)]
    lib.gg_stream_wait.argtypes = [P, C.c_void_p, C.c_int]
    lib.gg_join_probe.argtypes = [P, P, i64p, u64, C.POINTER(u64), C.POINTER(P)]
    lib.gg_expand_khop_mid.argtypes = [P, P, u64, u64, C.c_int, C.c_int, C.POINTER(KhopStats)]
    lib.gg_khop_partition_mid.argtypes = [P, P, C.c_int, C.POINTER(u64)]
    lib.gg_expand_khop_mid_result.argtypes = [P, P, u64, u64, C.c_int, C.POINTER(KhopStats), C.POINTER(P)]
    lib.gg_debug_force_frontier.argtypes = [P, C.c_int]
    lib.gg_debug_force_legacy_build.argtypes = [P, C.c_int]
    lib.gg_debug_rank_mode.argtypes = [P, C.c_int]
    lib.gg_debug_csr_reverse.argtypes = [P, i64p, i64p, i64p, C.POINTER(C.c_int)]
    lib.gg_debug_csr_reverse_ready.argtypes = [P, C.POINTER(C.c_int)]
    lib.gg_debug_csr_reverse_index_ready.argtypes = [P, C.POINTER(C.c_int)]
    lib.gg_debug_scan_fault.argtypes = [P, C.c_uint32, u64]
    lib.gg_debug_scan.argtypes = [P, C.c_void_p, u64, C.c_int, C.c_void_p, C.POINTER(u64)]
    lib.gg_debug_sort_pairs.argtypes = [P] + [C.c_void_p] * 3 + [u64, C.c_int] + [C.c_void_p] * 3 + [C.POINTER(u64)]
    lib.gg_debug_max_grid_tiles.argtypes = [P, u64]
    lib.gg_debug_reset.argtypes = [P]
    lib.gg_debug_placement.argtypes = [P, C.POINTER(u64), C.POINTER(u64)]
    lib.gg_debug_pool.argtypes = [P, C.POINTER(u64), C.POINTER(u64)]
    lib.gg_debug_pool_fill.argtypes = [P, C.POINTER(C.c_int), C.POINTER(u64), C.POINTER(u64)]
    lib.gg_debug_reach_visited.argtypes = [P, C.c_int, u64]
    lib.gg_debug_bfs_steps.argtypes = [P, C.POINTER(u64), u64, C.POINTER(u64), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.gg_result_rows.argtypes = [P, C.c_int, C.POINTER(u64)]
    lib.gg_result_fetch.argtypes = [P, C.c_int, u64, C.c_uint32, C.POINTER(i64p), C.POINTER(C.c_uint32)]
    lib.gg_expand_khop_result.argtypes = [P, P, i64p, u64, C.c_int, C.c_int, C.POINTER(KhopStats), C.POINTER(P)]
    lib.gg_result_filter_common_neighbour.argtypes = [P, P, C.c_int, P, C.POINTER(P)]
    lib.gg_result_filter_edge.argtypes = [P, P, C.c_int, P, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.POINTER(EdgeFilterStats), C.POINTER(P)]
    lib.gg_staging_clear_edges.argtypes = [P]
    lib.gg_vertices_from_edges.argtypes = [P, C.c_int, C.POINTER(u64)]
    lib.gg_result_destroy.argtypes = [P]
    lib.gg_result_destroy.restype = None
    lib.gg_result_digest.argtypes = [P, P, P, C.c_int, C.POINTER(u64), C.POINTER(u64)]
    lib.gg_expand_khop_edges.argtypes = [P, P, i64p, u64, C.c_int, C.POINTER(KhopStats), C.POINTER(P)]
    lib.gg_result_fetch_edges.argtypes = [P, C.c_int, u64, C.c_uint32, C.POINTER(i64p), C.POINTER(C.c_uint32)]
    lib.gg_bfs64.argtypes = [P, P, i64p, C.c_int, C.c_int, i64p, u64, C.POINTER(C.c_int32), C.POINTER(BfsStats)]
    lib.gg_host_alloc.argtypes = [P, u64, C.POINTER(C.c_void_p)]
    lib.gg_host_free.argtypes = [P, C.c_void_p]
    lib.gg_host_free.restype = None
    lib.gg_csr_lookup.argtypes = [P, P, i64p, u64, C.POINTER(C.c_uint32)]
    lib.gg_bfs64_pairs.argtypes = [P, P, i64p, C.c_int, C.c_int, C.POINTER(BfsStats), C.POINTER(P)]
    lib.gg_bfs64_pairs_packed.argtypes = [P, P, i64p, C.c_int, C.c_int, C.POINTER(BfsStats), C.POINTER(P)]
    lib.gg_bfs64_paths.argtypes = [P, P, i64p, C.c_int, C.c_int, C.POINTER(C.c_uint32), i64p, u64, C.c_int,
                                   C.POINTER(BfsStats), C.POINTER(P)]
    lib.gg_bfs64_paths_rows.argtypes = [P, C.POINTER(u64)]
    lib.gg_bfs64_paths_fetch.argtypes = [P, u64, C.c_uint32, i64p, C.POINTER(C.c_int32), i64p, i64p, C.POINTER(C.c_uint32)]
    u32p, i32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(u64)
    lib.gg_bfs64_all_paths.argtypes = [P, P, i64p, C.c_int, C.c_int, u32p, i64p, u64, u64, C.c_int, C.c_int,
                                       C.POINTER(AllPathsStats), C.POINTER(P)]
    lib.gg_bfs64_all_paths_rows.argtypes = [P, C.c_int, u64p]
    lib.gg_bfs64_all_paths_fetch_pairs.argtypes = [P, u64, C.c_uint32, i64p, i32p, u64p, u64p, u32p]
    lib.gg_bfs64_all_paths_fetch.argtypes = [P, u64, C.c_uint32, i64p, i64p, i32p, i64p, i64p, u32p]
    lib.gg_walk_endpoints.argtypes = [P, P, i64p, u64, C.c_int, C.POINTER(P)]
    lib.gg_walk_closure.argtypes = [P, P, i64p, u64, C.c_int, C.POINTER(P)]
    lib.gg_walk_closure_levels.argtypes = [P, C.POINTER(u64), C.c_int, C.POINTER(C.c_int)]
    lib.gg_walk_closure_fetch.argtypes = [P, u64, C.c_uint32, i64p, i64p, C.POINTER(C.c_int32), C.POINTER(C.c_uint32)]
    lib.gg_reach_closure.argtypes = [P, P, i64p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), u64, C.c_uint32,
                                     C.POINTER(P)]
    lib.gg_level_sets.argtypes = [P, P, i64p, C.POINTER(C.c_uint32), u64, C.c_uint32, C.c_int, C.POINTER(P)]
    lib.gg_level_sets_levels.argtypes = [P, C.POINTER(u64), C.c_int, C.POINTER(C.c_int)]
    lib.gg_level_sets_fetch.argtypes = [P, u64, C.c_uint32, i64p, i64p, C.POINTER(C.c_int32), C.POINTER(C.c_uint32)]
    lib.gg_result_extend_edge.argtypes = [P, P, C.c_int, P, C.c_int, C.c_int, C.c_int, C.POINTER(ExtendStats),
                                          C.POINTER(P)]
    lib.gg_debug_extend.argtypes = [P, C.c_uint32]
    lib.gg_result_group_by.argtypes = [P, P, C.c_int, C.c_int, P, C.c_int, P, i64p, C.POINTER(GroupStats), C.POINTER(P)]
    lib.gg_debug_group.argtypes = [P, C.c_int, C.c_uint32]
    lib.gg_result_filter_value.argtypes = [P, P, C.c_int, C.c_int, P, i64p, C.POINTER(u64), C.c_int64, C.c_int64, C.c_int,
                                           C.c_int, C.POINTER(ValueFilterStats), C.POINTER(P)]
    lib.gg_result_top_rows.argtypes = [P, P, C.c_int, C.c_int, P, i64p, C.POINTER(u64), C.c_int64, C.c_int64, C.c_int,
                                       C.c_int, C.c_int, u64, C.POINTER(ValueTopStats), C.POINTER(P)]
    lib.gg_debug_value_top.argtypes = [P, C.c_int, C.c_uint32]
    lib.gg_result_distinct.argtypes = [P, P, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(DistinctStats),
                                       C.POINTER(P)]
    lib.gg_debug_distinct.argtypes = [P, u64, C.c_int]
    lib.gg_result_group_tuples.argtypes = [P, P, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, P, i64p, C.POINTER(u64),
                                           C.POINTER(GroupTuplesStats), C.POINTER(P)]
    lib.gg_tuple_groups_rows.argtypes = [P, C.POINTER(u64), C.POINTER(C.c_int)]
    lib.gg_tuple_groups_fetch.argtypes = [P, u64, C.c_uint32, C.POINTER(i64p), C.POINTER(u64), C.POINTER(u64), i64p, i64p,
                                          i64p, i64p, C.POINTER(C.c_uint32)]
    lib.gg_debug_group_tuples.argtypes = [P, C.c_int, C.c_uint32]
    lib.gg_debug_level_sets.argtypes = [P, C.c_int, C.c_int]
    lib.gg_reach_closure_levels.argtypes = [P, C.POINTER(u64), C.c_int, C.POINTER(C.c_int)]
    lib.gg_reach_closure_fetch.argtypes = [P, u64, C.c_uint32, i64p, i64p, C.POINTER(C.c_int32), C.POINTER(C.c_uint32)]
    lib.gg_bfs_sharded_begin.argtypes = [P, P, i64p, C.c_int, C.POINTER(P)]
    lib.gg_bfs_sharded_expand.argtypes = [P, C.POINTER(C.c_void_p), C.POINTER(u64), C.POINTER(u64)]
    lib.gg_bfs_sharded_words.argtypes = [P, C.POINTER(C.c_uint64), C.c_int]
    lib.gg_bfs_sharded_commit.argtypes = [P]
    lib.gg_bfs_sharded_pairs.argtypes = [P, C.POINTER(P)]
    lib.gg_bfs_sharded_levels.argtypes = [P, C.POINTER(u64), C.POINTER(u64)]
    lib.gg_bfs_sharded_end.argtypes = [P]
    lib.gg_bfs_sharded_end.restype = None
    lib.gg_triangles.argtypes = [P, P, i64p, u64, C.c_int, C.c_int, C.POINTER(TriStats), C.POINTER(P)]
    lib.gg_triangles_edges.argtypes = [P, P, i64p, u64, C.c_int, C.POINTER(TriStats), C.POINTER(P)]
    lib.gg_triangles_fetch_edges.argtypes = [P, u64, C.c_uint32, C.POINTER(i64p), C.POINTER(C.c_uint32)]
    lib.gg_debug_triangle_tile.argtypes = [P, C.c_uint32]
    lib.gg_khop_aggregate.argtypes = [P, P, i64p, u64, C.c_int, C.c_int, C.c_int, i64p, C.POINTER(AggStats), C.POINTER(P)]
    lib.gg_khop_aggregate_rows.argtypes = [P, C.c_int, C.POINTER(u64)]
    lib.gg_khop_aggregate_fetch.argtypes = [P, C.c_int, u64, C.c_uint32, i64p, C.POINTER(u64), C.POINTER(u64), i64p,
                                            C.POINTER(C.c_uint32)]
    lib.gg_debug_aggregate_long_row.argtypes = [P, C.c_uint32]
    lib.gg_khop_aggregate_top.argtypes = [P, P, C.c_int, C.c_int, C.c_int, u64, P, i64p, C.POINTER(TopStats), C.POINTER(P)]
    lib.gg_debug_aggregate_top.argtypes = [P, C.c_int, C.c_uint32]
    lib.gg_debug_aggregate_top_listed.argtypes = [P, C.POINTER(u64)]
    lib.gg_khop_pair_counts.argtypes = [P, P, i64p, C.c_int, C.c_int, C.c_int, i64p, u64, C.POINTER(PairStats),
                                        C.POINTER(P)]
    lib.gg_khop_pair_counts_rows.argtypes = [P, C.c_int, C.POINTER(u64)]
    lib.gg_khop_pair_counts_fetch.argtypes = [P, C.c_int, u64, C.c_uint32, i64p, i64p, C.POINTER(u64), C.POINTER(C.c_uint32)]
    lib.gg_debug_pair_counts.argtypes = [P, C.c_uint32, C.c_int]
    lib.gg_edge_weights_create.argtypes = [P, P, i64p, u64, C.c_int, C.POINTER(P)]
    lib.gg_edge_weights_destroy.argtypes = [P]
    lib.gg_edge_weights_destroy.restype = None
    lib.gg_cheapest64.argtypes = [P, P, P, i64p, C.c_int, C.c_int64, i64p, u64, C.POINTER(CheapestStats), C.POINTER(P)]
    lib.gg_cheapest64_rows.argtypes = [P, C.POINTER(u64)]
    lib.gg_cheapest64_fetch.argtypes = [P, u64, C.c_uint32, i64p, i64p, i64p, C.POINTER(C.c_int32), C.POINTER(C.c_uint32)]
    lib.gg_debug_cheapest.argtypes = [P, C.c_uint32, C.c_int]
    lib.gg_cheapest64_paths.argtypes = [P, P, P, i64p, C.c_int, u32p, i64p, u64, C.c_int, C.POINTER(CheapestPathsStats),
                                        C.POINTER(P)]
    lib.gg_cheapest64_paths_rows.argtypes = [P, C.c_int, u64p]
    lib.gg_cheapest64_paths_fetch_pairs.argtypes = [P, u64, C.c_uint32, i64p, i64p, i32p, i32p, u32p]
    lib.gg_cheapest64_paths_fetch.argtypes = [P, u64, C.c_uint32, i64p, i32p, i64p, i64p, i64p, u32p]
    lib.gg_components.argtypes = [P, P, C.POINTER(CcStats), C.POINTER(P)]
    lib.gg_components_rows.argtypes = [P, C.c_int, C.POINTER(u64)]
    lib.gg_components_fetch.argtypes = [P, u64, C.c_uint32, i64p, i64p, C.POINTER(u64), C.POINTER(C.c_uint32)]
    lib.gg_components_fetch_sizes.argtypes = [P, u64, C.c_uint32, i64p, C.POINTER(u64), C.POINTER(C.c_uint32)]
    lib.gg_debug_components.argtypes = [P, C.c_int, C.c_uint32]
    lib.gg_profile_enable.argtypes = [P, C.c_int]
    lib.gg_profile_select.argtypes = [P, C.c_char_p]
    lib.gg_profile_reset.argtypes = [P]
    lib.gg_profile_count.argtypes = [P, C.POINTER(C.c_int)]
    lib.gg_profile_get.argtypes = [P, C.c_int, C.POINTER(C.c_char_p), C.POINTER(u64), C.POINTER(C.c_double)]
    if path is None:
        _lib = lib
    return lib


def _i64(a):
    a = np.ascontiguousarray(a, dtype=np.int64)
    return a, a.ctypes.data_as(C.POINTER(C.c_int64))


class ShardedBfs:
    """One rank's state of a graph-sharded BFS (gg_bfs_sharded_*)."""

    def __init__(self, gg: "GG", handle, V: int):
        self.gg, self.handle, self.V = gg, handle, V
        self.next_ptr = 0

    def expand(self) -> int:
        """Pull the next frontier words of the owned vertices; returns the rank's newly reached pairs."""
        ptr, n, new = C.c_void_p(), C.c_uint64(), C.c_uint64()
        self.gg._chk(self.gg.lib.gg_bfs_sharded_expand(self.handle, C.byref(ptr), C.byref(n), C.byref(new)))
        self.next_ptr = ptr.value or 0
        return int(new.value)

    @property
    def __cuda_array_interface__(self):
        """The rank's next-frontier words in HBM, for a device-side collective: torch.as_tensor(run, device="cuda")
        views them as int64[V] (a SUM all-reduce over disjoint supports is the OR of the ranks' words)."""
        return {"shape": (self.V,), "typestr": "<i8", "data": (self.next_ptr, False), "version": 2}

    def words(self) -> np.ndarray:
        out = np.empty(self.V, np.uint64)
        self.gg._chk(self.gg.lib.gg_bfs_sharded_words(self.handle, out.ctypes.data_as(C.POINTER(C.c_uint64)), 0))
        return out

    def set_words(self, words: np.ndarray):
        w = np.ascontiguousarray(words, np.uint64)
        self.gg._chk(self.gg.lib.gg_bfs_sharded_words(self.handle, w.ctypes.data_as(C.POINTER(C.c_uint64)), 1))

    def commit(self):
        self.gg._chk(self.gg.lib.gg_bfs_sharded_commit(self.handle))

    def levels(self):
        """(levels this rank pushed, levels it pulled) so far."""
        push, pull = C.c_uint64(), C.c_uint64()
        self.gg._chk(self.gg.lib.gg_bfs_sharded_levels(self.handle, C.byref(push), C.byref(pull)))
        return int(push.value), int(pull.value)

    def pairs(self) -> np.ndarray:
        i64p = C.POINTER(C.c_int64)
        res = C.c_void_p()
        self.gg._chk(self.gg.lib.gg_bfs_sharded_pairs(self.handle, C.byref(res)))
        try:
            n = C.c_uint64()
            self.gg._chk(self.gg.lib.gg_result_rows(res, 2, C.byref(n)))
            out = np.empty((3, n.value), np.int64)
            if n.value:
                ptrs = (i64p * 3)(*[out[c].ctypes.data_as(i64p) for c in range(3)])
                got = C.c_uint32()
                self.gg._chk(self.gg.lib.gg_result_fetch(res, 2, 0, n.value, ptrs, C.byref(got)))
        finally:
            self.gg.lib.gg_result_destroy(res)
        return out.T.copy()

    def close(self):
        if self.handle:
            self.gg.lib.gg_bfs_sharded_end(self.handle)
            self.handle = None


class DeviceWords:
    """n uint64 words in device memory owned by the library, viewable as a tensor (torch.as_tensor(words, device=...)):
    what a device-side collective reduces in place."""

    def __init__(self, ptr: int, n: int):
        self.ptr, self.n = ptr, n

    @property
    def __cuda_array_interface__(self):
        # (int64: torch has no uint64 arithmetic; sums of counts stay far below 2^63, digests are masked by the reader)
        return {"shape": (self.n,), "typestr": "<i8", "data": (self.ptr, False), "version": 2}


class KhopResult:
    """Materialised walks left in HBM (gg_expand_khop_result): row counts and <=1024-row slices on demand."""

    def __init__(self, gg: "GG", handle, stats):
        self.gg, self.handle, self.stats = gg, handle, stats

    def rows(self, h: int) -> int:
        n = C.c_uint64()
        self.gg._chk(self.gg.lib.gg_result_rows(self.handle, h, C.byref(n)))
        return int(n.value)

    def fetch_edges(self, h: int, offset: int, max_rows: int = GG_CHUNK_ROWS) -> np.ndarray:
        """Edge rowids e1..eh of rows [offset, offset + max_rows) (results of expand_khop_edges)."""
        bufs = [np.empty(GG_CHUNK_ROWS, np.int64) for _ in range(h)]
        ptrs = (C.POINTER(C.c_int64) * h)(*[b.ctypes.data_as(C.POINTER(C.c_int64)) for b in bufs])
        got = C.c_uint32()
        self.gg._chk(self.gg.lib.gg_result_fetch_edges(self.handle, h, offset, min(max_rows, GG_CHUNK_ROWS), ptrs, C.byref(got)))
        return np.stack([b[: got.value] for b in bufs], axis=1)

    def fetch_triangle_edges(self, offset: int, max_rows: int = GG_CHUNK_ROWS) -> np.ndarray:
        """Edge rowids e1, e2, e3 of rows [offset, offset + max_rows) (results of triangles_edges): [n, 3] int64."""
        bufs = [np.empty(GG_CHUNK_ROWS, np.int64) for _ in range(3)]
        ptrs = (C.POINTER(C.c_int64) * 3)(*[b.ctypes.data_as(C.POINTER(C.c_int64)) for b in bufs])
        got = C.c_uint32()
        self.gg._chk(self.gg.lib.gg_triangles_fetch_edges(self.handle, offset, min(max_rows, GG_CHUNK_ROWS), ptrs, C.byref(got)))
        return np.stack([b[: got.value] for b in bufs], axis=1)

    def digest(self, csr, h: int):
        """(rows, digest) of the h-hop rows as they stand in HBM — the figures a count-mode expansion reports."""
        n, d = C.c_uint64(), C.c_uint64()
        self.gg._chk(self.gg.lib.gg_result_digest(self.gg.ctx, csr.handle, self.handle, h, C.byref(n), C.byref(d)))
        return int(n.value), int(d.value)

    def fetch(self, h: int, offset: int, max_rows: int = GG_CHUNK_ROWS) -> np.ndarray:
        bufs = [np.empty(GG_CHUNK_ROWS, np.int64) for _ in range(h + 1)]
        ptrs = (C.POINTER(C.c_int64) * (h + 1))(*[b.ctypes.data_as(C.POINTER(C.c_int64)) for b in bufs])
        got = C.c_uint32()
        self.gg._chk(self.gg.lib.gg_result_fetch(self.handle, h, offset, min(max_rows, GG_CHUNK_ROWS), ptrs, C.byref(got)))
        return np.stack([b[: got.value] for b in bufs], axis=1)

    def close(self):
        if self.handle:
            self.gg.lib.gg_result_destroy(self.handle)
            self.handle = None


class KhopAggregate:
    """Grouped aggregates over walks (gg_khop_aggregate), left in HBM: per level one row (vertex id, walks, total) per
    group.  stats: {"groups", "walks", "entries_pulled"}; handle None: the call asked for the stats only."""

    def __init__(self, gg: "GG", handle, stats):
        self.gg, self.handle, self.stats = gg, handle, stats

    def rows(self, h: int) -> int:
        n = C.c_uint64()
        self.gg._chk(self.gg.lib.gg_khop_aggregate_rows(self.handle, h, C.byref(n)))
        return int(n.value)

    def fetch(self, h: int):
        """(ids int64, walks uint64, totals: an object array of Python ints put together from the two halves)"""
        n = self.rows(h)
        ids, walks = np.empty(n, np.int64), np.empty(n, np.uint64)
        lo, hi = np.empty(n, np.uint64), np.empty(n, np.int64)
        i64p, u64p = C.POINTER(C.c_int64), C.POINTER(C.c_uint64)
        got, o = C.c_uint32(), 0
        while o < n:
            self.gg._chk(self.gg.lib.gg_khop_aggregate_fetch(
                self.handle, h, o, min(n - o, 1 << 20), ids[o:].ctypes.data_as(i64p), walks[o:].ctypes.data_as(u64p),
                lo[o:].ctypes.data_as(u64p), hi[o:].ctypes.data_as(i64p), C.byref(got)))
            if not got.value:
                raise GGError(-6, f"gg_khop_aggregate_fetch: no row at offset {o} of {n}")
            o += got.value
        totals = np.empty(n, object)
        totals[:] = [(int(h_) << 64) + int(l_) for l_, h_ in zip(lo.tolist(), hi.tolist())]
        return ids, walks, totals

    def close(self):
        if self.handle:
            self.gg.lib.gg_result_destroy(self.handle)
            self.handle = None


class TupleGroups:
    """Aggregates per key tuple (gg_result_group_tuples), left in HBM: one row per distinct tuple over the chosen columns,
    in input order of the tuples' first rows.  stats: {"rows_in", "rows_valued", "groups", "slots", "probe_steps",
    "route"}; handle None: the call asked for the stats only."""

    COLUMNS = ("rows", "valued", "sum", "min", "max")

    def __init__(self, gg: "GG", handle, stats):
        self.gg, self.handle, self.stats = gg, handle, stats

    def shape(self):
        """(groups, key columns)"""
        n, k = C.c_uint64(), C.c_int()
        self.gg._chk(self.gg.lib.gg_tuple_groups_rows(self.handle, C.byref(n), C.byref(k)))
        return int(n.value), int(k.value)

    def rows(self) -> int:
        return self.shape()[0]

    def fetch(self, offset: int = 0, n=None) -> dict:
        """rows [offset, offset + n) (None: to the end) as {"keys": int64 [m, key columns], "rows" / "valued": uint64 [m],
        "sum": an object array of Python ints put together from the two halves, "min" / "max": int64 [m]}"""
        total, k = self.shape()
        m = max(0, min(total - offset, total if n is None else int(n)))
        keys = np.empty((k, m), np.int64)
        rows, valued, lo = np.empty(m, np.uint64), np.empty(m, np.uint64), np.empty(m, np.uint64)
        hi, mn, mx = np.empty(m, np.int64), np.empty(m, np.int64), np.empty(m, np.int64)
        i64p, u64p = C.POINTER(C.c_int64), C.POINTER(C.c_uint64)
        got, o = C.c_uint32(), 0
        while o < m:
            kp = (i64p * max(k, 1))(*[keys[j, o:].ctypes.data_as(i64p) for j in range(k)])
            self.gg._chk(self.gg.lib.gg_tuple_groups_fetch(
                self.handle, offset + o, min(m - o, 1 << 20), kp, rows[o:].ctypes.data_as(u64p),
                valued[o:].ctypes.data_as(u64p), lo[o:].view(np.int64).ctypes.data_as(i64p), hi[o:].ctypes.data_as(i64p),
                mn[o:].ctypes.data_as(i64p), mx[o:].ctypes.data_as(i64p), C.byref(got)))
            if not got.value:
                raise GGError(-6, f"gg_tuple_groups_fetch: no row at offset {offset + o} of {total}")
            o += got.value
        sums = np.empty(m, object)
        sums[:] = [(int(h_) << 64) + int(l_) for l_, h_ in zip(lo.tolist(), hi.tolist())]
        return {"keys": np.ascontiguousarray(keys.T), "rows": rows, "valued": valued, "sum": sums, "min": mn, "max": mx}

    def close(self):
        if self.handle:
            self.gg.lib.gg_result_destroy(self.handle)
            self.handle = None


class KhopPairCounts:
    """Walks counted per (source, end vertex) pair (gg_khop_pair_counts), left in HBM: per level one row (source index,
    vertex id, walks) per pair, ascending by (source index, dense index of the vertex).  A source list longer than 64 is
    several batches: `parts` holds (result handle, first source index) per batch.  stats: {"pairs", "walks",
    "entries_pulled", "rows_gathered"} summed over the batches; no parts: the call asked for the stats only."""

    def __init__(self, gg: "GG", parts, stats):
        self.gg, self.parts, self.stats = gg, parts, stats

    def rows(self, h: int) -> int:
        total = 0
        for handle, _ in self.parts:
            n = C.c_uint64()
            self.gg._chk(self.gg.lib.gg_khop_pair_counts_rows(handle, h, C.byref(n)))
            total += int(n.value)
        return total

    def fetch(self, h: int):
        """(src_index int64, vertex_id int64, walks uint64) of level h, the batches one after the other"""
        i64p, u64p = C.POINTER(C.c_int64), C.POINTER(C.c_uint64)
        out = []
        for handle, base in self.parts:
            cnt = C.c_uint64()
            self.gg._chk(self.gg.lib.gg_khop_pair_counts_rows(handle, h, C.byref(cnt)))
            n = int(cnt.value)
            idx, ids, walks = np.empty(n, np.int64), np.empty(n, np.int64), np.empty(n, np.uint64)
            got, o = C.c_uint32(), 0
            while o < n:
                self.gg._chk(self.gg.lib.gg_khop_pair_counts_fetch(
                    handle, h, o, min(n - o, 1 << 20), idx[o:].ctypes.data_as(i64p), ids[o:].ctypes.data_as(i64p),
                    walks[o:].ctypes.data_as(u64p), C.byref(got)))
                if not got.value:
                    raise GGError(-6, f"gg_khop_pair_counts_fetch: no row at offset {o} of {n}")
                o += got.value
            out.append((idx + base, ids, walks))
        if not out:
            return np.empty(0, np.int64), np.empty(0, np.int64), np.empty(0, np.uint64)
        return tuple(np.concatenate([part[c] for part in out]) for c in range(3))

    def close(self):
        for handle, _ in self.parts:
            self.gg.lib.gg_result_destroy(handle)
        self.parts = []


class EdgeWeights:
    """A device-resident weight column of one CSR (gg_edge_weights); close() before the CSR."""

    def __init__(self, gg: "GG", handle):
        self.gg, self.handle = gg, handle

    def close(self):
        if self.handle:
            self.gg.lib.gg_edge_weights_destroy(self.handle)
            self.handle = None


class CheapestPaths:
    """Cheapest path costs (gg_cheapest64), left in HBM: one row (source index, vertex id, cost, hops) per reached pair,
    ascending by (source index, dense index of the vertex).  A source list longer than 64 is several batches: `parts` holds
    (result handle, first source index) per batch.  stats: {"rounds", "reached_pairs", "cells_lowered", "entries_pulled",
    "rows_gathered"} summed over the batches; no parts: the call asked for the stats only."""

    def __init__(self, gg: "GG", parts, stats):
        self.gg, self.parts, self.stats = gg, parts, stats

    def rows(self) -> int:
        total = 0
        for handle, _ in self.parts:
            n = C.c_uint64()
            self.gg._chk(self.gg.lib.gg_cheapest64_rows(handle, C.byref(n)))
            total += int(n.value)
        return total

    def fetch(self):
        """(src_index int64, vertex_id int64, cost int64, hops int32), the batches one after the other"""
        i64p, i32p = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
        out = []
        for handle, base in self.parts:
            cnt = C.c_uint64()
            self.gg._chk(self.gg.lib.gg_cheapest64_rows(handle, C.byref(cnt)))
            n = int(cnt.value)
            idx, ids, cost, hops = (np.empty(n, np.int64), np.empty(n, np.int64), np.empty(n, np.int64),
                                    np.empty(n, np.int32))
            got, o = C.c_uint32(), 0
            while o < n:
                self.gg._chk(self.gg.lib.gg_cheapest64_fetch(
                    handle, o, min(n - o, 1 << 20), idx[o:].ctypes.data_as(i64p), ids[o:].ctypes.data_as(i64p),
                    cost[o:].ctypes.data_as(i64p), hops[o:].ctypes.data_as(i32p), C.byref(got)))
                if not got.value:
                    raise GGError(-6, f"gg_cheapest64_fetch: no row at offset {o} of {n}")
                o += got.value
            out.append((idx + base, ids, cost, hops))
        if not out:
            return np.empty(0, np.int64), np.empty(0, np.int64), np.empty(0, np.int64), np.empty(0, np.int32)
        return tuple(np.concatenate([part[c] for part in out]) for c in range(4))

    def close(self):
        for handle, _ in self.parts:
            self.gg.lib.gg_result_destroy(handle)
        self.parts = []


class WalkClosure:
    """Every walk from a seed list (gg_walk_closure), left in HBM: level counts and row slices on demand."""
    _levels_fn, _fetch_fn = "gg_walk_closure_levels", "gg_walk_closure_fetch"

    def __init__(self, gg: "GG", handle):
        self.gg, self.handle = gg, handle

    def levels(self) -> int:
        """the deepest level with walks (0: none)"""
        n = C.c_int()
        self.gg._chk(getattr(self.gg.lib, self._levels_fn)(self.handle, None, 0, C.byref(n)))
        return int(n.value)

    def rows(self, level: int | None = None):
        """walks of `level` edges (level >= 1); without a level, every level's count as a list"""
        n = self.levels()
        counts = (C.c_uint64 * max(n, 1))()
        got = C.c_int()
        self.gg._chk(getattr(self.gg.lib, self._levels_fn)(self.handle, counts, n, C.byref(got)))
        if level is None:
            return [int(counts[i]) for i in range(n)]
        return int(counts[level - 1]) if 1 <= level <= n else 0

    def fetch(self, offset: int = 0, max_rows: int | None = None):
        """(seed_index int64, edge_rowid int64, level int32) of rows [offset, offset + max_rows), in row order"""
        total = sum(self.rows())
        want = max(0, total - offset) if max_rows is None else max(0, min(max_rows, total - offset))
        seed, rowid, level = np.empty(want, np.int64), np.empty(want, np.int64), np.empty(want, np.int32)
        i64p = C.POINTER(C.c_int64)
        done = 0
        while done < want:
            got = C.c_uint32()
            take = min(want - done, 1 << 30)
            self.gg._chk(getattr(self.gg.lib, self._fetch_fn)(
                self.handle, offset + done, take, seed[done:].ctypes.data_as(i64p), rowid[done:].ctypes.data_as(i64p),
                level[done:].ctypes.data_as(C.POINTER(C.c_int32)), C.byref(got)))
            if got.value == 0:
                break
            done += got.value
        return seed[:done], rowid[:done], level[:done]

    def close(self):
        if self.handle:
            self.gg.lib.gg_result_destroy(self.handle)
            self.handle = None


class ReachClosure(WalkClosure):
    """Every (class, vertex) reachable from a seed list (gg_reach_closure), left in HBM.  fetch() gives (class int64,
    vertex id int64, level int32) by level, inside a level ascending by (class, dense vertex index)."""
    _levels_fn, _fetch_fn = "gg_reach_closure_levels", "gg_reach_closure_fetch"


class LevelSets(ReachClosure):
    """The level sets of a seed list (gg_level_sets), left in HBM.  fetch() gives (class int64, vertex id int64, level
    int32): the members of level 1, then of level 2, ..., inside a level ascending by (class, dense vertex index)."""
    _levels_fn, _fetch_fn = "gg_level_sets_levels", "gg_level_sets_fetch"


class Csr:
    def __init__(self, gg: "GG", handle):
        self.gg, self.handle = gg, handle
        V, E, D = C.c_uint64(), C.c_uint64(), C.c_uint64()
        gg._chk(gg.lib.gg_csr_info(handle, C.byref(V), C.byref(E), C.byref(D)))
        self.V, self.E, self.dropped = V.value, E.value, D.value

    def export(self):
        off = np.empty(self.V + 1, np.int64)
        nbr = np.empty(self.E, np.int64)
        eid = np.empty(self.E, np.int64)
        vid = np.empty(self.V, np.int64)
        p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))  # noqa: E731
        self.gg._chk(self.gg.lib.gg_csr_export(self.handle, p(off), p(nbr), p(eid), p(vid)))
        return off, nbr, eid, vid

    @property
    def reverse_derived(self) -> int:
        """1 if the build derived the reverse CSR from the forward rows (a fully mirrored edge table)."""
        d = C.c_int()
        self.gg._chk(self.gg.lib.gg_debug_csr_reverse(self.handle, None, None, None, C.byref(d)))
        return d.value

    @property
    def reverse_rows_ready(self) -> bool:
        """True if the reverse rows (rnbr) are written; asking does not write them (gg_debug_csr_reverse_ready)."""
        r = C.c_int()
        self.gg._chk(self.gg.lib.gg_debug_csr_reverse_ready(self.handle, C.byref(r)))
        return bool(r.value)

    @property
    def reverse_index_ready(self) -> bool:
        """True if the row index of the reverse entries (rrow) is written; asking does not write it
        (gg_debug_csr_reverse_index_ready)."""
        r = C.c_int()
        self.gg._chk(self.gg.lib.gg_debug_csr_reverse_index_ready(self.handle, C.byref(r)))
        return bool(r.value)

    def export_reverse_index(self):
        """rrow alone: builds the offsets and the row index if absent, not the reverse rows."""
        p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))  # noqa: E731
        roff = np.empty(self.V + 1, np.int64)
        self.gg._chk(self.gg.lib.gg_debug_csr_reverse(self.handle, p(roff), None, None, None))
        rrow = np.empty(int(roff[-1]), np.int64)
        self.gg._chk(self.gg.lib.gg_debug_csr_reverse(self.handle, None, None, p(rrow), None))
        return rrow

    def export_reverse(self):
        """(roff, rnbr, rrow) of the reverse CSR as int64 arrays (gg_debug_csr_reverse)."""
        p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))  # noqa: E731
        roff = np.empty(self.V + 1, np.int64)
        self.gg._chk(self.gg.lib.gg_debug_csr_reverse(self.handle, p(roff), None, None, None))
        rnbr = np.empty(int(roff[-1]), np.int64)  # (a shard keeps the edges whose DESTINATION it owns here)
        rrow = np.empty(int(roff[-1]), np.int64)
        self.gg._chk(self.gg.lib.gg_debug_csr_reverse(self.handle, None, p(rnbr), p(rrow), None))
        return roff, rnbr, rrow

    def close(self):
        if self.handle:
            self.gg.lib.gg_csr_destroy(self.handle)
            self.handle = None


class GG:
    """One gg_ctx.  Mirrors the call sequence of the C++ operators: append (Sink) -> build (Finalize)
    -> expand / bfs (GetData)."""

    def __init__(self, device: int = 0, chunk_rows: int = 0):
        self.lib = load_library()
        h = C.c_void_p()
        self._chk(self.lib.gg_ctx_create(device, C.byref(h)))
        self.ctx = h
        self.chunk_rows = chunk_rows  # >0: append in DataChunk-sized pieces like the Sink would

    def _chk(self, rc: int):
        if rc != 0:
            raise GGError(rc, self.lib.gg_last_error().decode())

    def close(self):
        if self.ctx:
            self.lib.gg_ctx_destroy(self.ctx)
            self.ctx = None

    # ---- staging
    def append_vertices(self, ids):
        a, p = _i64(ids)
        step = self.chunk_rows or max(1, a.size)
        for o in range(0, a.size, step):
            n = min(step, a.size - o)
            self._chk(self.lib.gg_vertices_append(self.ctx, C.cast(C.addressof(p.contents) + 8 * o, C.POINTER(C.c_int64)), n))

    def append_edges(self, src, dst, rowid=None):
        s, ps = _i64(src)
        d, pd = _i64(dst)
        assert s.size == d.size
        if rowid is not None:
            r, pr = _i64(rowid)
        step = self.chunk_rows or max(1, s.size)
        i64p = C.POINTER(C.c_int64)
        for o in range(0, s.size, step):
            n = min(step, s.size - o)
            a = C.cast(C.addressof(ps.contents) + 8 * o, i64p)
            b = C.cast(C.addressof(pd.contents) + 8 * o, i64p)
            c = C.cast(C.addressof(pr.contents) + 8 * o, i64p) if rowid is not None else None
            self._chk(self.lib.gg_edges_append(self.ctx, a, b, c, n))

    def staging_sync(self):
        self._chk(self.lib.gg_staging_sync(self.ctx))

    def staging_clear(self):
        self._chk(self.lib.gg_staging_clear(self.ctx))

    def staging_counts(self):
        a, b = C.c_uint64(), C.c_uint64()
        self._chk(self.lib.gg_staging_counts(self.ctx, C.byref(a), C.byref(b)))
        return a.value, b.value

    # ---- build
    def build_csr(self) -> Csr:
        h = C.c_void_p()
        self._chk(self.lib.gg_csr_build(self.ctx, C.byref(h)))
        return Csr(self, h)

    def set_edge_rowid(self, keep: bool):
        self._chk(self.lib.gg_ctx_set_edge_rowid(self.ctx, int(keep)))

    def build_csr_shard(self, part: int, n_parts: int) -> Csr:
        h = C.c_void_p()
        self._chk(self.lib.gg_csr_build_shard(self.ctx, part, n_parts, C.byref(h)))
        return Csr(self, h)

    # ---- k-hop
    @staticmethod
    def _stats_dict(st: KhopStats):
        return {
            "rows": list(st.rows),
            "digest": list(st.digest),
            "traversed_edges": st.traversed_edges,
            "frontier_entries": st.frontier_entries,
        }

    def _collect(self, res, k_min, k_max):
        out = {}
        try:
            for h in range(k_min, k_max + 1):
                n = C.c_uint64()
                self._chk(self.lib.gg_result_rows(res, h, C.byref(n)))
                table = np.empty((n.value, h + 1), np.int64)
                bufs = [np.empty(GG_CHUNK_ROWS, np.int64) for _ in range(h + 1)]
                ptrs = (C.POINTER(C.c_int64) * (h + 1))(*[b.ctypes.data_as(C.POINTER(C.c_int64)) for b in bufs])
                got = C.c_uint32()
                o = 0
                while o < n.value:  # <=1024-row slices: one DataChunk per fetch
                    self._chk(self.lib.gg_result_fetch(res, h, o, GG_CHUNK_ROWS, ptrs, C.byref(got)))
                    for c in range(h + 1):
                        table[o : o + got.value, c] = bufs[c][: got.value]
                    o += got.value
                out[h] = table
        finally:
            self.lib.gg_result_destroy(res)
        return out

    def expand_khop(self, csr: Csr, k_min: int, k_max: int, sources=None, materialise=False):
        st = KhopStats()
        res = C.c_void_p()
        if sources is None:
            rc = self.lib.gg_expand_khop(self.ctx, csr.handle, None, 0, k_min, k_max, int(materialise), C.byref(st), C.byref(res))
        else:
            a, p = _i64(sources)
            rc = self.lib.gg_expand_khop(self.ctx, csr.handle, p, a.size, k_min, k_max, int(materialise), C.byref(st), C.byref(res))
        self._chk(rc)
        d = self._stats_dict(st)
        if materialise:
            d["tables"] = self._collect(res, k_min, k_max)
        return d

    def expand_khop_dev(self, csr: Csr, k_min: int = 1) -> "DeviceWords":
        """All-sources 1..2-hop count + digest with the six result words left on the device (sharding.FIELDS order);
        nothing waits.  The returned view is valid until the next such call on this context."""
        ptr = C.c_void_p()
        self._chk(self.lib.gg_expand_khop_dev(self.ctx, csr.handle, k_min, C.byref(ptr)))
        return DeviceWords(ptr.value, 6)

    def stream_wait(self, other_stream: int, direction: int = 0):
        """direction 0: `other_stream` (raw hipStream_t, e.g. torch.cuda.current_stream().cuda_stream) waits for the
        library's stream; 1: the library's stream waits for it.  No host synchronisation."""
        self._chk(self.lib.gg_stream_wait(self.ctx, C.c_void_p(other_stream), direction))

    def join_probe(self, csr: Csr, keys) -> np.ndarray:
        """(position in `keys`, rowid) for every edge row whose source equals keys[position] (gg_join_probe)."""
        a, p = _i64(keys)
        m, res = C.c_uint64(), C.c_void_p()
        self._chk(self.lib.gg_join_probe(self.ctx, csr.handle, p, a.size, C.byref(m), C.byref(res)))
        out = np.empty((m.value, 2), np.int64)
        bufs = [np.empty(GG_CHUNK_ROWS, np.int64) for _ in range(2)]
        ptrs = (C.POINTER(C.c_int64) * 2)(*[b.ctypes.data_as(C.POINTER(C.c_int64)) for b in bufs])
        got, o = C.c_uint32(), 0
        try:
            while o < m.value:
                self._chk(self.lib.gg_result_fetch(res, 1, o, GG_CHUNK_ROWS, ptrs, C.byref(got)))
                out[o:o + got.value, 0] = bufs[0][:got.value]
                out[o:o + got.value, 1] = bufs[1][:got.value]
                o += got.value
        finally:
            self.lib.gg_result_destroy(res)
        return out

    def khop_count(self, csr: Csr, k_min: int, k_max: int, sources=None) -> list:
        """Number of h-hop walks per length (index h), from degrees: no row, no digest (gg_khop_count)."""
        rows = (C.c_uint64 * (GG_MAX_HOPS + 1))()
        if sources is None:
            self._chk(self.lib.gg_khop_count(self.ctx, csr.handle, None, 0, k_min, k_max, rows))
        else:
            a, p = _i64(sources)
            self._chk(self.lib.gg_khop_count(self.ctx, csr.handle, p, a.size, k_min, k_max, rows))
        return list(rows)

    def expand_khop_result(self, csr: Csr, k: int, sources=None, k_min: int | None = None) -> KhopResult:
        """k-hop walks from `sources` (None: all vertices) materialised in HBM; nothing crosses PCIe.  k_min: also the
        tables of k_min..k - 1 hops."""
        st = KhopStats()
        res = C.c_void_p()
        if sources is None:
            sp, ns = None, 0
        else:
            a, sp = _i64(sources)
            ns = a.size
        self._chk(self.lib.gg_expand_khop_result(self.ctx, csr.handle, sp, ns, k if k_min is None else k_min, k,
                                                 C.byref(st), C.byref(res)))
        return KhopResult(self, res, self._stats_dict(st))

    def expand_khop_edges(self, csr: Csr, k: int, sources=None) -> "KhopResult":
        """k-hop walks with the rowid of every edge taken (sources None: from every vertex)."""
        st = KhopStats()
        res = C.c_void_p()
        if sources is None:
            sp, ns = None, 0
        else:
            a, sp = _i64(sources)
            ns = a.size
        self._chk(self.lib.gg_expand_khop_edges(self.ctx, csr.handle, sp, ns, k, C.byref(st), C.byref(res)))
        return KhopResult(self, res, self._stats_dict(st))

    def staging_clear_edges(self):
        self._chk(self.lib.gg_staging_clear_edges(self.ctx))

    def vertices_from_edges(self, keep_staged: bool = False) -> int:
        """Vertex table := distinct endpoint ids of the staged edges (keep_staged: united with the ids
        already staged as vertices), ascending; returns their number."""
        n = C.c_uint64()
        self._chk(self.lib.gg_vertices_from_edges(self.ctx, int(keep_staged), C.byref(n)))
        return int(n.value)

    def connected_paths_same_neighbour(self, path_csr: Csr, filter_csr: Csr, hops: int, sources=None):
        """`hops`-hop walks over path_csr whose vertices all share a neighbour in filter_csr; rows (w, v0..vh)."""
        st = KhopStats()
        res, out = C.c_void_p(), C.c_void_p()
        if sources is None:
            sp, ns = None, 0
        else:
            a, sp = _i64(sources)
            ns = a.size
        self._chk(self.lib.gg_expand_khop_result(self.ctx, path_csr.handle, sp, ns, hops, hops, C.byref(st), C.byref(res)))
        try:
            self._chk(self.lib.gg_result_filter_common_neighbour(self.ctx, res, hops, filter_csr.handle, C.byref(out)))
        finally:
            self.lib.gg_result_destroy(res)
        return self._collect(out, hops + 1, hops + 1)[hops + 1]

    def filter_edge(self, res: KhopResult, hops: int, csr: Csr, from_col: int, to_col: int, mode: str = "inner",
                    materialise: bool = True):
        """gg_result_filter_edge: the rows of res's `hops`-hop table by the number m of edge rows v_from_col -> v_to_col
        in csr — "inner": m copies, "semi": the row if m > 0, "anti": the row if m == 0; input order is kept.  Returns
        {"rows_in", "rows_out", "matches"}; with materialise, (that dict, KhopResult whose table `hops` holds the rows —
        the caller closes it)."""
        if mode not in EDGE_MODES:
            raise ValueError(f"mode {mode!r}: one of {sorted(EDGE_MODES)}")
        st, out = EdgeFilterStats(), C.c_void_p()
        self._chk(self.lib.gg_result_filter_edge(self.ctx, res.handle, hops, csr.handle, from_col, to_col,
                                                 EDGE_MODES[mode], int(materialise), C.byref(st), C.byref(out)))
        d = {"rows_in": int(st.rows_in), "rows_out": int(st.rows_out), "matches": int(st.matches)}
        return (d, KhopResult(self, out, d)) if materialise else d

    def extend_edge(self, res: KhopResult, hops: int, csr: Csr, from_col: int, edges: bool = False,
                    materialise: bool = True):
        """gg_result_extend_edge: every row of res's `hops`-hop table joined with the edge rows of csr whose source is the
        row's cell in from_col — one output row (v0..v_hops, w) per such edge row, input order kept, the copies of a row in
        CSR order.  edges: the output carries e1..e_{hops+1} (fetch_edges), the last being the joined row's rowid.  Returns
        {"rows_in", "rows_out", "rows_matched"}; with materialise, (that dict, KhopResult whose table hops + 1 holds the
        rows — the caller closes it)."""
        st, out = ExtendStats(), C.c_void_p()
        self._chk(self.lib.gg_result_extend_edge(self.ctx, res.handle, hops, csr.handle, from_col, int(edges),
                                                 int(materialise), C.byref(st), C.byref(out)))
        d = {"rows_in": int(st.rows_in), "rows_out": int(st.rows_out), "rows_matched": int(st.rows_matched)}
        return (d, KhopResult(self, out, d)) if materialise else d

    def debug_extend(self, tile_rows: int = 0):
        """Output rows per workgroup of extend_edge's write pass (0: the default).  Results must not depend on it."""
        self._chk(self.lib.gg_debug_extend(self.ctx, int(tile_rows)))

    def group_by(self, res: KhopResult, hops: int, key_col: int, key_csr: Csr, weight_col=None, weight_csr=None,
                 weights=None, fetch: bool = True) -> "KhopAggregate":
        """gg_result_group_by: the rows of res's `hops`-hop table grouped by column key_col, whose cells are vertices of
        key_csr (other rows form no group): per key one row (vertex id, walks = its rows, total = the sum of
        weights[vertex of weight_csr (None: key_csr) in column weight_col]; without weights total == walks), ascending by
        dense index in key_csr.  weights: V(weight_csr) integers in vertex-table order.  The answer is a KhopAggregate of
        the one level `hops` (khop_aggregate_top orders it); stats: {"rows_in", "rows_grouped", "groups", "route"}.
        fetch=False: the stats only, nothing is kept on the device."""
        wcsr = weight_csr if weight_csr is not None else key_csr
        wp = None
        if weights is not None:
            w, wp = _i64(weights)
            if w.ndim != 1 or w.size != wcsr.V:
                raise ValueError(f"weights: {w.size} entries for {wcsr.V} vertices")
        st, out = GroupStats(), C.c_void_p()
        self._chk(self.lib.gg_result_group_by(self.ctx, res.handle, hops, key_col, key_csr.handle,
                                              -1 if weight_col is None else int(weight_col),
                                              weight_csr.handle if weight_csr is not None else None, wp, C.byref(st),
                                              C.byref(out) if fetch else None))
        d = {"rows_in": int(st.rows_in), "rows_grouped": int(st.rows_grouped), "groups": int(st.groups),
             "route": int(st.route)}
        return KhopAggregate(self, out if fetch else None, d)

    def debug_group(self, route: int = 0, lds_keys: int = 0):
        """group_by accumulates in the workgroup-private LDS table where it fits (1) or in the global cells (2); lds_keys
        shrinks the keys that table may hold (0: the defaults).  Results must not depend on it."""
        self._chk(self.lib.gg_debug_group(self.ctx, int(route), int(lds_keys)))

    @staticmethod
    def _value_args(value_csr: Csr, values, valid):
        """(values array, its pointer, valid array, its pointer or None) for the value calls; the arrays must outlive the
        call"""
        v, vp = _i64(values)
        if v.ndim != 1 or v.size != value_csr.V:
            raise ValueError(f"values: {v.size} entries for {value_csr.V} vertices")
        b, bp = None, None
        if valid is not None:
            b = np.ascontiguousarray(valid, dtype=np.uint64)
            if b.ndim != 1 or b.size != (value_csr.V + 63) // 64:
                raise ValueError(f"valid: {b.size} words for {value_csr.V} vertices")
            bp = b.ctypes.data_as(C.POINTER(C.c_uint64))
        return v, vp, b, bp

    def filter_value(self, res: KhopResult, hops: int, value_col: int, value_csr: Csr, values, valid=None,
                     lo: int = INT64_MIN, hi: int = INT64_MAX, mode: str = "in", materialise: bool = True):
        """gg_result_filter_value: the rows of res's `hops`-hop table whose value passes — the cell of value_col is a vertex
        d of value_csr, bit d of `valid` (uint64 words; None: every vertex) is set and values[d] lies in [lo, hi] ("in") or
        outside it ("not_in"); rows without a value pass nothing.  Input order and the input's edge columns are kept.
        Returns {"rows_in", "rows_valued", "rows_out"}; with materialise, (that dict, KhopResult whose table `hops` holds
        the rows — the caller closes it)."""
        if mode not in VALUE_MODES:
            raise ValueError(f"mode {mode!r}: one of {sorted(VALUE_MODES)}")
        v, vp, b, bp = self._value_args(value_csr, values, valid)
        st, out = ValueFilterStats(), C.c_void_p()
        self._chk(self.lib.gg_result_filter_value(self.ctx, res.handle, hops, value_col, value_csr.handle, vp, bp, int(lo),
                                                  int(hi), VALUE_MODES[mode], int(materialise), C.byref(st), C.byref(out)))
        d = {"rows_in": int(st.rows_in), "rows_valued": int(st.rows_valued), "rows_out": int(st.rows_out)}
        return (d, KhopResult(self, out, d)) if materialise else d

    def top_rows(self, res: KhopResult, hops: int, value_col: int, value_csr: Csr, values, n: int, valid=None,
                 lo: int = INT64_MIN, hi: int = INT64_MAX, mode: str = "in", descending: bool = True, tie_col=None):
        """gg_result_top_rows: the best n of the rows filter_value would keep, in rank order — by value (descending or
        ascending, signed), then by the cell of tie_col ascending (None: no tie column), then by input row.  Returns
        ({"rows_in", "rows_valued", "candidates", "rows_out", "select_passes", "sort_route"}, KhopResult whose table `hops`
        holds the min(n, candidates) rows and the input's edge columns — the caller closes it)."""
        if mode not in VALUE_MODES:
            raise ValueError(f"mode {mode!r}: one of {sorted(VALUE_MODES)}")
        v, vp, b, bp = self._value_args(value_csr, values, valid)
        st, out = ValueTopStats(), C.c_void_p()
        self._chk(self.lib.gg_result_top_rows(self.ctx, res.handle, hops, value_col, value_csr.handle, vp, bp, int(lo),
                                              int(hi), VALUE_MODES[mode], 1 if descending else 0,
                                              -1 if tie_col is None else int(tie_col), int(n), C.byref(st), C.byref(out)))
        d = {f: int(getattr(st, f)) for f, _ in ValueTopStats._fields_}
        return d, KhopResult(self, out, d)

    def debug_value_top(self, sort_route: int = 0, candidate_floor: int = 0):
        """top_rows orders its survivors in LDS (1) or by the global passes (2) and compacts the selection's candidates at
        candidate_floor or fewer (0: the defaults).  Results must not depend on it."""
        self._chk(self.lib.gg_debug_value_top(self.ctx, int(sort_route), int(candidate_floor)))

    def distinct(self, res: KhopResult, hops: int, cols, materialise: bool = True):
        """gg_result_distinct: SELECT DISTINCT over the columns `cols` (pairwise different numbers in 0..hops, in output
        order) of res's `hops`-hop table.  Cells are compared as raw int64 values.  One row per distinct tuple — the first
        input row that holds it — in input order.  Returns {"rows_in", "rows_out", "slots", "probe_steps"}; with
        materialise, (that dict, KhopResult whose table len(cols) - 1 holds the rows — the caller closes it)."""
        cs = [int(c) for c in cols]
        arr = (C.c_int * max(len(cs), 1))(*cs)
        st, out = DistinctStats(), C.c_void_p()
        self._chk(self.lib.gg_result_distinct(self.ctx, res.handle, hops, arr, len(cs), int(materialise), C.byref(st),
                                              C.byref(out) if materialise else None))
        d = {f: int(getattr(st, f)) for f, _ in DistinctStats._fields_}
        return (d, KhopResult(self, out, d)) if materialise else d

    def debug_distinct(self, slots: int = 0, combine: int = 0):
        """distinct uses a table of `slots` slots (0: the default; rounded up to a power of two above the row count) and,
        with combine = 1, never combines adjacent equal lanes.  Results must not depend on it."""
        self._chk(self.lib.gg_debug_distinct(self.ctx, int(slots), int(combine)))

    def group_tuples(self, res: KhopResult, hops: int, cols, value_col=None, value_csr=None, values=None, valid=None,
                     fetch: bool = True) -> "TupleGroups":
        """gg_result_group_tuples: GROUP BY the columns `cols` (as distinct's) of res's `hops`-hop table, cells compared as
        raw int64 values: per distinct tuple count(*), and over the value of a row (filter_value's: the cell of value_col
        looked up in value_csr, values, valid) count(x), sum(x) as a Python int mod 2^128, min(x) and max(x).  value_col
        None: the count form, the value columns are 0.  The answer is a TupleGroups whose rows are distinct's rows in
        distinct's order; fetch=False: the stats only, nothing is kept on the device."""
        cs = [int(c) for c in cols]
        arr = (C.c_int * max(len(cs), 1))(*cs)
        v, vp, b, bp = (None, None, None, None)
        if value_col is not None:
            v, vp, b, bp = self._value_args(value_csr, values, valid)
        elif value_csr is not None or values is not None or valid is not None:
            raise ValueError("value_csr, values and valid go with a value column")
        st, out = GroupTuplesStats(), C.c_void_p()
        self._chk(self.lib.gg_result_group_tuples(self.ctx, res.handle, hops, arr, len(cs),
                                                  -1 if value_col is None else int(value_col),
                                                  value_csr.handle if value_csr is not None else None, vp, bp,
                                                  C.byref(st), C.byref(out) if fetch else None))
        d = {f: int(getattr(st, f)) for f, _ in GroupTuplesStats._fields_}
        return TupleGroups(self, out if fetch else None, d)

    def debug_group_tuples(self, route: int = 0, lds_groups: int = 0):
        """group_tuples accumulates in the workgroup-private LDS cells where the groups fit (1) or in the global cells (2);
        lds_groups shrinks the groups those cells may hold (0: the defaults).  Results must not depend on it."""
        self._chk(self.lib.gg_debug_group_tuples(self.ctx, int(route), int(lds_groups)))

    def closed_walks(self, csr: Csr, k: int, sources=None, materialise: bool = True):
        """Closed walks of k edges v0 -> v1 -> ... -> v_{k-1} -> v0 with v0 from `sources` (None: every vertex), as rows
        (v0..v_{k-1}): the (k - 1)-hop walks whose last vertex has an edge row back to the first, one row per such edge
        row.  2 <= k <= GG_MAX_HOPS + 1.  Returns what filter_edge returns."""
        if not 2 <= k <= GG_MAX_HOPS + 1:
            raise ValueError(f"closed walks of {k} edges: need 2 <= k <= {GG_MAX_HOPS + 1}")
        walks = self.expand_khop_result(csr, k - 1, sources)
        try:
            return self.filter_edge(walks, k - 1, csr, k - 1, 0, "inner", materialise)
        finally:
            walks.close()

    def expand_khop_range(self, csr: Csr, lo: int, hi: int, k_min: int, k_max: int, materialise=False):
        st = KhopStats()
        res = C.c_void_p()
        self._chk(self.lib.gg_expand_khop_range(self.ctx, csr.handle, lo, hi, k_min, k_max, int(materialise), C.byref(st), C.byref(res)))
        d = self._stats_dict(st)
        if materialise:
            d["tables"] = self._collect(res, k_min, k_max)
        return d

    def expand_khop_mid(self, csr: Csr, lo: int, hi: int, k_min: int = 1, k_max: int = 2):
        st = KhopStats()
        self._chk(self.lib.gg_expand_khop_mid(self.ctx, csr.handle, lo, hi, k_min, k_max, C.byref(st)))
        return self._stats_dict(st)

    def expand_khop_mid_result(self, csr: Csr, lo: int, hi: int, k_min: int = 2, with_stats: bool = True) -> "KhopResult":
        """The 2-hop rows (k_min == 1: also the 1-hop rows) with the middle vertex in [lo, hi), materialised in HBM.
        with_stats=False: no counting expansion (count + digest) in front of the rows; KhopResult.rows() still works."""
        st = KhopStats()
        res = C.c_void_p()
        self._chk(self.lib.gg_expand_khop_mid_result(self.ctx, csr.handle, lo, hi, k_min,
                                                     C.byref(st) if with_stats else None, C.byref(res)))
        return KhopResult(self, res, self._stats_dict(st) if with_stats else None)

    def khop_partition_mid(self, csr: Csr, n_parts: int):
        b = (C.c_uint64 * (n_parts + 1))()
        self._chk(self.lib.gg_khop_partition_mid(self.ctx, csr.handle, n_parts, b))
        return list(b)

    def force_frontier(self, on):
        """False / 0: normal; True / 1: frontier kernels only; 2 / 3: the product form of an explicit frontier's last hop /
        last two hops at any size (and no all-sources product kernels)."""
        self._chk(self.lib.gg_debug_force_frontier(self.ctx, int(on)))

    def scan_fault(self, spin_limit: int = 0, mute_tile: int = (1 << 64) - 1):
        self._chk(self.lib.gg_debug_scan_fault(self.ctx, spin_limit, mute_tile))

    def debug_scan(self, values: np.ndarray, in_place: bool = False):
        """(exclusive prefix, total) of a uint32 / uint64 array by the library's shared scan (gg_debug_scan); the prefix
        has the input's type (uint32: mod 2^32), the total is exact.  in_place: the device scans over its input."""
        a = np.ascontiguousarray(values)
        assert a.dtype in (np.uint32, np.uint64) and a.ndim == 1
        out = a.copy() if in_place else np.empty_like(a)
        src = out if in_place else a
        total = C.c_uint64()
        self._chk(self.lib.gg_debug_scan(self.ctx, src.ctypes.data, a.size, a.dtype.itemsize, out.ctypes.data,
                                         C.byref(total)))
        return out, int(total.value)

    def debug_sort_pairs(self, key, a, b=None, key_bits: int = 31):
        """(key_out, a_out, b_out or None, n_valid) of the library's shared stable radix sort (gg_debug_sort_pairs): the
        first n_valid outputs are the elements whose key is not 0xFFFFFFFF, sorted stably by key; the rest hold
        SORT_PREFILL."""
        cols = [np.ascontiguousarray(c, dtype=np.uint32) for c in (key, a) + (() if b is None else (b,))]
        n = cols[0].size
        assert all(c.ndim == 1 and c.size == n for c in cols)
        outs = [np.zeros(n, np.uint32) for _ in cols]
        ptr = lambda arrs: [x.ctypes.data for x in arrs] + [None] * (3 - len(arrs))
        n_valid = C.c_uint64()
        self._chk(self.lib.gg_debug_sort_pairs(self.ctx, *ptr(cols), n, int(key_bits), *ptr(outs), C.byref(n_valid)))
        return outs[0], outs[1], (outs[2] if b is not None else None), int(n_valid.value)

    def rank_mode(self, mode: int):
        """0: probe the LDS atomic order once (default), 1: ranks from ds_add_rtn, 2: ranks from match masks."""
        self._chk(self.lib.gg_debug_rank_mode(self.ctx, int(mode)))

    def force_legacy_build(self, on: bool):
        self._chk(self.lib.gg_debug_force_legacy_build(self.ctx, int(on)))

    def max_grid_tiles(self, n: int = 0):
        """Expansion launches of at most n workgroups (0: the hardware bound)."""
        self._chk(self.lib.gg_debug_max_grid_tiles(self.ctx, int(n)))

    def debug_reset(self):
        """Every testing knob and the edge-rowid switch back to its default."""
        self._chk(self.lib.gg_debug_reset(self.ctx))

    def placement(self):
        """(column sets placed by probing, fast pairs of the last set: 3 = each result column in its own memory rank)."""
        a, b = C.c_uint64(), C.c_uint64()
        self._chk(self.lib.gg_debug_placement(self.ctx, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def pool(self):
        """(blocks the device pool holds, blocks handed out right now) (gg_debug_pool)."""
        a, b = C.c_uint64(), C.c_uint64()
        self._chk(self.lib.gg_debug_pool(self.ctx, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def pool_fill(self):
        """(the byte GG_POOL_FILL gave this context or -1, blocks filled, bytes filled since it was created)
        (gg_debug_pool_fill)."""
        f, a, b = C.c_int(), C.c_uint64(), C.c_uint64()
        self._chk(self.lib.gg_debug_pool_fill(self.ctx, C.byref(f), C.byref(a), C.byref(b)))
        return int(f.value), int(a.value), int(b.value)

    def khop_partition(self, csr: Csr, n_parts: int):
        b = (C.c_uint64 * (n_parts + 1))()
        self._chk(self.lib.gg_khop_partition(self.ctx, csr.handle, n_parts, b))
        return list(b)

    # ---- bfs
    def bfs64(self, csr: Csr, sources, max_hops: int, targets=None, fetch=True):
        s, ps = _i64(sources)
        n_out = csr.V if targets is None else len(targets)
        st = BfsStats()
        if not fetch:  # stats only: distances stay on the device
            self._chk(self.lib.gg_bfs64(self.ctx, csr.handle, ps, s.size, max_hops, None, 0, None, C.byref(st)))
            return None, {"levels": st.levels, "traversed_edges": st.traversed_edges,
                          "active_vertices": st.active_vertices, "reached_pairs": st.reached_pairs}
        out = np.empty((s.size, n_out), np.int32)
        if targets is None:
            rc = self.lib.gg_bfs64(self.ctx, csr.handle, ps, s.size, max_hops, None, 0, out.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(st))
        else:
            t, pt = _i64(targets)
            rc = self.lib.gg_bfs64(self.ctx, csr.handle, ps, s.size, max_hops, pt, t.size, out.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(st))
        self._chk(rc)
        return out, {"levels": st.levels, "traversed_edges": st.traversed_edges, "active_vertices": st.active_vertices, "reached_pairs": st.reached_pairs}

    def debug_bfs_steps(self):
        """The last 64-lane BFS of this context as its levels recorded it (gg_debug_bfs_steps): a dict of `steps`, a
        uint64 array [entries, 4] of (n_active, te, reached, cur) for the seed and every level that ran (no entries: no
        BFS since the last reset), `levels` = entries - 1, `cell_bytes` and `pull_factor`."""
        n, cell, factor = C.c_uint64(), C.c_int(), C.c_int()
        self._chk(self.lib.gg_debug_bfs_steps(self.ctx, None, 0, C.byref(n), None, None))
        steps = np.zeros((int(n.value), 4), np.uint64)
        self._chk(self.lib.gg_debug_bfs_steps(self.ctx, steps.ctypes.data_as(C.POINTER(C.c_uint64)), steps.shape[0],
                                              C.byref(n), C.byref(cell), C.byref(factor)))
        assert int(n.value) == steps.shape[0]
        return {"steps": steps, "levels": steps.shape[0] - 1, "cell_bytes": int(cell.value),
                "pull_factor": int(factor.value)}

    def lookup(self, csr: Csr, ids) -> np.ndarray:
        """Dense index of each id (uint32, 0xFFFFFFFF = not a vertex)."""
        a, pa = _i64(ids)
        out = np.empty(a.size, np.uint32)
        self._chk(self.lib.gg_csr_lookup(self.ctx, csr.handle, pa, a.size, out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    def host_buffer(self, n_int64: int) -> np.ndarray:
        """An int64 array in page-locked memory owned by the context (for gg_result_fetch at PCIe rate)."""
        p = C.c_void_p()
        self._chk(self.lib.gg_host_alloc(self.ctx, 8 * max(1, n_int64), C.byref(p)))
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int64)), shape=(max(1, n_int64),))[:n_int64]

    def bfs64_pairs_packed(self, csr: Csr, sources, max_hops: int) -> np.ndarray:
        """gg_bfs64_pairs_packed: one word per reached pair, lane << 58 | distance << 32 | dense vertex index."""
        i64p = C.POINTER(C.c_int64)
        s, ps = _i64(sources)
        st, res = BfsStats(), C.c_void_p()
        self._chk(self.lib.gg_bfs64_pairs_packed(self.ctx, csr.handle, ps, s.size, max_hops, C.byref(st), C.byref(res)))
        try:
            n = C.c_uint64()
            self._chk(self.lib.gg_result_rows(res, 0, C.byref(n)))
            out = np.empty(n.value, np.int64)
            if n.value:
                ptrs = (i64p * 1)(out.ctypes.data_as(i64p))
                got = C.c_uint32()
                self._chk(self.lib.gg_result_fetch(res, 0, 0, n.value, ptrs, C.byref(got)))
        finally:
            self.lib.gg_result_destroy(res)
        return out.view(np.uint64)

    def bfs64_pairs(self, csr: Csr, sources, max_hops: int):
        """Reached (source id, vertex id, distance) rows of one <=64-source batch, compacted on the device."""
        i64p = C.POINTER(C.c_int64)
        s, ps = _i64(sources)
        st, res = BfsStats(), C.c_void_p()
        self._chk(self.lib.gg_bfs64_pairs(self.ctx, csr.handle, ps, s.size, max_hops, C.byref(st), C.byref(res)))
        try:
            n = C.c_uint64()
            self._chk(self.lib.gg_result_rows(res, 2, C.byref(n)))
            out = np.empty((3, n.value), np.int64)
            if n.value:
                ptrs = (i64p * 3)(*[out[c].ctypes.data_as(i64p) for c in range(3)])
                got = C.c_uint32()
                self._chk(self.lib.gg_result_fetch(res, 2, 0, n.value, ptrs, C.byref(got)))  # one bulk copy
                assert got.value == n.value
        finally:
            self.lib.gg_result_destroy(res)
        return out.T.copy(), {"levels": st.levels, "traversed_edges": st.traversed_edges,
                              "active_vertices": st.active_vertices, "reached_pairs": st.reached_pairs}

    def bfs64_paths(self, csr: Csr, sources, pair_lane, pair_dst, max_hops: int = -1, edges: bool = True):
        """gg_bfs64_paths: the pinned shortest path of each (sources[pair_lane[i]], pair_dst[i]) of one <=64-source batch,
        unnested: (pair_index int64, step int32, vertex int64, edge int64) arrays ascending by (pair, step), and the
        BFS's statistics."""
        i64p, i32p = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
        s, ps = _i64(sources)
        d, pd = _i64(pair_dst)
        lane = np.ascontiguousarray(pair_lane, dtype=np.uint32)
        if lane.size != d.size:
            raise ValueError("one source lane per target")
        st, res = BfsStats(), C.c_void_p()
        self._chk(self.lib.gg_bfs64_paths(self.ctx, csr.handle, ps, s.size, int(max_hops),
                                          lane.ctypes.data_as(C.POINTER(C.c_uint32)), pd, d.size, 1 if edges else 0,
                                          C.byref(st), C.byref(res)))
        try:
            n = C.c_uint64()
            self._chk(self.lib.gg_bfs64_paths_rows(res, C.byref(n)))
            n = int(n.value)
            pair, step = np.empty(n, np.int64), np.empty(n, np.int32)
            vtx, edge = np.empty(n, np.int64), np.empty(n, np.int64)
            done = 0
            while done < n:
                got = C.c_uint32()
                self._chk(self.lib.gg_bfs64_paths_fetch(
                    res, done, min(n - done, 1 << 30), pair[done:].ctypes.data_as(i64p), step[done:].ctypes.data_as(i32p),
                    vtx[done:].ctypes.data_as(i64p), edge[done:].ctypes.data_as(i64p), C.byref(got)))
                assert got.value
                done += got.value
        finally:
            self.lib.gg_result_destroy(res)
        return (pair, step, vtx, edge), {"levels": st.levels, "traversed_edges": st.traversed_edges,
                                         "active_vertices": st.active_vertices, "reached_pairs": st.reached_pairs}

    def shortest_paths(self, csr: Csr, src, dst, max_hops: int = -1, edges: bool = True):
        """The pinned shortest path (include/gg.h, gg_bfs64_paths) of every pair (src[i], dst[i]), unnested: arrays
        (pair_index int64, step int32, vertex int64, edge int64), one row per step 0..d of every pair that has a path of at
        most max_hops edges (max_hops < 0: of any length), ascending by (pair index, step); edge is the rowid of the edge
        into the step's vertex, -1 at step 0 (and everywhere with edges=False).  Any number of pairs: they are grouped by
        source into device batches of at most 64 distinct sources."""
        s, _ = _i64(src)
        d, _ = _i64(dst)
        if s.size != d.size:
            raise ValueError("one target per source")
        uniq, inv = np.unique(s, return_inverse=True)
        parts = []
        for b0 in range(0, uniq.size, GG_BFS_LANES):
            members = np.flatnonzero((inv >= b0) & (inv < b0 + GG_BFS_LANES))  # ascending pair index
            (pair, step, vtx, edge), _ = self.bfs64_paths(csr, uniq[b0:b0 + GG_BFS_LANES], inv[members] - b0, d[members],
                                                          max_hops, edges)
            parts.append((members[pair], step, vtx, edge))
        if not parts:
            return np.empty(0, np.int64), np.empty(0, np.int32), np.empty(0, np.int64), np.empty(0, np.int64)
        pair, step, vtx, edge = (np.concatenate([p[c] for p in parts]) for c in range(4))
        order = np.argsort(pair, kind="stable")  # batches interleave; inside a pair the steps already ascend
        return pair[order], step[order], vtx[order], edge[order]

    def bfs64_all_paths(self, csr: Csr, sources, pair_lane, pair_dst, max_hops: int = -1, path_limit: int = 0,
                        edges: bool = True, materialise: bool = True, fetch: bool = True):
        """gg_bfs64_all_paths: one <=64-source batch.  Returns (table 0, table 1, stats): table 0 = (pair int64, hops int32,
        paths uint64, kept uint64) per reached pair; table 1 = (pair int64, path int64, step int32, vertex int64, edge int64)
        per step of every kept path, ascending by (pair, path, step) — None with materialise=False; stats = the call's
        gg_all_paths_stats as a dict, the BFS's under "bfs".  fetch=False: the stats alone, the tables are made and left on the
        device (benchmarks)."""
        i64p, i32p, u64p = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_uint64)
        s, ps = _i64(sources)
        d, pd = _i64(pair_dst)
        lane = np.ascontiguousarray(pair_lane, dtype=np.uint32)
        if lane.size != d.size:
            raise ValueError("one source lane per target")
        st, res = AllPathsStats(), C.c_void_p()
        self._chk(self.lib.gg_bfs64_all_paths(self.ctx, csr.handle, ps, s.size, int(max_hops),
                                              lane.ctypes.data_as(C.POINTER(C.c_uint32)), pd, d.size, int(path_limit),
                                              1 if edges else 0, 1 if materialise else 0, C.byref(st), C.byref(res)))
        try:
            def fetch_table(table, cols, call):
                n = C.c_uint64()
                self._chk(self.lib.gg_bfs64_all_paths_rows(res, table, C.byref(n)))
                n = int(n.value)
                out = [np.empty(n, t) for t in cols]
                done = 0
                while done < n:
                    got = C.c_uint32()
                    ptrs = [a[done:].ctypes.data_as({np.int64: i64p, np.int32: i32p, np.uint64: u64p}[t])
                            for a, t in zip(out, cols)]
                    self._chk(call(res, done, min(n - done, 1 << 30), *ptrs, C.byref(got)))
                    assert got.value
                    done += got.value
                return tuple(out)
            t0 = t1 = None
            if fetch:
                t0 = fetch_table(0, (np.int64, np.int32, np.uint64, np.uint64), self.lib.gg_bfs64_all_paths_fetch_pairs)
            if fetch and materialise:
                t1 = fetch_table(1, (np.int64, np.int64, np.int32, np.int64, np.int64), self.lib.gg_bfs64_all_paths_fetch)
        finally:
            self.lib.gg_result_destroy(res)
        stats = {k: int(getattr(st, k)) for k in ("pairs_reached", "paths", "paths_kept", "rows", "sigma_entries",
                                                  "sigma_gathered")}
        stats["bfs"] = {"levels": st.bfs.levels, "traversed_edges": st.bfs.traversed_edges,
                        "active_vertices": st.bfs.active_vertices, "reached_pairs": st.bfs.reached_pairs}
        return (t0, t1, stats) if fetch else stats

    def _all_paths_batches(self, src, dst):
        """(sources of the batch, lanes of its pairs, their targets, their pair indices) per batch of 64 distinct sources,
        grouped as shortest_paths groups them"""
        s, _ = _i64(src)
        d, _ = _i64(dst)
        if s.size != d.size:
            raise ValueError("one target per source")
        uniq, inv = np.unique(s, return_inverse=True)
        for b0 in range(0, uniq.size, GG_BFS_LANES):
            members = np.flatnonzero((inv >= b0) & (inv < b0 + GG_BFS_LANES))  # ascending pair index
            yield uniq[b0:b0 + GG_BFS_LANES], inv[members] - b0, d[members], members

    def all_shortest_paths(self, csr: Csr, src, dst, max_hops: int = -1, path_limit: int = 0, edges: bool = True):
        """Every shortest path (include/gg.h, gg_bfs64_all_paths) of every pair (src[i], dst[i]), at most path_limit of a
        pair (0: all), unnested: arrays (pair_index int64, path int64, step int32, vertex int64, edge int64) ascending by
        (pair, path, step).  Any number of pairs, grouped by source into device batches of at most 64 distinct sources."""
        parts = []
        for sources, lanes, targets, members in self._all_paths_batches(src, dst):
            _, t1, _ = self.bfs64_all_paths(csr, sources, lanes, targets, max_hops, path_limit, edges)
            parts.append((members[t1[0]],) + t1[1:])
        if not parts:
            return tuple(np.empty(0, np.int32 if k == 2 else np.int64) for k in range(5))
        cols = [np.concatenate([p[c] for p in parts]) for c in range(5)]
        order = np.argsort(cols[0], kind="stable")  # batches interleave; inside a pair (path, step) already ascend
        return tuple(c[order] for c in cols)

    def shortest_path_counts(self, csr: Csr, src, dst, max_hops: int = -1):
        """(pair_index int64, hops int32, paths uint64) of the pairs that have a path, ascending by pair index; paths is the
        number of shortest paths, 2^64 - 1 standing for that many or more."""
        parts = []
        for sources, lanes, targets, members in self._all_paths_batches(src, dst):
            t0, _, _ = self.bfs64_all_paths(csr, sources, lanes, targets, max_hops, 0, False, materialise=False)
            parts.append((members[t0[0]], t0[1], t0[2]))
        if not parts:
            return np.empty(0, np.int64), np.empty(0, np.int32), np.empty(0, np.uint64)
        cols = [np.concatenate([p[c] for p in parts]) for c in range(3)]
        order = np.argsort(cols[0], kind="stable")
        return tuple(c[order] for c in cols)

    def walk_endpoints(self, csr: Csr, sources, k_max: int):
        """gg_walk_endpoints: (vertex ids, masks) — bit h of a mask: the vertex ends a walk of exactly h edges
        from one of the sources."""
        i64p = C.POINTER(C.c_int64)
        s, ps = _i64(sources)
        res = C.c_void_p()
        self._chk(self.lib.gg_walk_endpoints(self.ctx, csr.handle, ps, s.size, k_max, C.byref(res)))
        try:
            n = C.c_uint64()
            self._chk(self.lib.gg_result_rows(res, 1, C.byref(n)))
            out = np.empty((2, n.value), np.int64)
            if n.value:
                ptrs = (i64p * 2)(*[out[c].ctypes.data_as(i64p) for c in range(2)])
                got = C.c_uint32()
                self._chk(self.lib.gg_result_fetch(res, 1, 0, n.value, ptrs, C.byref(got)))
                assert got.value == n.value
        finally:
            self.lib.gg_result_destroy(res)
        return out[0].copy(), out[1].copy()

    def walk_closure(self, csr: Csr, seeds, max_levels: int | None = None) -> WalkClosure:
        """gg_walk_closure: every walk of >= 1 edges from the seeds (max_levels None: until a level is empty).  The CSR
        must keep edge rowids (the default)."""
        s, ps = _i64(seeds)
        res = C.c_void_p()
        self._chk(self.lib.gg_walk_closure(self.ctx, csr.handle, ps, s.size, -1 if max_levels is None else max_levels,
                                           C.byref(res)))
        return WalkClosure(self, res)

    def reach_closure(self, csr: Csr, seeds, classes, seen=None, n_classes: int | None = None) -> ReachClosure:
        """gg_reach_closure: every (class, vertex) reachable from the seeds (seed i in class classes[i]; seen[i] true:
        its (class, vertex) is visited from the start).  n_classes defaults to max(classes) + 1."""
        s, ps = _i64(seeds)
        c = np.ascontiguousarray(classes, dtype=np.uint32)
        if c.size != s.size:
            raise ValueError("one class per seed")
        m = None
        if seen is not None:
            m = np.ascontiguousarray(seen, dtype=np.uint8)
            if m.size != s.size:
                raise ValueError("one seen flag per seed")
        n = (int(c.max()) + 1 if c.size else 0) if n_classes is None else n_classes
        res = C.c_void_p()
        self._chk(self.lib.gg_reach_closure(self.ctx, csr.handle, ps, c.ctypes.data_as(C.POINTER(C.c_uint32)),
                                            None if m is None else m.ctypes.data_as(C.POINTER(C.c_uint8)), s.size, n,
                                            C.byref(res)))
        return ReachClosure(self, res)

    def debug_reach_visited(self, mode: int = 0, slots: int = 0):
        """gg_reach_closure's visited set: 0 the budget decides, 1 bitmap, 2 hash set (first `slots` slots if != 0)."""
        self._chk(self.lib.gg_debug_reach_visited(self.ctx, int(mode), int(slots)))

    def level_sets(self, csr: Csr, seeds, classes, n_classes: int | None = None, max_levels: int = -1) -> LevelSets:
        """gg_level_sets: for L = 1, 2, ... the set of (class, vertex) that L edges lead to from the seeds (seed i in
        class classes[i]); max_levels < 0: until a level is empty.  n_classes defaults to max(classes) + 1."""
        s, ps = _i64(seeds)
        c = np.ascontiguousarray(classes, dtype=np.uint32)
        if c.size != s.size:
            raise ValueError("one class per seed")
        n = (int(c.max()) + 1 if c.size else 0) if n_classes is None else n_classes
        res = C.c_void_p()
        self._chk(self.lib.gg_level_sets(self.ctx, csr.handle, ps, c.ctypes.data_as(C.POINTER(C.c_uint32)), s.size, n,
                                         int(max_levels), C.byref(res)))
        return LevelSets(self, res)

    def debug_level_sets(self, set_mode: int = 0, order_mode: int = 0):
        """gg_level_sets' per-level set (0 the budget decides, 1 bitmap, 2 hash set) and order route (0 the byte model
        decides, 1 claim and sort, 2 read the rows off the bitmap; not with the hash set)."""
        self._chk(self.lib.gg_debug_level_sets(self.ctx, int(set_mode), int(order_mode)))

    # ---- triangles
    def triangles(self, csr: Csr, sources=None, ordered: bool = False, materialise: bool = False):
        """gg_triangles: the closed 3-edge walks (a, b, c) with a from `sources` (None: every vertex); ordered: only
        id(a) < id(b) < id(c).  Returns {"rows", "digest", "wedges"}; with materialise, (that dict, KhopResult whose
        table 2 holds the rows — the caller closes it)."""
        st, res = TriStats(), C.c_void_p()
        if sources is None:
            sp, ns = None, 0
        else:
            a, sp = _i64(sources)
            ns = a.size
            if ns == 0:  # an empty list, not "every vertex": a non-NULL pointer with n_src = 0
                sp = C.cast((C.c_int64 * 1)(), C.POINTER(C.c_int64))
        self._chk(self.lib.gg_triangles(self.ctx, csr.handle, sp, ns, int(ordered), int(materialise), C.byref(st),
                                        C.byref(res)))
        d = {"rows": int(st.rows), "digest": int(st.digest), "wedges": int(st.wedges)}
        return (d, KhopResult(self, res, d)) if materialise else d

    def triangles_edges(self, csr: Csr, sources=None, ordered: bool = False):
        """gg_triangles_edges: triangles(..., materialise=True) whose result also holds the rowids e1: a -> b, e2: b -> c,
        e3: c -> a of every row (KhopResult.fetch_triangle_edges).  Returns (stats dict, KhopResult — the caller closes
        it)."""
        st, res = TriStats(), C.c_void_p()
        keep, sp, ns = self._triangle_sources(sources)  # (keep: the array sp points into)
        self._chk(self.lib.gg_triangles_edges(self.ctx, csr.handle, sp, ns, int(ordered), C.byref(st), C.byref(res)))
        d = {"rows": int(st.rows), "digest": int(st.digest), "wedges": int(st.wedges)}
        return d, KhopResult(self, res, d)

    @staticmethod
    def _triangle_sources(sources):
        if sources is None:
            return None, None, 0
        a, sp = _i64(sources)
        if a.size == 0:  # an empty list, not "every vertex": a non-NULL pointer with n_src = 0
            sp = C.cast((C.c_int64 * 1)(), C.POINTER(C.c_int64))
        return a, sp, a.size

    # ---- grouped aggregates over walks
    def khop_aggregate(self, csr: Csr, k_min: int, k_max: int, group_by: str = "start", sources=None, weights=None,
                       fetch: bool = True) -> "KhopAggregate":
        """gg_khop_aggregate: count(*) and sum(weight) over the h-hop walks from `sources` (None: every vertex once;
        a list counts with multiplicity), h in k_min..k_max, grouped by their "start" vertex (the sum is over the end
        vertices' weights) or their "end" vertex (over the start vertices').  weights: V integers in vertex-table order
        (None: all 1, total == walks).  fetch=False: the stats only, nothing is kept on the device."""
        if group_by not in GROUP_BY:
            raise ValueError(f"group_by {group_by!r}: one of {sorted(GROUP_BY)}")
        wp = None
        if weights is not None:
            w, wp = _i64(weights)
            if w.ndim != 1 or w.size != csr.V:
                raise ValueError(f"weights: {w.size} entries for {csr.V} vertices")
        if sources is None:
            sp, ns = None, 0
        else:
            a = np.ascontiguousarray(sources, dtype=np.int64).reshape(-1)
            keep = a if a.size else np.zeros(1, np.int64)  # (an empty list is a list: the pointer must not be NULL)
            sp, ns = keep.ctypes.data_as(C.POINTER(C.c_int64)), a.size
        st, res = AggStats(), C.c_void_p()
        self._chk(self.lib.gg_khop_aggregate(self.ctx, csr.handle, sp, ns, k_min, k_max, GROUP_BY[group_by], wp,
                                             C.byref(st), C.byref(res) if fetch else None))
        d = {"groups": list(st.groups), "walks": list(st.walks), "entries_pulled": int(st.entries_pulled)}
        return KhopAggregate(self, res if fetch else None, d)

    def khop_aggregate_top(self, agg: "KhopAggregate", hops: int, order_by: str = "total", descending: bool = True,
                           n: int = 100, csr=None, bias=None) -> "KhopAggregate":
        """gg_khop_aggregate_top: the best n groups of level `hops` of `agg` in rank order — ORDER BY key [DESC], id
        LIMIT n with key = "total" (+ bias[vertex]: V integers in vertex-table order, which needs `csr`) or "walks".
        The answer is a KhopAggregate of that one level; stats: {"rows_in", "rows_out", "select_passes", "sort_route"}."""
        if order_by not in TOP_BY:
            raise ValueError(f"order_by {order_by!r}: one of {sorted(TOP_BY)}")
        bp = None
        if bias is not None:
            if csr is None:
                raise ValueError("a bias needs the csr of its vertices")
            b, bp = _i64(bias)
            if b.ndim != 1 or b.size != csr.V:
                raise ValueError(f"bias: {b.size} entries for {csr.V} vertices")
        st, res = TopStats(), C.c_void_p()
        self._chk(self.lib.gg_khop_aggregate_top(self.ctx, agg.handle, hops, TOP_BY[order_by], 1 if descending else 0,
                                                 int(n), csr.handle if csr is not None else None, bp, C.byref(st),
                                                 C.byref(res)))
        d = {"rows_in": int(st.rows_in), "rows_out": int(st.rows_out), "select_passes": int(st.select_passes),
             "sort_route": int(st.sort_route)}
        return KhopAggregate(self, res, d)

    def debug_aggregate_top(self, sort_route: int = 0, candidate_floor: int = 0):
        """gg_khop_aggregate_top orders its survivors in LDS (1) or by the global passes (2) and compacts the selection's
        candidates at candidate_floor or fewer (0: the defaults)."""
        self._chk(self.lib.gg_debug_aggregate_top(self.ctx, int(sort_route), int(candidate_floor)))

    def debug_aggregate_top_listed(self) -> int:
        """entries of the candidate list the last khop_aggregate_top's selection wrote (0: it did not compact)"""
        n = C.c_uint64()
        self._chk(self.lib.gg_debug_aggregate_top_listed(self.ctx, C.byref(n)))
        return int(n.value)

    def debug_aggregate_long_row(self, n: int = 0):
        """gg_khop_aggregate gives rows of more than n entries to a whole workgroup each (0: the default)."""
        self._chk(self.lib.gg_debug_aggregate_long_row(self.ctx, int(n)))

    # ---- walks counted per (source, end vertex) pair
    def khop_pair_counts(self, csr: Csr, k_min: int, k_max: int, sources=None, targets=None,
                         fetch: bool = True) -> "KhopPairCounts":
        """gg_khop_pair_counts: per level h in k_min..k_max one row (index into `sources`, end vertex id, walks) per pair
        with walks != 0.  sources None: every vertex in vertex-table order; a list longer than 64 runs in batches of 64, one
        C call each, the rows concatenated with the batch's offset added to the source index and the stats added (walks
        mod 2^64).  targets: only these ids may end a row (None: every vertex; an empty list: no rows).  fetch=False: the
        stats only, nothing is kept on the device."""
        if sources is None:
            a = np.ascontiguousarray(csr.export()[3], dtype=np.int64)
        else:
            a = np.ascontiguousarray(sources, dtype=np.int64).reshape(-1)
        tp, nt = None, 0
        if targets is not None:
            t = np.ascontiguousarray(targets, dtype=np.int64).reshape(-1)
            keep = t if t.size else np.zeros(1, np.int64)  # (an empty list is a list: the pointer must not be NULL)
            tp, nt = keep.ctypes.data_as(C.POINTER(C.c_int64)), t.size
        d = {"pairs": [0] * (GG_MAX_HOPS + 1), "walks": [0] * (GG_MAX_HOPS + 1), "entries_pulled": 0, "rows_gathered": 0}
        out = KhopPairCounts(self, [], d)
        try:
            for base in range(0, a.size, GG_BFS_LANES):  # (an empty list: no batch, no rows)
                part = np.ascontiguousarray(a[base:base + GG_BFS_LANES])
                st, res = PairStats(), C.c_void_p()
                self._chk(self.lib.gg_khop_pair_counts(
                    self.ctx, csr.handle, part.ctypes.data_as(C.POINTER(C.c_int64)), part.size,
                    k_min, k_max, tp, nt, C.byref(st), C.byref(res) if fetch else None))
                if fetch:
                    out.parts.append((res, base))
                for h in range(GG_MAX_HOPS + 1):
                    d["pairs"][h] += int(st.pairs[h])
                    d["walks"][h] = (d["walks"][h] + int(st.walks[h])) % (1 << 64)
                d["entries_pulled"] += int(st.entries_pulled)
                d["rows_gathered"] += int(st.rows_gathered)
        except Exception:
            out.close()
            raise
        return out

    def debug_pair_counts(self, long_row_entries: int = 0, gather_mode: int = 0):
        """gg_khop_pair_counts gives in-rows of more than long_row_entries entries to a whole workgroup each (0: the
        default) and with gather_mode 1 reads every entry's state row whatever its mask."""
        self._chk(self.lib.gg_debug_pair_counts(self.ctx, int(long_row_entries), int(gather_mode)))

    # ---- cheapest paths over weighted edge rows
    def edge_weights(self, csr: Csr, weights, by: str = "rowid") -> "EdgeWeights":
        """gg_edge_weights_create: one int64 weight >= 0 per edge row, by="rowid": indexed by the edge row's rowid (without
        explicit rowids: in the order of append_edges), by="entry": one per kept entry in the order of csr.export()."""
        w = np.ascontiguousarray(weights, dtype=np.int64).reshape(-1)
        keep = w if w.size else np.zeros(1, np.int64)
        h = C.c_void_p()
        self._chk(self.lib.gg_edge_weights_create(self.ctx, csr.handle, keep.ctypes.data_as(C.POINTER(C.c_int64)), w.size,
                                                  WEIGHTS_BY[by], C.byref(h)))
        return EdgeWeights(self, h)

    def _cheapest(self, csr: Csr, weights: "EdgeWeights", a, max_hops: int, targets, fetch: bool) -> "CheapestPaths":
        tp, nt = None, 0
        if targets is not None:
            t = np.ascontiguousarray(targets, dtype=np.int64).reshape(-1)
            keep = t if t.size else np.zeros(1, np.int64)  # (an empty list is a list: the pointer must not be NULL)
            tp, nt = keep.ctypes.data_as(C.POINTER(C.c_int64)), t.size
        d = {"rounds": 0, "reached_pairs": 0, "cells_lowered": 0, "entries_pulled": 0, "rows_gathered": 0}
        out = CheapestPaths(self, [], d)
        try:
            for base in range(0, a.size, GG_BFS_LANES):  # (an empty list: no batch, no rows)
                part = np.ascontiguousarray(a[base:base + GG_BFS_LANES])
                st, res = CheapestStats(), C.c_void_p()
                self._chk(self.lib.gg_cheapest64(
                    self.ctx, csr.handle, weights.handle, part.ctypes.data_as(C.POINTER(C.c_int64)), part.size,
                    int(max_hops), tp, nt, C.byref(st), C.byref(res) if fetch else None))
                if fetch:
                    out.parts.append((res, base))
                for k in d:
                    d[k] += int(getattr(st, k))
        except Exception:
            out.close()
            raise
        return out

    def cheapest64(self, csr: Csr, weights: "EdgeWeights", sources, max_hops: int = -1, targets=None,
                   fetch: bool = True) -> "CheapestPaths":
        """gg_cheapest64, one call: 1..64 sources, one row (index into `sources`, vertex id, cost, hops) per reached pair.
        max_hops < 0: to the fixpoint.  targets: only these ids may have a row (None: every vertex; an empty list: no
        rows).  fetch=False: the stats only, nothing is kept on the device."""
        a = np.ascontiguousarray(sources, dtype=np.int64).reshape(-1)
        if not 1 <= a.size <= GG_BFS_LANES:
            raise GGError(-1, f"cheapest64: {a.size} sources outside 1..{GG_BFS_LANES}")
        return self._cheapest(csr, weights, a, max_hops, targets, fetch)

    def cheapest_path_lengths(self, csr: Csr, weights: "EdgeWeights", sources=None, max_hops: int = -1, targets=None,
                              fetch: bool = True) -> "CheapestPaths":
        """gg_cheapest64 over any number of sources (None: every vertex in vertex-table order): batches of 64, one C call
        each, the rows concatenated with the batch's offset added to the source index and the stats added."""
        if sources is None:
            a = np.ascontiguousarray(csr.export()[3], dtype=np.int64)
        else:
            a = np.ascontiguousarray(sources, dtype=np.int64).reshape(-1)
        return self._cheapest(csr, weights, a, max_hops, targets, fetch)

    def cheapest64_paths(self, csr: Csr, weights: "EdgeWeights", sources, pair_lane, pair_dst, edges: bool = True):
        """gg_cheapest64_paths: the pinned cheapest path of each (sources[pair_lane[i]], pair_dst[i]) of one <=64-source batch
        run to the fixpoint.  Returns ((pair int64, step int32, vertex int64, edge int64, cost int64) ascending by (pair,
        step), the pair table (pair int64, cost int64, hops int32, traced int32) of the reached pairs, stats): stats = the
        call's gg_cheapest_paths_stats as a dict, the rounds' under "search"."""
        i64p, i32p = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
        s, ps = _i64(sources)
        d, pd = _i64(pair_dst)
        lane = np.ascontiguousarray(pair_lane, dtype=np.uint32)
        if lane.size != d.size:
            raise ValueError("one source lane per target")
        st, res = CheapestPathsStats(), C.c_void_p()
        self._chk(self.lib.gg_cheapest64_paths(self.ctx, csr.handle, weights.handle, ps, s.size,
                                               lane.ctypes.data_as(C.POINTER(C.c_uint32)), pd, d.size, 1 if edges else 0,
                                               C.byref(st), C.byref(res)))
        try:
            def fetch_table(table, cols, call):
                n = C.c_uint64()
                self._chk(self.lib.gg_cheapest64_paths_rows(res, table, C.byref(n)))
                n = int(n.value)
                out = [np.empty(n, t) for t in cols]
                done = 0
                while done < n:
                    got = C.c_uint32()
                    ptrs = [a[done:].ctypes.data_as({np.int64: i64p, np.int32: i32p}[t]) for a, t in zip(out, cols)]
                    self._chk(call(res, done, min(n - done, 1 << 30), *ptrs, C.byref(got)))
                    assert got.value
                    done += got.value
                return tuple(out)
            pairs = fetch_table(0, (np.int64, np.int64, np.int32, np.int32), self.lib.gg_cheapest64_paths_fetch_pairs)
            rows = fetch_table(1, (np.int64, np.int32, np.int64, np.int64, np.int64), self.lib.gg_cheapest64_paths_fetch)
        finally:
            self.lib.gg_result_destroy(res)
        stats = {k: int(getattr(st, k)) for k in ("pairs_reached", "pairs_saturated", "rows", "entries_scanned")}
        stats["search"] = {name: int(getattr(st.search, name)) for name, _ in CheapestStats._fields_}
        return rows, pairs, stats

    def cheapest_paths(self, csr: Csr, weights: "EdgeWeights", src, dst, edges: bool = True):
        """The pinned cheapest path (include/gg.h, gg_cheapest64_paths) of every pair (src[i], dst[i]), unnested: arrays
        (pair_index int64, step int32, vertex int64, edge int64, cost int64), one row per step 0..hops of every pair that has
        an unsaturated cost, ascending by (pair index, step); edge is the rowid of the edge into the step's vertex, -1 at step
        0 (and everywhere with edges=False).  Any number of pairs, grouped by source into device batches of at most 64
        distinct sources as shortest_paths groups them."""
        parts = []
        for sources, lanes, targets, members in self._all_paths_batches(src, dst):
            rows, _, _ = self.cheapest64_paths(csr, weights, sources, lanes, targets, edges)
            parts.append((members[rows[0]],) + rows[1:])
        if not parts:
            return tuple(np.empty(0, np.int32 if k == 1 else np.int64) for k in range(5))
        cols = [np.concatenate([p[c] for p in parts]) for c in range(5)]
        order = np.argsort(cols[0], kind="stable")  # batches interleave; inside a pair the steps already ascend
        return tuple(c[order] for c in cols)

    def debug_cheapest(self, long_row_entries: int = 0, gather_mode: int = 0):
        """gg_cheapest64 gives in-rows of more than long_row_entries entries to a whole workgroup each (0: the default)
        and with gather_mode 1 counts every entry as live whatever its mask."""
        self._chk(self.lib.gg_debug_cheapest(self.ctx, int(long_row_entries), int(gather_mode)))

    # ---- weakly connected components
    def components(self, csr: Csr, fetch: bool = True) -> dict:
        """gg_components: {"stats": {...}} and, with fetch, table 0 as "vertex", "component" (int64) and "size" (uint64), one
        row per vertex in vertex-table order, and table 1 as "components" (int64) and "sizes" (uint64), one row per component
        ascending by its representative's position.  A component's id is the id of its first vertex in the vertex table."""
        st, res = CcStats(), C.c_void_p()
        self._chk(self.lib.gg_components(self.ctx, csr.handle, C.byref(st), C.byref(res) if fetch else None))
        out = {"stats": {name: int(getattr(st, name)) for name, _ in CcStats._fields_}}
        if not fetch:
            return out
        i64p, u64p = C.POINTER(C.c_int64), C.POINTER(C.c_uint64)
        try:
            tables = []
            for table in (0, 1):
                cnt = C.c_uint64()
                self._chk(self.lib.gg_components_rows(res, table, C.byref(cnt)))
                n = int(cnt.value)
                cols = [np.empty(n, np.int64) for _ in range(2 - table)] + [np.empty(n, np.uint64)]
                got, o = C.c_uint32(), 0
                while o < n:
                    ptrs = [c[o:].ctypes.data_as(i64p) for c in cols[:-1]] + [cols[-1][o:].ctypes.data_as(u64p)]
                    fn = self.lib.gg_components_fetch_sizes if table else self.lib.gg_components_fetch
                    self._chk(fn(res, o, min(n - o, 1 << 20), *ptrs, C.byref(got)))
                    if not got.value:
                        raise GGError(-6, f"gg_components_fetch: no row at offset {o} of {n}")
                    o += got.value
                tables.append(cols)
        finally:
            self.lib.gg_result_destroy(res)
        out["vertex"], out["component"], out["size"] = tables[0]
        out["components"], out["sizes"] = tables[1]
        return out

    def debug_components(self, init_mode: int = 0, jumps_per_check: int = 0):
        """gg_components looks at the flatten's changed word once per jumps_per_check launches (0: the default); init_mode 1
        starts every vertex as its own root, which is also the default start (0)."""
        self._chk(self.lib.gg_debug_components(self.ctx, int(init_mode), int(jumps_per_check)))

    def debug_triangle_tile(self, n: int = 0):
        """gg_triangles stages at most n entries of an in-row in LDS (0: the default); longer rows are searched in
        global memory."""
        self._chk(self.lib.gg_debug_triangle_tile(self.ctx, int(n)))

    # ---- graph-sharded BFS (one shard per GPU; see include/gg.h)
    def bfs_sharded_begin(self, shard: Csr, sources) -> "ShardedBfs":
        s, ps = _i64(sources)
        h = C.c_void_p()
        self._chk(self.lib.gg_bfs_sharded_begin(self.ctx, shard.handle, ps, s.size, C.byref(h)))
        return ShardedBfs(self, h, shard.V)

    def bfs_sharded_emulated(self, shards, sources, max_hops: int):
        """All ranks of a graph-sharded BFS in ONE process (the shards live on this context): the exchange is
        a host-side sum of the ranks' words.  Returns the union of the ranks' (source, vertex, distance) rows
        and the number of levels expanded — what N GPUs with an RCCL all-reduce between them produce."""
        runs = [self.bfs_sharded_begin(c, sources) for c in shards]
        try:
            level = 0
            while max_hops < 0 or level < max_hops:
                words = np.zeros(runs[0].V, np.uint64)
                new = 0
                for r in runs:
                    new += r.expand()
                    words += r.words()  # disjoint supports: the sum is the OR
                if new == 0:
                    break
                for r in runs:
                    r.set_words(words)
                    r.commit()
                level += 1
            rows = [r.pairs() for r in runs]
            self.last_sharded_levels = [r.levels() for r in runs]  # (pushed, pulled) per rank
            return np.concatenate(rows, axis=0), level
        finally:
            for r in runs:
                r.close()

    # ---- profiling
    def profile(self, on: bool):
        self._chk(self.lib.gg_profile_enable(self.ctx, int(on)))

    def profile_select(self, names=None):
        """Time only these kernels (list of names; None: all)."""
        self._chk(self.lib.gg_profile_select(self.ctx, None if names is None else ",".join(names).encode()))

    def profile_reset(self):
        self._chk(self.lib.gg_profile_reset(self.ctx))

    def profile_get(self):
        n = C.c_int()
        self._chk(self.lib.gg_profile_count(self.ctx, C.byref(n)))
        out = {}
        for i in range(n.value):
            name, cnt, ms = C.c_char_p(), C.c_uint64(), C.c_double()
            self._chk(self.lib.gg_profile_get(self.ctx, i, C.byref(name), C.byref(cnt), C.byref(ms)))
            out[name.value.decode()] = (cnt.value, ms.value)
        return out
