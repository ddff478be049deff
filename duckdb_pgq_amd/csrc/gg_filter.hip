// gg_filter.hip — filters over materialised path rows: the same-neighbour filter, and the edge condition between two columns.
//
// Train Benchmark ConnectedSegments (benchmark/trainbenchmark/queries/connectedsegments.sql:1-25) is a
// 5-edge path over connectsTo whose six segments must all be monitored by the SAME sensor: in the
// reference, six more hash joins with monitoredBy plus five equality predicates on the sensor column
// (PhysicalHashJoin probes, src/execution/operator/join/physical_hash_join.cpp:217-254).  Here the
// path rows are already in HBM (gg_expand_khop, materialised); one pass keeps, for every row, each
// neighbour w of the row's FIRST vertex in the filter graph that is also a neighbour of all the other
// vertices of the row (join multiplicities multiply, as the chained joins would produce).
//   k_filter_count  per row: walk adj_f(v0) (a few entries), membership tests by linear scan
//   scan            exclusive prefix of the per-row output counts
//   k_filter_fill   same walk, writing (w, v0..vh) as int64 ids
//
// Edge condition between two columns of a walk table (gg_result_filter_edge, second half of this file).  The reference
// asks "is there an edge row v_i -> v_j" of walk rows in three ways: the last hash join of a chain carrying two conditions
// (`k4.dst = k1.src`: PhysicalHashJoin::Execute -> JoinHashTable::Probe + ScanStructure::NextInnerJoin,
// src/execution/join_hashtable.cpp:304-476), NOT EXISTS over knows (benchmark/ldbc/queries/interactive-complex-10.sql:
// 19-24: ScanStructure::ScanKeyMatches + NextAntiJoin, join_hashtable.cpp:478-540) and EXISTS (interactive-complex-7.sql:5,
// interactive-short-7.sql:3: NextSemiJoin, join_hashtable.cpp:522).  Here the rows are in HBM already and the answer is a
// run length: csr->rnbr_by_src (gg_paths.hip) holds the in-row of every vertex with its sources ascending, so the number m
// of edge rows v_from -> v_to is upper bound - lower bound of dense(v_from) in the in-row of dense(v_to).
//   k_edge_filter_count  one thread per row: the two condition cells, two dictionary probes, the two bounds; m per row
//                        (u32) and per workgroup of 256 rows the rows it puts out (u64) — inner m, semi m > 0, anti m == 0
//   scan                 exclusive prefix of the workgroups' rows
//   k_edge_filter_write  reads m (no search is repeated), places the row by workgroup base + prefix inside the workgroup
//                        (ballot + popcount in semi and anti mode, a wavefront scan in inner mode) and copies its
//                        hops + 1 cells: the kept lanes of a wavefront write consecutive cells of every column, in the
//                        input's order, at the same places on every run.
// Bytes per input row (model): 16 B of condition cells, two 16-byte dictionary slots, 2 x ceil(log2 |in(v_to)|) probes of
// 4 B (the first ones of a hub's row shared through L2), 4 B of m written and read once each, 8 (hops + 1) B read per
// kept row and 8 (hops + 1) B written per output row.
#include "gg_internal.h"
#include "gg_walk_table.h"

using namespace gg;

namespace gg {

struct RowCols {
  const int64_t *c[GG_MAX_HOPS + 1];
};
struct OutCols {
  int64_t *c[GG_MAX_HOPS + 2];
};

// number of filter edges v -> w
__device__ __forceinline__ uint32_t mult_of(const uint32_t *__restrict__ off, const uint32_t *__restrict__ nbr,
                                            uint32_t v, uint32_t w) {
  uint32_t m = 0;
  for (uint32_t i = off[v]; i < off[v + 1]; i++) m += (nbr[i] == w);
  return m;
}

template <bool FILL>
__global__ __launch_bounds__(256) void k_filter(RowCols in, int ncols, uint64_t n_rows, DictView dict,
                                                const uint32_t *__restrict__ off, const uint32_t *__restrict__ nbr,
                                                const int64_t *__restrict__ vid, uint64_t *__restrict__ counts,
                                                const uint64_t *__restrict__ offsets, OutCols out) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rows) return;
  uint32_t d[GG_MAX_HOPS + 1];
  bool ok = true;
  for (int c = 0; c < ncols; c++) {
    d[c] = dict.lookup(in.c[c][r]);  // row vertex -> dense index in the FILTER graph
    ok = ok && d[c] != INVALID_U32;
  }
  uint64_t n = 0, o = FILL ? offsets[r] : 0;
  if (ok) {
    for (uint32_t i = off[d[0]]; i < off[d[0] + 1]; i++) {
      const uint32_t w = nbr[i];
      uint64_t m = 1;
      for (int c = 1; c < ncols && m; c++) m *= mult_of(off, nbr, d[c], w);
      if (FILL) {
        for (uint64_t k = 0; k < m; k++, o++) {
          out.c[0][o] = vid[w];
          for (int c = 0; c < ncols; c++) out.c[c + 1][o] = in.c[c][r];
        }
      }
      n += m;
    }
  }
  if (!FILL) counts[r] = n;
}

}  // namespace gg

extern "C" int gg_result_filter_common_neighbour(gg_ctx *ctx, const gg_result *res, int hops, const gg_csr *filter,
                                                 gg_result **out) {
  const char *fn = "gg_result_filter_common_neighbour";
  // (this entry point has one code for every fault, a shard included)
  GG_TRY(walk_table_arg(fn, ctx, res, hops, KindRule::INVALID_ARG, GG_MAX_HOPS - 1));
  GG_TRY(csr_arg(fn, ctx, filter));
  if (!out || filter->n_parts > 1) {
    set_error("%s: NULL out, or a CSR shard (gg_csr_build_shard) as the filter graph", fn);
    return GG_ERR_INVALID_ARG;
  }
  *out = nullptr;
  ApiScope scope(ctx);
  GG_HIP(hipSetDevice(ctx->device));
  const uint64_t n_rows = res->rows[hops];
  const int ncols = hops + 1;
  ResultOwner o = make_result(ctx, ResultKind::TABLES, hops + 1, hops + 1);  // the table with hops+2 columns: (w, v0..vh)
  RowCols in;
  for (int c = 0; c < ncols; c++) in.c[c] = res->cols[hops][c];
  OutCols oc;
  for (int c = 0; c < GG_MAX_HOPS + 2; c++) oc.c[c] = nullptr;
  uint64_t total = 0;
  DictView dict{};
  if (n_rows) GG_TRY(dict_view(ctx, filter, &dict));
  if (dict.ht) {  // (rows to filter, and a filter graph with vertices: without one no row is kept)
    uint64_t *counts = nullptr;
    GG_TRY(ctx->dev_alloc((void **)&counts, (n_rows + 1) * sizeof(uint64_t)));
    const unsigned grid = (unsigned)((n_rows + 255) / 256);
    GG_LAUNCH(ctx, "filter_count", (k_filter<false>), dim3(grid), dim3(256), 0, in, ncols, n_rows, dict, filter->off,
              filter->nbr, filter->vid, counts, (const uint64_t *)nullptr, oc);
    GG_TRY(scan_total_u64(ctx, counts, counts, n_rows, &total));
    GG_TRY(alloc_kept_columns(ctx, o->cols[hops + 1], ncols + 1, total ? total : 1));
    for (int c = 0; c <= ncols; c++) oc.c[c] = o->cols[hops + 1][c];
    if (total)
      GG_LAUNCH(ctx, "filter_fill", (k_filter<true>), dim3(grid), dim3(256), 0, in, ncols, n_rows, dict, filter->off,
                filter->nbr, filter->vid, (uint64_t *)nullptr, (const uint64_t *)counts, oc);
    GG_TRY(sync_checked(ctx));
  } else {
    GG_TRY(alloc_kept_columns(ctx, o->cols[hops + 1], ncols + 1, 1));
  }
  o->rows[hops + 1] = total;
  *out = o.release();
  return GG_OK;
}

// ---- edge condition between two columns of a walk table --------------------------------------------------------------
namespace gg {

struct EdgeOut {
  int64_t *c[GG_MAX_HOPS + 1];
};

// how often u occurs in the ascending row[0..n): upper bound - lower bound (the search of tri_run in gg_triangles.hip, which
// stays private to its kernel; only the length is wanted here)
__device__ __forceinline__ uint32_t edge_run(const uint32_t *__restrict__ row, uint32_t n, uint32_t u) {
  uint32_t lo = 0, hi = n;  // first idx with row[idx] >= u
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (row[mid] < u) lo = mid + 1; else hi = mid;
  }
  if (lo == n || row[lo] != u) return 0;
  uint32_t l2 = lo + 1, h2 = n;  // first idx with row[idx] > u
  while (l2 < h2) {
    const uint32_t mid = (l2 + h2) >> 1;
    if (row[mid] <= u) l2 = mid + 1; else h2 = mid;
  }
  return l2 - lo;
}

// rows a row with m matching edge rows puts out
__device__ __forceinline__ uint32_t edge_keep(int mode, uint32_t m) {
  return mode == GG_EDGE_INNER ? m : (uint32_t)((m != 0) == (mode == GG_EDGE_SEMI));
}

// Workgroup g0 + blockIdx.x owns rows [256 g, 256 g + 256).  Count (FILL false): `from` / `to` are the condition columns,
// dict.ht == null says the condition graph has no edge (m = 0 everywhere); m_rows (nullable) gets m, group[g] the workgroup's
// output rows, *matches += its sum of m.  Write (FILL true): m_rows is read, group[g] is the workgroup's first output row.
template <bool FILL>
__global__ __launch_bounds__(256) void k_edge_filter(RowCols in, int ncols, const int64_t *__restrict__ from,
                                                     const int64_t *__restrict__ to, int mode, uint64_t g0,
                                                     uint64_t n_rows, DictView dict, const uint32_t *__restrict__ roff,
                                                     const uint32_t *__restrict__ rin, uint32_t *__restrict__ m_rows,
                                                     uint64_t *__restrict__ group, unsigned long long *__restrict__ matches,
                                                     EdgeOut out) {
  __shared__ uint64_t s_keep[4], s_m[4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint64_t g = g0 + blockIdx.x, r = g * 256 + threadIdx.x;
  const bool live = r < n_rows;
  if (!FILL) {
    uint32_t m = 0;
    if (live && dict.ht) {
      const uint32_t u = dict.lookup(from[r]), t = dict.lookup(to[r]);
      if (u != INVALID_U32 && t != INVALID_U32) {  // (t < V: roff has V + 1 entries, the row lies inside rin)
        const uint32_t lo = roff[t];
        m = edge_run(rin + lo, roff[t + 1] - lo, u);
      }
    }
    if (live && m_rows) m_rows[r] = m;
    const uint64_t k = wave_reduce_add_u64(live ? edge_keep(mode, m) : 0u), mm = wave_reduce_add_u64(m);
    if (lane == 0) s_keep[wave] = k, s_m[wave] = mm;
    __syncthreads();
    if (threadIdx.x == 0) {
      group[g] = s_keep[0] + s_keep[1] + s_keep[2] + s_keep[3];
      const uint64_t all = s_m[0] + s_m[1] + s_m[2] + s_m[3];
      if (all) atomicAdd(matches, (unsigned long long)all);
    }
  } else {
    const uint32_t keep = live ? edge_keep(mode, m_rows[r]) : 0u;
    uint32_t before, wave_rows;  // (fewer than 2^32 rows in all, or they are not written: 32-bit prefixes are exact)
    if (mode == GG_EDGE_INNER) {  // (uniform: a kernel argument)
      const uint32_t incl = wave_scan_incl(keep);
      before = incl - keep;
      wave_rows = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    } else {
      const uint64_t kept = __ballot(keep != 0);
      before = (uint32_t)__popcll(kept & ((1ull << lane) - 1));
      wave_rows = (uint32_t)__popcll(kept);
    }
    if (lane == 0) s_keep[wave] = wave_rows;
    __syncthreads();
    uint64_t pos = group[g] + before;
    for (int w = 0; w < wave; w++) pos += s_keep[w];
    if (keep) {  // (pos + keep <= the scan's total: the count pass counted the same rows)
#pragma unroll
      for (int c = 0; c <= GG_MAX_HOPS; c++) {
        if (c < ncols) {
          const int64_t v = in.c[c][r];
          int64_t *__restrict__ o = out.c[c] + pos;
          for (uint32_t k = 0; k < keep; k++) o[k] = v;
        }
      }
    }
  }
}

struct EdgeArgs {
  RowCols in;
  int ncols;
  const int64_t *from, *to;
  int mode;
  uint64_t n_rows;
  DictView dict;  // ht null: the condition graph has no edge
  const uint32_t *roff, *rin;
  uint32_t *m_rows;
  uint64_t *group;
  unsigned long long *matches;
  EdgeOut out;
};

// split under gg_debug_max_grid_tiles like the expansion and triangle kernels
template <bool FILL>
int edge_filter_launch(gg_ctx *ctx, const EdgeArgs &a) {
  return split_groups(ctx, (a.n_rows + 255) / 256, [&](uint64_t g0, uint64_t ng) -> int {
    GG_LAUNCH(ctx, FILL ? "k_edge_filter_write" : "k_edge_filter_count", (k_edge_filter<FILL>), dim3((unsigned)ng),
              dim3(256), 0, a.in, a.ncols, a.from, a.to, a.mode, g0, a.n_rows, a.dict, a.roff, a.rin, a.m_rows, a.group,
              a.matches, a.out);
    return GG_OK;
  });
}

}  // namespace gg

extern "C" int gg_result_filter_edge(gg_ctx *ctx, const gg_result *res, int hops, const gg_csr *csr_c, int from_col,
                                     int to_col, int mode, int materialise, gg_edge_filter_stats *stats,
                                     gg_result **out_result) {
  if (out_result) *out_result = nullptr;
  if (stats) memset(stats, 0, sizeof(*stats));
  const char *fn = "gg_result_filter_edge";
  GG_TRY(result_arg(fn, ctx, res));
  GG_TRY(csr_arg(fn, ctx, csr_c));
  if (materialise && !out_result) {
    set_error("%s: materialise without out_result", fn);
    return GG_ERR_INVALID_ARG;
  }
  GG_TRY(whole_csr(fn, csr_c, "the condition graph"));
  GG_TRY(walk_kind_arg(fn, res, KindRule::STATE));
  GG_TRY(hops_arg(fn, res, hops));
  GG_TRY(column_arg(fn, "from", from_col, 0, hops));
  GG_TRY(column_arg(fn, "to", to_col, 0, hops));
  if (mode != GG_EDGE_INNER && mode != GG_EDGE_SEMI && mode != GG_EDGE_ANTI) {
    set_error("%s: mode %d (0: inner, 1: semi, 2: anti)", fn, mode);
    return GG_ERR_INVALID_ARG;
  }
  ApiScope scope(ctx);
  GG_HIP(hipSetDevice(ctx->device));
  gg_csr *csr = const_cast<gg_csr *>(csr_c);
  const uint64_t n_rows = res->rows[hops];
  ResultOwner o;
  // table hops: the id columns v0..v_hops, no edge columns
  if (materialise) o = make_result(ctx, ResultKind::TABLES, hops, hops);
  uint64_t total = 0, matches = 0;
  if (n_rows) {
    EdgeArgs a{};
    a.ncols = hops + 1;
    for (int c = 0; c < a.ncols; c++) a.in.c[c] = res->cols[hops][c];
    a.from = res->cols[hops][from_col], a.to = res->cols[hops][to_col];
    a.mode = mode;
    a.n_rows = n_rows;
    if (csr->V && csr->E) {  // (without an edge every m is 0: nothing to look up)
      GG_TRY(dict_view(ctx, csr, &a.dict));
      GG_TRY(ensure_reverse_by_source(ctx, csr));
      a.roff = csr->roff, a.rin = csr->rnbr_by_src;
    }
    const uint64_t groups = (n_rows + 255) / 256;
    if (materialise) GG_TRY(ctx->dev_alloc((void **)&a.m_rows, n_rows * sizeof(uint32_t)));
    GG_TRY(ctx->dev_alloc((void **)&a.group, groups * sizeof(uint64_t)));
    GG_TRY(ctx->dev_alloc((void **)&a.matches, sizeof(unsigned long long)));
    GG_HIP(hipMemsetAsync(a.matches, 0, sizeof(unsigned long long), ctx->stream));
    GG_TRY(edge_filter_launch<false>(ctx, a));
    GG_TRY(scan_total_u64(ctx, a.group, a.group, groups, &total, false, {{a.matches, sizeof(uint64_t), &matches}}));
    if (materialise && total) {
      if (total >= (1ull << 32)) {
        set_error("gg_result_filter_edge: %llu rows to materialise (2^32 or more); count them, or filter a smaller table",
                  (unsigned long long)total);
        return GG_ERR_TOO_LARGE;
      }
      GG_TRY(alloc_kept_columns(ctx, o->cols[hops], a.ncols, total));
      for (int c = 0; c < a.ncols; c++) a.out.c[c] = o->cols[hops][c];
      GG_TRY(edge_filter_launch<true>(ctx, a));
      GG_TRY(sync_checked(ctx));
    }
  }
  if (stats) stats->rows_in = n_rows, stats->rows_out = total, stats->matches = matches;
  if (materialise) {
    o->rows[hops] = total;
    *out_result = o.release();
  }
  return GG_OK;
}
