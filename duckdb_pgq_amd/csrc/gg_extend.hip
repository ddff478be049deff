// gg_extend.hip — one more hop over a second edge table: the rows of a walk table joined with the edge rows of another CSR.
//
// The reference's LDBC statements rarely stay inside one table: they walk `knows` and then join a different keyed table on a
// column of the walk (benchmark/ldbc/queries/interactive-complex-2.sql:2-7: knows -> message on k_person2id = m_creatorid;
// interactive-complex-4.sql:2-8: knows -> message -> message_tag; interactive-complex-9.sql:13-15 and
// interactive-complex-6.sql:14-17: friends and friends of friends, their messages, their tags; interactive-complex-5.sql:15:
// forum_person joined on a middle column).  There that is the next PhysicalHashJoin of the chain over a different build table
// (JoinHashTable::Probe + ScanStructure::NextInnerJoin, src/execution/join_hashtable.cpp:304-476) whose payload
// (m_creationdate, m_content) ScanStructure::GatherResult fetches by row.  Here the walk rows are in HBM already
// (gg_expand_khop_result, gg_result_filter_edge, this function) and the second table is a CSR of the same context: the join
// is one dictionary probe per input row and one forward row of that CSR, and the payload's handle is the edge row's rowid.
//   k_extend_count   one thread per input row: the cell of from_col, one dictionary probe, deg = off[u + 1] - off[u]; u (u32)
//                    and the row's prefix inside its workgroup of 256 rows (u32) are kept for the write pass, the
//                    workgroup's total (u64) goes to the scan, the rows with deg > 0 are counted
//   scan             exclusive prefix of the workgroups' totals; P(r) = group[r / 256] + pre[r] is row r's first output row
//   k_extend_tiles   one thread per tile boundary: the input row that owns output row t * tile_rows (a search in P)
//   k_extend_write   one workgroup per tile of tile_rows consecutive OUTPUT rows (1024; gg_debug_extend shrinks it).  The
//                    tile stages P of its span of input rows in LDS (EX_WIN entries; a span made longer than that by
//                    zero-degree rows is finished by a search in global memory), every output row finds its parent by a
//                    search there, copies the parent's cells and gathers vid[nbr[off[u] + k]] — and eid / epos of that
//                    entry with edge columns.  Consecutive lanes write consecutive cells of every column; a parent of
//                    thousands of edge rows is spread over as many lanes and tiles as it has rows, a run of rows without
//                    any costs its tile a longer search and nothing else.
// Placement is count, scan, write: no atomic orders a row, so the rows stand at the same places on every run and for
// every tile size.
// Bytes per input row (model): 8 B of condition cell, one 16-byte dictionary slot, two offsets of 4 B, 8 B of u and prefix
// written and 8 B read again per tile that touches the row.  Per output row: 8 (hops + 1) B of parent cells read (shared
// through L2 / L1 among the copies of one parent), 4 B of nbr, 8 B of vid (a gather), 8 (hops + 2) B written; with edge
// columns 4 or 8 B of rowid read, 8 hops B of the parent's edge cells read and 8 (hops + 1) B written.
#include "gg_internal.h"
#include "gg_walk_table.h"

using namespace gg;

namespace gg {

constexpr uint32_t EX_TILE_ROWS = 1024;  // output rows per workgroup of the write pass
constexpr int EX_PER = EX_TILE_ROWS / 256;  // output rows per lane of a full tile
constexpr uint32_t EX_WIN = 1024;        // input rows whose prefixes a tile stages in LDS

struct ExIn {
  const int64_t *c[GG_MAX_HOPS + 1];  // id columns v0..v_hops of the input (hops + 1 <= GG_MAX_HOPS: c[GG_MAX_HOPS] stays null)
  const int64_t *e[GG_MAX_HOPS];      // its edge columns e1..e_hops, all null if it has none
};
struct ExOut {
  int64_t *c[GG_MAX_HOPS + 1];  // v0..v_hops, w
  int64_t *e[GG_MAX_HOPS];      // e1..e_{hops+1}, all null without edge columns
};

// Workgroup g0 + blockIdx.x owns input rows [256 g, 256 g + 256).  u_rows / pre (both nullable: count mode keeps nothing
// per row) get the dense index of the row's cell and the sum of the degrees of the workgroup's earlier rows; group[g] the
// workgroup's total, *matched += its rows with an edge row.
__global__ __launch_bounds__(256) void k_extend_count(const int64_t *__restrict__ from, uint64_t g0, uint64_t n_rows,
                                                      DictView dict, const uint32_t *__restrict__ off, uint32_t *__restrict__ u_rows,
                                                      uint32_t *__restrict__ pre, uint64_t *__restrict__ group,
                                                      unsigned long long *__restrict__ matched) {
  __shared__ uint64_t s_sum[4];
  __shared__ uint32_t s_hit[4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint64_t g = g0 + blockIdx.x, r = g * 256 + threadIdx.x;
  const bool live = r < n_rows;
  uint32_t u = INVALID_U32, deg = 0;
  if (live) {
    u = dict.lookup(from[r]);
    if (u != INVALID_U32) deg = off[u + 1] - off[u];  // (u < V: off has V + 1 entries)
  }
  // (the prefixes are exact whenever they are used: rows are only written if fewer than 2^32 come out in all)
  const uint32_t incl = wave_scan_incl(deg);
  const uint64_t sum = wave_reduce_add_u64(deg), hit = __ballot(deg != 0);
  if (lane == 0) s_sum[wave] = sum, s_hit[wave] = (uint32_t)__popcll(hit);
  __syncthreads();
  uint32_t before = incl - deg;
  for (int w = 0; w < wave; w++) before += (uint32_t)s_sum[w];
  if (live && u_rows) u_rows[r] = u, pre[r] = before;
  if (threadIdx.x == 0) {
    group[g] = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
    const uint32_t hits = s_hit[0] + s_hit[1] + s_hit[2] + s_hit[3];
    if (hits) atomicAdd(matched, (unsigned long long)hits);
  }
}

// first output row of input row r (fewer than 2^32 output rows: 32 bits hold it)
__device__ __forceinline__ uint32_t ex_prefix(const uint64_t *__restrict__ group, const uint32_t *__restrict__ pre,
                                              uint64_t r) {
  return (uint32_t)group[r >> 8] + pre[r];
}

// the last row r in [lo, hi] with P(r) <= p, given P(lo) <= p: the row that owns output row p if p < the total — of the
// rows that start at p every one but the last has no edge row
__device__ __forceinline__ uint64_t ex_owner(const uint64_t *__restrict__ group, const uint32_t *__restrict__ pre,
                                             uint64_t lo, uint64_t hi, uint32_t p) {
  uint64_t a = lo + 1, b = hi + 1;  // first row in (lo, hi + 1] with P > p
  while (a < b) {
    const uint64_t mid = (a + b) >> 1;
    if (ex_prefix(group, pre, mid) <= p) a = mid + 1; else b = mid;
  }
  return a - 1;
}

// tile_row[t], t < n_tiles: the input row that owns output row t * tile_rows; tile_row[n_tiles]: the owner of the last one
__global__ __launch_bounds__(256) void k_extend_tiles(const uint64_t *__restrict__ group, const uint32_t *__restrict__ pre,
                                                      uint64_t n_rows, uint32_t total, uint32_t tile_rows,
                                                      uint64_t n_tiles, uint64_t *__restrict__ tile_row) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t > n_tiles) return;
  const uint32_t p = t < n_tiles ? (uint32_t)(t * tile_rows) : total - 1;  // (t * tile_rows < total < 2^32)
  tile_row[t] = ex_owner(group, pre, 0, n_rows - 1, p);                    // (P(0) = 0 <= p)
}

struct ExWrite {
  ExIn in;
  ExOut out;
  int ncols;  // hops + 1 id columns of the input
  uint64_t n_rows;
  uint32_t total, tile_rows;
  const uint64_t *group;
  const uint32_t *pre, *u_rows;
  const uint64_t *tile_row;
  const uint32_t *off, *nbr, *epos;
  const int64_t *vid, *eid;  // eid nullable: the rowid is epos
};

// Workgroup t0 + blockIdx.x writes output rows [t * tile_rows, min(total, (t + 1) * tile_rows)).
template <bool EDGES>
__global__ __launch_bounds__(256) void k_extend_write(ExWrite X, uint64_t t0) {
  __shared__ uint32_t s_pre[EX_WIN];
  const uint64_t t = t0 + blockIdx.x;
  const uint64_t r_lo = X.tile_row[t], r_hi = X.tile_row[t + 1];  // (r_lo <= r_hi < n_rows: owners of ascending rows)
  const uint64_t span = r_hi - r_lo + 1;
  const uint32_t n_win = span < EX_WIN ? (uint32_t)span : EX_WIN;
  for (uint32_t j = threadIdx.x; j < n_win; j += 256) s_pre[j] = ex_prefix(X.group, X.pre, r_lo + j);
  __syncthreads();
  const uint32_t p0 = (uint32_t)(t * X.tile_rows);
  const uint32_t len = X.total - p0 < X.tile_rows ? X.total - p0 : X.tile_rows;
  // Every lane first finds the parent row and the CSR entry of its (up to EX_PER) output rows, then the columns are
  // written one after the other: a column's two pointers are live for its own copies only.
  uint64_t row[EX_PER];
  uint32_t at[EX_PER];
#pragma unroll
  for (int q = 0; q < EX_PER; q++) {
    const uint32_t i = threadIdx.x + 256u * q;
    row[q] = r_lo, at[q] = 0;
    if (i < len) {
      const uint32_t p = p0 + i;
      uint32_t lo = 1, hi = n_win;  // first idx in [1, n_win] with s_pre[idx] > p  (s_pre[0] = P(r_lo) <= p0 <= p)
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (s_pre[mid] <= p) lo = mid + 1; else hi = mid;
      }
      uint64_t r = r_lo + lo - 1;
      uint32_t start = s_pre[lo - 1];
      if (lo == n_win && span > n_win) {  // the window ended inside the span (rows without an edge row): finish in global memory
        r = ex_owner(X.group, X.pre, r, r_hi, p);
        start = ex_prefix(X.group, X.pre, r);
      }
      // (p < total, so row r has an edge row: u is a vertex and p - start < its degree; the entry lies inside nbr)
      row[q] = r, at[q] = X.off[X.u_rows[r]] + (p - start);
    }
  }
#pragma unroll
  for (int c = 0; c <= GG_MAX_HOPS; c++) {
    if (c > X.ncols) break;
    int64_t *__restrict__ o = X.out.c[c] + p0;
    if (c < X.ncols) {
      const int64_t *__restrict__ in = X.in.c[c];
#pragma unroll
      for (int q = 0; q < EX_PER; q++)
        if (threadIdx.x + 256u * q < len) o[threadIdx.x + 256u * q] = in[row[q]];
    } else {
#pragma unroll
      for (int q = 0; q < EX_PER; q++)
        if (threadIdx.x + 256u * q < len) o[threadIdx.x + 256u * q] = X.vid[X.nbr[at[q]]];
    }
  }
  if (EDGES) {
#pragma unroll
    for (int c = 0; c < GG_MAX_HOPS; c++) {
      if (c >= X.ncols) break;
      int64_t *__restrict__ o = X.out.e[c] + p0;
      if (c < X.ncols - 1) {
        const int64_t *__restrict__ in = X.in.e[c];  // null: the input has no edge columns
#pragma unroll
        for (int q = 0; q < EX_PER; q++)
          if (threadIdx.x + 256u * q < len) o[threadIdx.x + 256u * q] = in ? in[row[q]] : -1;
      } else {
#pragma unroll
        for (int q = 0; q < EX_PER; q++)
          if (threadIdx.x + 256u * q < len)
            o[threadIdx.x + 256u * q] = X.eid ? X.eid[at[q]] : (int64_t)X.epos[at[q]];
      }
    }
  }
}

}  // namespace gg

extern "C" int gg_result_extend_edge(gg_ctx *ctx, const gg_result *res, int hops, const gg_csr *csr_c, int from_col,
                                     int want_edges, int materialise, gg_extend_stats *stats, gg_result **out_result) {
  if (out_result) *out_result = nullptr;
  if (stats) memset(stats, 0, sizeof(*stats));
  const char *fn = "gg_result_extend_edge";
  GG_TRY(result_arg(fn, ctx, res));
  GG_TRY(csr_arg(fn, ctx, csr_c));
  if (materialise && !out_result) {
    set_error("%s: materialise without out_result", fn);
    return GG_ERR_INVALID_ARG;
  }
  GG_TRY(whole_csr(fn, csr_c, "the joined table"));
  GG_TRY(walk_kind_arg(fn, res, KindRule::STATE));
  GG_TRY(hops_arg(fn, res, hops, GG_MAX_HOPS - 1));  // (the output has hops + 1)
  GG_TRY(column_arg(fn, "from", from_col, 0, hops));
  if (want_edges && !csr_c->has_rowid) {
    set_error("%s: edge columns need a CSR built with edge rowids (gg_ctx_set_edge_rowid(ctx, 1))", fn);
    return GG_ERR_STATE;
  }
  ApiScope scope(ctx);
  GG_HIP(hipSetDevice(ctx->device));
  gg_csr *csr = const_cast<gg_csr *>(csr_c);
  const uint64_t n_rows = res->rows[hops];
  const int out_hops = hops + 1;
  ResultOwner o;
  // table hops + 1: v0..v_hops, w (and e1..e_{hops+1})
  if (materialise) o = make_result(ctx, ResultKind::TABLES, out_hops, out_hops);
  uint64_t total = 0, matched = 0;
  if (n_rows && csr->V && csr->E) {  // (without an edge row nothing matches: nothing to look up)
    DictView dict;
    GG_TRY(dict_view(ctx, csr, &dict));
    const uint64_t groups = (n_rows + 255) / 256;
    uint32_t *u_rows = nullptr, *pre = nullptr;
    uint64_t *group = nullptr;
    unsigned long long *matched_dev = nullptr;
    if (materialise) {
      GG_TRY(ctx->dev_alloc((void **)&u_rows, n_rows * sizeof(uint32_t)));
      GG_TRY(ctx->dev_alloc((void **)&pre, n_rows * sizeof(uint32_t)));
    }
    GG_TRY(ctx->dev_alloc((void **)&group, groups * sizeof(uint64_t)));
    GG_TRY(ctx->dev_alloc((void **)&matched_dev, sizeof(unsigned long long)));
    GG_HIP(hipMemsetAsync(matched_dev, 0, sizeof(unsigned long long), ctx->stream));
    GG_TRY(split_groups(ctx, groups, [&](uint64_t g0, uint64_t ng) -> int {
      GG_LAUNCH(ctx, "k_extend_count", k_extend_count, dim3((unsigned)ng), dim3(256), 0, res->cols[hops][from_col], g0,
                n_rows, dict, (const uint32_t *)csr->off, u_rows, pre, group, matched_dev);
      return GG_OK;
    }));
    GG_TRY(scan_total_u64(ctx, group, group, groups, &total, false, {{matched_dev, sizeof(uint64_t), &matched}}));
    if (materialise && total) {
      if (total >= (1ull << 32)) {
        set_error("gg_result_extend_edge: %llu rows to materialise (2^32 or more); count them, or extend a smaller table",
                  (unsigned long long)total);
        return GG_ERR_TOO_LARGE;
      }
      ExWrite X{};
      X.ncols = hops + 1;
      X.n_rows = n_rows;
      X.total = (uint32_t)total;
      X.tile_rows = ctx->extend_tile_rows && ctx->extend_tile_rows < EX_TILE_ROWS ? ctx->extend_tile_rows : EX_TILE_ROWS;
      X.group = group, X.pre = pre, X.u_rows = u_rows;
      X.off = csr->off, X.nbr = csr->nbr, X.vid = csr->vid, X.epos = csr->epos, X.eid = csr->eid;
      const bool in_edges = want_edges && walk_edge_columns(res, hops);
      for (int c = 0; c <= hops; c++) X.in.c[c] = res->cols[hops][c];
      for (int c = 0; c < hops; c++) X.in.e[c] = in_edges ? res->ecols[hops][c] : nullptr;
      GG_TRY(alloc_kept_columns(ctx, o->cols[out_hops], out_hops + 1, total));
      for (int c = 0; c <= out_hops; c++) X.out.c[c] = o->cols[out_hops][c];
      if (want_edges) GG_TRY(alloc_kept_columns(ctx, o->ecols[out_hops], out_hops, total));
      for (int c = 0; want_edges && c < out_hops; c++) X.out.e[c] = o->ecols[out_hops][c];
      const uint64_t n_tiles = (total + X.tile_rows - 1) / X.tile_rows;
      uint64_t *tile_row = nullptr;
      GG_TRY(ctx->dev_alloc((void **)&tile_row, (n_tiles + 1) * sizeof(uint64_t)));
      X.tile_row = tile_row;
      GG_LAUNCH(ctx, "k_extend_tiles", k_extend_tiles, dim3((unsigned)((n_tiles + 1 + 255) / 256)), dim3(256), 0,
                (const uint64_t *)group, (const uint32_t *)pre, n_rows, X.total, X.tile_rows, n_tiles, tile_row);
      GG_TRY(split_groups(ctx, n_tiles, [&](uint64_t t0, uint64_t nt) -> int {
        if (want_edges)
          GG_LAUNCH(ctx, "k_extend_write_edges", (k_extend_write<true>), dim3((unsigned)nt), dim3(256), 0, X, t0);
        else
          GG_LAUNCH(ctx, "k_extend_write", (k_extend_write<false>), dim3((unsigned)nt), dim3(256), 0, X, t0);
        return GG_OK;
      }));
      GG_TRY(sync_checked(ctx));
    }
  }
  if (stats) stats->rows_in = n_rows, stats->rows_out = total, stats->rows_matched = matched;
  if (materialise) {
    o->rows[out_hops] = total;
    *out_result = o.release();
  }
  return GG_OK;
}

extern "C" int gg_debug_extend(gg_ctx *ctx, uint32_t tile_rows) {
  if (!ctx) return GG_ERR_INVALID_ARG;
  ctx->extend_tile_rows = tile_rows;
  return GG_OK;
}
