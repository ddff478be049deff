// gg_pairs.hip — count(*) over the h-hop walks grouped by BOTH ends: one row (source, end vertex, walks) per pair.
//
// The reference answers `SELECT p1.id, p2.id, count(*) ... GROUP BY p1.id, p2.id` (the pair form of
// benchmark/ldbc/queries/bi-14.sql:103-112; h = 2 over a mirrored knows is the mutual-friend count behind
// interactive-complex-10.sql:19-24, and the rows with walks != 0 are the SELECT DISTINCT p1, p2 of bi-14.sql:30-102) with
// PhysicalHashAggregate on two keys (src/execution/operator/aggregate/physical_hash_aggregate.cpp:152-266) above the
// hash-join chain (ScanStructure::NextInnerJoin, src/execution/join_hashtable.cpp:442-476): every walk row is formed and
// folded away again.  The answer is a sparse matrix product.  With w_0 = the indicator of source s and
//     w_h(v) = sum over the entries u of v's reverse row of w_{h-1}(u)
// w_h(v) is the number of h-walks s -> v.  One wavefront lane carries one source (gg_bfs64's organisation), so a vertex's
// state is 64 u64 counts, 512 B, which a wavefront reads in one coalesced access; the BFS's 64-bit frontier word becomes
// the mask of the lanes of a vertex that are not 0, and a gather whose mask is 0 is skipped.
//   W[v * 64 + lane]  u64 counts, two buffers swapped per level; a row whose mask is 0 is never read, so it is neither
//                     written nor cleared (gather_mode 1 reads every row and therefore clears both buffers first and
//                     writes every row)
//   mask[v]           bit l set iff W[v * 64 + l] != 0; written for every vertex by every pass
//   k_pc_seed         W0[s * 64 + i] = 1, mask0[s] |= 1 << i for lane i with dense index s (the only atomics; none on W)
//   k_pc_long_flag / scan / k_pc_long_list   the in-rows longer than the threshold, once per call (as k_agg_long_list)
//   k_pc_pull         one wavefront per vertex of up to `threshold` in-entries: 64 entries and their masks are loaded a
//                     lane each, the entries with a mask are taken four at a time — four independent 512-B gathers in
//                     flight instead of a chain — each lane adding W[u * 64 + lane] where its bit of the mask is set;
//                     new_mask[v] = ballot(acc != 0), the row is written only if that is not 0
//   k_pc_pull_long    one workgroup of 256 per listed row: its four wavefronts take every fourth 64-entry chunk and fold
//                     their 64 partials through LDS (4 x 64 u64); addition mod 2^64 commutes, so the same bits
//   k_pc_targets      flag[v] = 1 for the listed end vertices
//   k_pc_count        tiles of 64 vertices, a wavefront per tile, lane = source lane: cnt[lane * n_tiles + tile] = the
//                     lane's pairs in the tile that pass the target filter; + the level's walks
//   scan              exclusive prefix over that lane-major, tile-minor array: the order (source index, dense index)
//   k_pc_write        the tile again with a per-lane cursor: (lane, vertex id, walks) into three int64 columns
// Bytes per pass (model): E * (4 B entry + 8 B mask) + rows_gathered * 512 B + V * (8 B offsets + 8 B mask) + 512 B per
// vertex written.  The gathered table is 512 V bytes (about 230 MB at SF100); whether its rows are served from L2 /
// Infinity Cache is not measured here.
#include "gg_internal.h"

using namespace gg;

namespace gg {
namespace {

constexpr uint32_t PC_LONG_ROW = 512;  // default: rows of more entries go to a whole workgroup
constexpr int PC_LANES = GG_BFS_LANES;
static_assert(PC_LANES == 64, "one wavefront lane per source");

__device__ __forceinline__ uint64_t readlane_u64(uint64_t x, int j) {  // j wave-uniform
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, j);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), j);
  return ((uint64_t)hi << 32) | lo;
}

__global__ __launch_bounds__(64) void k_pc_seed(const uint32_t *__restrict__ dense, int n_src,
                                                uint64_t *__restrict__ W, unsigned long long *__restrict__ mask) {
  const int i = threadIdx.x;
  if (i < n_src && dense[i] != INVALID_U32) {  // (dense[i] < V: W has 64 V entries, mask V)
    W[(uint64_t)dense[i] * PC_LANES + i] = 1;
    atomicOr(&mask[dense[i]], 1ull << i);
  }
}

__global__ __launch_bounds__(256) void k_pc_long_flag(const uint32_t *__restrict__ off, uint64_t V, uint32_t threshold,
                                                      uint32_t *__restrict__ flag) {
  for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (uint64_t)gridDim.x * blockDim.x)
    flag[v] = off[v + 1] - off[v] > threshold ? 1u : 0u;
}

// pos: the exclusive prefix of the flags
__global__ __launch_bounds__(256) void k_pc_long_list(const uint32_t *__restrict__ off, uint64_t V, uint32_t threshold,
                                                      const uint32_t *__restrict__ pos, uint32_t *__restrict__ list) {
  for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (uint64_t)gridDim.x * blockDim.x)
    if (off[v + 1] - off[v] > threshold) list[pos[v]] = (uint32_t)v;  // (pos[v] < number of long rows <= V)
}

// The calling wavefront's share of the reverse row [lo, hi): the 64-entry chunks that start at lo + first, lo + first +
// stride, ...  Every argument but `lane` is wave-uniform.  *gathered += the entries whose state row was read.
__device__ __forceinline__ uint64_t pc_pull_span(const uint32_t *__restrict__ rnbr,
                                                 const unsigned long long *__restrict__ mask,
                                                 const uint64_t *__restrict__ W, uint64_t lo, uint64_t hi, uint32_t first,
                                                 uint32_t stride, bool all, int lane, uint64_t *gathered) {
  uint64_t acc = 0;
  for (uint64_t c = lo + first; c < hi; c += stride) {
    const uint64_t i = c + lane;
    uint32_t un = 0;
    uint64_t mk = 0;
    if (i < hi) {  // (i < hi <= E)
      un = rnbr[i];
      mk = all ? ~0ull : mask[un];  // (un < V)
    }
    uint64_t live = __ballot(mk != 0);
    *gathered += (uint64_t)__popcll(live);
    while (live) {
      uint32_t u[4];
      uint64_t m[4], x[4];
#pragma unroll
      for (int q = 0; q < 4; q++) {
        u[q] = 0, m[q] = 0;
        if (live) {
          const int j = __builtin_ctzll(live);
          live &= live - 1;
          u[q] = (uint32_t)__builtin_amdgcn_readlane((int)un, j);
          m[q] = readlane_u64(mk, j);
        }
      }
#pragma unroll
      for (int q = 0; q < 4; q++) x[q] = (m[q] >> lane) & 1 ? W[(uint64_t)u[q] * PC_LANES + lane] : 0;
      acc += (x[0] + x[1]) + (x[2] + x[3]);
    }
  }
  return acc;
}

// one wavefront per vertex; rows longer than the threshold are left to k_pc_pull_long
__global__ __launch_bounds__(256) void k_pc_pull(const uint32_t *__restrict__ roff, const uint32_t *__restrict__ rnbr,
                                                 const unsigned long long *__restrict__ mask,
                                                 const uint64_t *__restrict__ W, uint64_t V, uint32_t threshold, int all,
                                                 unsigned long long *__restrict__ new_mask, uint64_t *__restrict__ Wn,
                                                 unsigned long long *__restrict__ gathered_total) {
  const int lane = threadIdx.x & 63;
  uint64_t gathered = 0;
  for (uint64_t v = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); v < V; v += (uint64_t)gridDim.x * 4) {
    const uint32_t lo = roff[v], hi = roff[v + 1];
    if (hi - lo > threshold) continue;
    const uint64_t acc = pc_pull_span(rnbr, mask, W, lo, hi, 0, 64, all != 0, lane, &gathered);
    const uint64_t nm = __ballot(acc != 0);
    if (nm || all) Wn[v * PC_LANES + lane] = acc;
    if (lane == 0) new_mask[v] = nm;
  }
  if (lane == 0 && gathered) atomicAdd(gathered_total, (unsigned long long)gathered);
}

// one workgroup per listed row (workgroups stride over the list: its length is a device word, no host round trip)
__global__ __launch_bounds__(256) void k_pc_pull_long(const uint32_t *__restrict__ roff, const uint32_t *__restrict__ rnbr,
                                                      const unsigned long long *__restrict__ mask,
                                                      const uint64_t *__restrict__ W, const uint32_t *__restrict__ list,
                                                      const uint64_t *__restrict__ n_list, int all,
                                                      unsigned long long *__restrict__ new_mask,
                                                      uint64_t *__restrict__ Wn,
                                                      unsigned long long *__restrict__ gathered_total) {
  __shared__ uint64_t s_part[4][PC_LANES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t n = *n_list;
  uint64_t gathered = 0;
  for (uint64_t r = blockIdx.x; r < n; r += gridDim.x) {
    const uint32_t v = list[r];
    const uint32_t lo = roff[v], hi = roff[v + 1];
    s_part[wave][lane] = pc_pull_span(rnbr, mask, W, lo, hi, (uint32_t)wave * 64, 256, all != 0, lane, &gathered);
    __syncthreads();
    if (wave == 0) {
      const uint64_t acc = (s_part[0][lane] + s_part[1][lane]) + (s_part[2][lane] + s_part[3][lane]);
      const uint64_t nm = __ballot(acc != 0);
      if (nm || all) Wn[(uint64_t)v * PC_LANES + lane] = acc;
      if (lane == 0) new_mask[v] = nm;
    }
    __syncthreads();  // (s_part is written again by the next row)
  }
  if (lane == 0 && gathered) atomicAdd(gathered_total, (unsigned long long)gathered);
}

__global__ __launch_bounds__(256) void k_pc_targets(const uint32_t *__restrict__ dense, uint64_t n,
                                                    uint8_t *__restrict__ flag) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    if (dense[i] != INVALID_U32) flag[dense[i]] = 1;  // (dense[i] < V; duplicates write the same byte)
}

// the masks of tile `tile` that pass the target filter, one vertex a lane (0 past V)
__device__ __forceinline__ uint64_t pc_tile_mask(const unsigned long long *__restrict__ mask,
                                                 const uint8_t *__restrict__ tflag, uint64_t V, uint64_t tile, int lane) {
  const uint64_t v = tile * 64 + lane;
  uint64_t mk = v < V ? mask[v] : 0;
  if (mk && tflag && !tflag[v]) mk = 0;
  return mk;
}

// cnt[lane * n_tiles + tile] = pairs of source lane `lane` in the tile; *walks += their walks (mod 2^64)
__global__ __launch_bounds__(256) void k_pc_count(const unsigned long long *__restrict__ mask,
                                                  const uint64_t *__restrict__ W, const uint8_t *__restrict__ tflag,
                                                  uint64_t V, uint64_t n_tiles, uint32_t *__restrict__ cnt,
                                                  unsigned long long *__restrict__ walks) {
  const int lane = threadIdx.x & 63;
  uint64_t sum = 0;
  for (uint64_t tile = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); tile < n_tiles; tile += (uint64_t)gridDim.x * 4) {
    const uint64_t mk = pc_tile_mask(mask, tflag, V, tile, lane);
    uint64_t live = __ballot(mk != 0);
    uint32_t c = 0;
    while (live) {
      const int j = __builtin_ctzll(live);
      live &= live - 1;
      if ((readlane_u64(mk, j) >> lane) & 1) {
        c++;
        sum += W[(tile * 64 + j) * PC_LANES + lane];  // (tile * 64 + j < V: its mask is not 0)
      }
    }
    cnt[(uint64_t)lane * n_tiles + tile] = c;
  }
  sum = wave_reduce_add_u64(sum);
  if (lane == 0 && sum) atomicAdd(walks, (unsigned long long)sum);
}

// pos: the exclusive prefix of cnt; the level's total (< 2^32, checked by the caller) is the columns' length
__global__ __launch_bounds__(256) void k_pc_write(const unsigned long long *__restrict__ mask,
                                                  const uint64_t *__restrict__ W, const uint8_t *__restrict__ tflag,
                                                  uint64_t V, uint64_t n_tiles, const uint32_t *__restrict__ pos,
                                                  const int64_t *__restrict__ vid, int64_t *__restrict__ out_src,
                                                  int64_t *__restrict__ out_id, int64_t *__restrict__ out_walks) {
  const int lane = threadIdx.x & 63;
  for (uint64_t tile = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); tile < n_tiles; tile += (uint64_t)gridDim.x * 4) {
    const uint64_t mk = pc_tile_mask(mask, tflag, V, tile, lane);
    uint64_t live = __ballot(mk != 0);
    uint32_t at = pos[(uint64_t)lane * n_tiles + tile];
    while (live) {
      const int j = __builtin_ctzll(live);
      live &= live - 1;
      if ((readlane_u64(mk, j) >> lane) & 1) {  // (at < pos of the next (lane, tile) <= the level's total)
        const uint64_t v = tile * 64 + j;
        out_src[at] = lane;
        out_id[at] = vid[v];
        out_walks[at] = (int64_t)W[v * PC_LANES + lane];
        at++;
      }
    }
  }
}

inline dim3 wave_grid(gg_ctx *ctx, uint64_t n) {  // 256-thread workgroups, a wavefront per item, striding
  const uint64_t want = (n + 3) / 4, cap = (uint64_t)ctx->num_cus * 32;
  return dim3((unsigned)(want < cap ? (want ? want : 1) : cap));
}

}  // namespace
}  // namespace gg

extern "C" int gg_khop_pair_counts(gg_ctx *ctx, const gg_csr *csr_c, const int64_t *src_ids, int n_src, int k_min,
                                   int k_max, const int64_t *dst_ids, uint64_t n_dst, gg_pair_stats *stats,
                                   gg_result **out_result) {
  if (out_result) *out_result = nullptr;
  if (stats) memset(stats, 0, sizeof(*stats));
  if (!ctx || !csr_c || csr_c->ctx != ctx || !src_ids) {
    set_error("gg_khop_pair_counts: bad context / csr / source argument");
    return GG_ERR_INVALID_ARG;
  }
  if (n_src < 1 || n_src > GG_BFS_LANES) {
    set_error("gg_khop_pair_counts: %d sources outside 1..%d (one wavefront lane each)", n_src, GG_BFS_LANES);
    return GG_ERR_INVALID_ARG;
  }
  if (k_min < 1 || k_max > GG_MAX_HOPS || k_min > k_max) {
    set_error("gg_khop_pair_counts: hops %d..%d outside 1..%d", k_min, k_max, GG_MAX_HOPS);
    return GG_ERR_INVALID_ARG;
  }
  if (!dst_ids && n_dst) {
    set_error("gg_khop_pair_counts: %llu targets without a list", (unsigned long long)n_dst);
    return GG_ERR_INVALID_ARG;
  }
  if (!stats && !out_result) {
    set_error("gg_khop_pair_counts: neither stats nor out_result is asked for");
    return GG_ERR_INVALID_ARG;
  }
  if (csr_c->n_parts > 1) {
    set_error("gg_khop_pair_counts needs a whole CSR, not a shard (gg_csr_build_shard)");
    return GG_ERR_STATE;
  }
  ApiScope scope(ctx);
  GG_HIP(hipSetDevice(ctx->device));
  gg_csr *csr = const_cast<gg_csr *>(csr_c);
  const uint64_t V = csr->V, E = csr->E;
  ResultOwner res;
  if (out_result) res = make_result(ctx, ResultKind::PAIR_COUNTS, k_min, k_max);
  if (V && E) {
    hipStream_t st = ctx->stream;
    GG_TRY(ensure_reverse(ctx, csr));
    const uint32_t threshold = ctx->pc_long_row ? ctx->pc_long_row : PC_LONG_ROW;
    const int all = ctx->pc_gather_mode == 1;

    // device words: pairs[h], walks[h], rows gathered, then the number of long rows
    uint64_t *words = nullptr;
    constexpr int NW = 2 * (GG_MAX_HOPS + 1) + 2;
    GG_TRY(ctx->dev_alloc((void **)&words, NW * sizeof(uint64_t)));
    GG_HIP(hipMemsetAsync(words, 0, NW * sizeof(uint64_t), st));
    uint64_t *d_pairs = words, *d_walks = words + GG_MAX_HOPS + 1, *d_gathered = words + 2 * (GG_MAX_HOPS + 1);
    uint64_t *d_nlong = d_gathered + 1;

    // the state: 2 x 512 V bytes (GG_ERR_OOM from the pool if they do not fit)
    uint64_t *W[2] = {nullptr, nullptr};
    unsigned long long *mask[2] = {nullptr, nullptr};
    for (int b = 0; b < 2; b++) {
      GG_TRY(ctx->dev_alloc((void **)&W[b], V * PC_LANES * sizeof(uint64_t)));
      GG_TRY(ctx->dev_alloc((void **)&mask[b], V * sizeof(uint64_t)));
      if (all) GG_HIP(hipMemsetAsync(W[b], 0, V * PC_LANES * sizeof(uint64_t), st));
    }
    GG_HIP(hipMemsetAsync(mask[0], 0, V * sizeof(uint64_t), st));

    const dim3 vgrid = stride_grid(ctx, V);
    const uint32_t *list = nullptr;
    if (threshold != UINT32_MAX) {
      uint32_t *flag = nullptr, *l = nullptr;
      GG_TRY(ctx->dev_alloc((void **)&flag, V * sizeof(uint32_t)));
      GG_TRY(ctx->dev_alloc((void **)&l, V * sizeof(uint32_t)));
      GG_LAUNCH(ctx, "pc_long_flag", k_pc_long_flag, vgrid, dim3(256), 0, (const uint32_t *)csr->roff, V, threshold, flag);
      GG_TRY(scan_exclusive_u32(ctx, flag, flag, V, d_nlong));
      GG_LAUNCH(ctx, "pc_long_list", k_pc_long_list, vgrid, dim3(256), 0, (const uint32_t *)csr->roff, V, threshold,
                (const uint32_t *)flag, l);
      ctx->dev_free(flag);
      list = l;
    }

    uint32_t *dense = nullptr;
    GG_TRY(upload_ids(ctx, csr, src_ids, (uint64_t)n_src, &dense));
    GG_LAUNCH(ctx, "pc_seed", k_pc_seed, dim3(1), dim3(64), 0, (const uint32_t *)dense, n_src, W[0], mask[0]);

    uint8_t *tflag = nullptr;  // null: every vertex may end a row
    if (dst_ids) {
      uint32_t *tdense = nullptr;
      GG_TRY(ctx->dev_alloc((void **)&tflag, V));
      GG_HIP(hipMemsetAsync(tflag, 0, V, st));
      GG_TRY(upload_ids(ctx, csr, dst_ids, n_dst, &tdense));
      if (n_dst)
        GG_LAUNCH(ctx, "pc_targets", k_pc_targets, stride_grid(ctx, n_dst), dim3(256), 0, (const uint32_t *)tdense, n_dst,
                  tflag);
    }

    const uint64_t n_tiles = (V + 63) / 64;
    uint32_t *cnt = nullptr;  // 64 x n_tiles, lane-major
    GG_TRY(ctx->dev_alloc((void **)&cnt, PC_LANES * n_tiles * sizeof(uint32_t)));
    const dim3 pull_grid = wave_grid(ctx, V), tile_grid = wave_grid(ctx, n_tiles);
    const uint64_t long_cap = (uint64_t)ctx->num_cus * 8;
    int cur = 0;
    for (int h = 1; h <= k_max; h++) {
      const int nxt = cur ^ 1;
      GG_LAUNCH(ctx, "pc_pull", k_pc_pull, pull_grid, dim3(256), 0, (const uint32_t *)csr->roff,
                (const uint32_t *)csr->rnbr_rows, (const unsigned long long *)mask[cur], (const uint64_t *)W[cur], V, threshold,
                all, mask[nxt], W[nxt], (unsigned long long *)d_gathered);
      if (list)
        GG_LAUNCH(ctx, "pc_pull_long", k_pc_pull_long, dim3((unsigned)(V < long_cap ? V : long_cap)), dim3(256), 0,
                  (const uint32_t *)csr->roff, (const uint32_t *)csr->rnbr_rows, (const unsigned long long *)mask[cur],
                  (const uint64_t *)W[cur], list, (const uint64_t *)d_nlong, all, mask[nxt], W[nxt],
                  (unsigned long long *)d_gathered);
      cur = nxt;
      if (h < k_min) continue;
      GG_LAUNCH(ctx, "pc_count", k_pc_count, tile_grid, dim3(256), 0, (const unsigned long long *)mask[cur],
                (const uint64_t *)W[cur], (const uint8_t *)tflag, V, n_tiles, cnt, (unsigned long long *)(d_walks + h));
      GG_TRY(scan_exclusive_u32(ctx, cnt, cnt, PC_LANES * n_tiles, d_pairs + h));
      if (!res) continue;
      // the columns are sized from the level's own count: one read-back per reported level
      uint64_t n_rows = 0;
      GG_TRY(read_back(ctx, {{d_pairs + h, sizeof(uint64_t), &n_rows}}));
      if (n_rows >= (1ull << 32)) {
        set_error("gg_khop_pair_counts: level %d has %llu rows (2^32 or more): ask for fewer sources or targets", h,
                  (unsigned long long)n_rows);
        return GG_ERR_TOO_LARGE;
      }
      res->rows[h] = n_rows;
      if (!n_rows) continue;
      for (int c = 0; c < 3; c++) {
        GG_TRY(ctx->dev_alloc((void **)&res->cols[h][c], n_rows * sizeof(int64_t)));
        ctx->keep(res->cols[h][c]);
      }
      GG_LAUNCH(ctx, "pc_write", k_pc_write, tile_grid, dim3(256), 0, (const unsigned long long *)mask[cur],
                (const uint64_t *)W[cur], (const uint8_t *)tflag, V, n_tiles, (const uint32_t *)cnt,
                (const int64_t *)csr->vid, res->cols[h][0], res->cols[h][1], res->cols[h][2]);
    }
    uint64_t hw[2 * (GG_MAX_HOPS + 1) + 1];
    GG_TRY(read_back(ctx, {{words, sizeof(hw), hw}}));
    for (int h = k_min; h <= k_max; h++)
      if (hw[h] >= (1ull << 32)) {  // (stats only: the same refusal, from the same 64-bit count)
        set_error("gg_khop_pair_counts: level %d has %llu rows (2^32 or more)", h, (unsigned long long)hw[h]);
        return GG_ERR_TOO_LARGE;
      }
    if (stats) {
      for (int h = k_min; h <= k_max; h++) stats->pairs[h] = hw[h], stats->walks[h] = hw[GG_MAX_HOPS + 1 + h];
      stats->entries_pulled = (uint64_t)k_max * E;
      stats->rows_gathered = hw[2 * (GG_MAX_HOPS + 1)];
    }
  }
  if (out_result) *out_result = res.release();
  return GG_OK;
}

extern "C" int gg_khop_pair_counts_rows(const gg_result *res, int hops, uint64_t *n_rows) {
  if (!res || !n_rows) return GG_ERR_INVALID_ARG;
  GG_TRY(expect_kind(res, ResultKind::PAIR_COUNTS, "gg_khop_pair_counts_rows"));
  if (hops < res->k_min || hops > res->k_max) return GG_ERR_INVALID_ARG;
  *n_rows = res->rows[hops];
  return GG_OK;
}

extern "C" int gg_khop_pair_counts_fetch(const gg_result *res, int hops, uint64_t offset, uint32_t max_rows,
                                         int64_t *src_index, int64_t *vertex_id, uint64_t *walks, uint32_t *n_out) {
  if (!res || !n_out) return GG_ERR_INVALID_ARG;
  GG_TRY(expect_kind(res, ResultKind::PAIR_COUNTS, "gg_khop_pair_counts_fetch"));
  if (hops < res->k_min || hops > res->k_max) return GG_ERR_INVALID_ARG;
  int64_t *const *col = res->cols[hops];
  return fetch_slice(res->ctx, res->rows[hops], offset, max_rows,
                     {{src_index, col[0]}, {vertex_id, col[1]}, {walks, col[2]}}, n_out);
}

extern "C" int gg_debug_pair_counts(gg_ctx *ctx, uint32_t long_row_entries, int gather_mode) {
  if (!ctx || gather_mode < 0 || gather_mode > 1) return GG_ERR_INVALID_ARG;
  ctx->pc_long_row = long_row_entries;
  ctx->pc_gather_mode = gather_mode;
  return GG_OK;
}
