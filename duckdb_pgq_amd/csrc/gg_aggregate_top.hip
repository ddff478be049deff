// gg_aggregate_top.hip — the best n groups of one level of a grouped aggregate, ordered on the device.
//
// The reference ends its aggregating statements with `ORDER BY <aggregate> DESC, <id> LIMIT n`
// (benchmark/ldbc/queries/bi-8.sql:41-53: ORDER BY p.score + sum(f.score) DESC, p.personid LIMIT 100) and runs that tail as
// PhysicalTopN (src/execution/operator/order/physical_top_n.cpp:238-293 heap sink / reduce, :421-454 Sink / Combine) directly
// above PhysicalHashAggregate.  Here the groups are already columns in HBM (gg_aggregate.hip), so the order is made where
// they lie and only the n rows of the answer cross the link.
//
// Every row has one 192-bit unsigned key in which smaller is better, three words (w2, w1, w0), never stored:
//   w2:w1  the 128-bit total (+ the row's bias) with its sign bit flipped, or (0, walks); complemented if descending
//          (for walks w2 stays 0 in both directions: the digit passes start below it)
//   w0     the vertex id with its sign bit flipped, never complemented: ORDER BY key [DESC], id
// Ids are unique within a level, so keys are: the n-th smallest key exists and exactly n rows are not above it.
//   k_top_bias      bias of every row's vertex (through the CSR's id dictionary), and how many ids are no vertices
//   k_top_hist      one digit pass, most significant byte first: 256 bins of byte b over the rows that match the prefix
//                   fixed so far — per-wave bins in LDS, folded per workgroup, one global add per non-empty bin; a tile
//                   of TOP_TILE consecutive rows per workgroup, whose candidate count is kept per tile
//   k_top_pick      one workgroup: scans the bins, fixes byte b of the prefix and the rank that remains below it.  The
//                   selection is decided ("done") as soon as the rank equals the candidates left: every one of them is in.
//                   When the candidates fall to candidate_floor or fewer (and to half the rows or fewer), the NEXT pass's
//                   tile counts are scanned here and k_top_compact writes the candidates' row numbers, in input order, to a
//                   list; later passes read the list only.
//   k_top_compact   (k_top_place<0>) count, scan, write: a tile's place is the scan of the tile counts, a row's place
//                   inside the tile a workgroup scan of its flags.  No append through an atomic counter anywhere.
//   k_top_count / scan / k_top_place<1>   the survivors (rows whose key, cut to the bytes fixed, is not above the prefix),
//                   in input order: the permutation to order
//   k_top_sort_lds  up to GG_CHUNK_ROWS survivors: one workgroup, keys in LDS (24 KB), each row's rank is the number of
//                   smaller keys (keys are unique, so the ranks are a permutation)
//   k_top_chunk + sort_pairs_by_key   more survivors: stable LSD passes over 24-bit pieces of the key, on the permutation
//                   (24, not 32 bits: the shared radix sort keeps 0xFFFFFFFF for "no element")
//   k_top_gather    (id, walks, lo, hi) through the permutation into the exact-size result columns
// The host enqueues every pass; nothing is read back until the call's one read_back (passes run, ids unknown, survivors, and
// the length of the list if one was written: gg_debug_aggregate_top_listed).
// Every kernel after the decisive pass checks one device word and returns.
// Bytes per pass (model): before compaction N rows x (8 B per key word the pass needs: 8 in the top word, 16 in the
// middle one, 24 with the id; + 8 B with a bias); after it candidates x (4 B list entry + the same, gathered).
#include "gg_internal.h"

using namespace gg;

namespace gg {
namespace {

constexpr int TOP_TILE = 4096;                   // rows per workgroup of the tiled kernels (16 steps of 256)
constexpr uint32_t TOP_CANDIDATE_FLOOR = 65536;  // default: compact at this many candidates or fewer
constexpr uint32_t TOP_LDS_ROWS = GG_CHUNK_ROWS; // survivors one workgroup orders in LDS

// device words of one call
enum TopWord {
  TW_P0 = 0, TW_P1 = 1, TW_P2 = 2,  // the prefix: bytes fixed so far, zero below
  TW_K = 3,       // rank that remains among the candidates (1-based)
  TW_DONE = 4,    // the prefix is decisive
  TW_STATE = 5,   // TopState (below)
  TW_NLIST = 6,   // entries of the list
  TW_CPASS = 7,   // the pass whose k_top_compact writes the list
  TW_LOW = 8,     // lowest byte fixed (24: none)
  TW_PASSES = 9,  // digit passes that ran             (TW_PASSES, TW_BAD, TW_NSURV are read back as one piece)
  TW_BAD = 10,    // group ids that are no vertices of the bias's CSR
  TW_NSURV = 11,  // survivors counted
  TW_WORDS = 12
};

enum TopState : uint64_t {
  TS_ROWS = 0,     // the passes read every row
  TS_COUNTING = 1, // so does the next pass, whose tile counts become the list's places
  TS_LISTED = 2    // the passes read the list (written by k_top_compact of pass TW_CPASS)
};

struct Key {
  uint64_t w2, w1, w0;
};

struct TopCols {  // the level's columns, the gathered bias (null: none) and the order
  const int64_t *id, *walks, *lo, *hi, *brow;
  int by_walks, desc;
};

// NEED: the lowest key word the caller looks at (words below it are left 0 and their columns unread)
template <int NEED>
__device__ __forceinline__ Key top_key(const TopCols &c, uint64_t i) {
  Key k{0, 0, 0};
  if (c.by_walks) {
    if (NEED <= 1) k.w1 = (uint64_t)c.walks[i];
    if (c.desc) k.w1 = ~k.w1;
  } else {
    uint64_t hi = (uint64_t)c.hi[i], lo = 0;
    if (NEED <= 1 || c.brow) lo = (uint64_t)c.lo[i];
    if (c.brow) {  // + the sign-extended bias, mod 2^128
      const int64_t b = c.brow[i];
      const uint64_t s = lo + (uint64_t)b;
      hi += (uint64_t)(b >> 63) + (uint64_t)(s < lo);
      lo = s;
    }
    k.w2 = hi ^ (1ull << 63);
    k.w1 = lo;
    if (c.desc) k.w2 = ~k.w2, k.w1 = ~k.w1;
  }
  if (NEED == 0) k.w0 = (uint64_t)c.id[i] ^ (1ull << 63);
  return k;
}

// the key with the bytes below `low` cleared (low in 0..24; 24 clears everything)
__device__ __forceinline__ Key key_trunc(Key k, int low) {
  const int word = low >> 3;
  const uint64_t m = ~0ull << ((low & 7) * 8);
  if (word == 0) {
    k.w0 &= m;
  } else {
    k.w0 = 0;
    if (word == 1) {
      k.w1 &= m;
    } else {
      k.w1 = 0;
      k.w2 = word == 2 ? (k.w2 & m) : 0;
    }
  }
  return k;
}
__device__ __forceinline__ bool key_eq(const Key &a, const Key &b) { return a.w2 == b.w2 && a.w1 == b.w1 && a.w0 == b.w0; }
__device__ __forceinline__ bool key_less(const Key &a, const Key &b) {
  return a.w2 < b.w2 || (a.w2 == b.w2 && (a.w1 < b.w1 || (a.w1 == b.w1 && a.w0 < b.w0)));
}
__device__ __forceinline__ uint32_t key_byte(const Key &k, int b) {
  const int word = b >> 3;
  const uint64_t w = word == 2 ? k.w2 : word == 1 ? k.w1 : k.w0;
  return (uint32_t)(w >> ((b & 7) * 8)) & 255u;
}
// bits [24 c, 24 c + 24) of the key, c in 0..7
__device__ __forceinline__ uint32_t key_chunk24(const Key &k, int c) {
  const int bit = 24 * c, word = bit >> 6, sh = bit & 63;
  const uint64_t lo = word == 2 ? k.w2 : word == 1 ? k.w1 : k.w0;
  const uint64_t hi = word == 1 ? k.w2 : word == 0 ? k.w1 : 0;
  const uint64_t v = sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
  return (uint32_t)v & 0xFFFFFFu;
}
__device__ __forceinline__ Key top_prefix(const uint64_t *__restrict__ w) { return Key{w[TW_P2], w[TW_P1], w[TW_P0]}; }

// inclusive prefix of v over the workgroup's 256 threads, *total their sum (every thread calls; s_w: 4 words of LDS)
__device__ __forceinline__ uint32_t block_scan_incl(uint32_t v, uint32_t *s_w, uint32_t *total) {
  const uint32_t incl = wave_scan_incl(v);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 63) s_w[wave] = incl;
  __syncthreads();
  uint32_t add = 0, all = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const uint32_t sv = s_w[i];
    if (i < wave) add += sv;
    all += sv;
  }
  __syncthreads();  // (s_w is written again by the next call)
  *total = all;
  return incl + add;
}

__global__ __launch_bounds__(64) void k_top_init(uint64_t *__restrict__ w, uint64_t rank) {
  if (threadIdx.x == 0) w[TW_K] = rank, w[TW_LOW] = 24;
}

// brow[i] = bias of the vertex of row i (dense: its index, INVALID_U32 if the id is no vertex: counted, bias 0)
__global__ __launch_bounds__(256) void k_top_bias(const uint32_t *__restrict__ dense, const int64_t *__restrict__ bias,
                                                  uint64_t N, int64_t *__restrict__ brow,
                                                  unsigned long long *__restrict__ bad) {
  uint32_t mine = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t d = dense[i];
    brow[i] = d != INVALID_U32 ? bias[d] : 0;  // (d < V: a dense index of the CSR the bias has V entries for)
    mine += d == INVALID_U32;
  }
  mine = wave_total_u32(mine);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(bad, (unsigned long long)mine);
}

// One digit pass over byte b (of word W).  hist: this pass's 256 bins, zero before the pass.  tile_count[blockIdx.x] =
// the tile's candidates, while the passes still read every row.
template <int W>
__global__ __launch_bounds__(256) void k_top_hist(TopCols c, uint64_t N, int b, const uint64_t *__restrict__ w,
                                                  const uint32_t *__restrict__ list, uint32_t *__restrict__ hist,
                                                  uint32_t *__restrict__ tile_count) {
  __shared__ uint32_t s_bins[4 * 256];
  __shared__ uint32_t s_cnt[4];
  if (w[TW_DONE]) return;
  const bool listed = w[TW_STATE] == TS_LISTED;
  const uint64_t n = listed ? w[TW_NLIST] : N;  // (n_list <= N: the list has N entries)
  const uint64_t base = (uint64_t)blockIdx.x * TOP_TILE;
  if (base >= n) return;  // (only with a list: the grid covers N rows)
  for (int t = threadIdx.x; t < 4 * 256; t += 256) s_bins[t] = 0;
  __syncthreads();
  const Key p = key_trunc(top_prefix(w), b + 1);
  uint32_t *my_bins = s_bins + (threadIdx.x >> 6) * 256;
  uint32_t mine = 0;
  for (int s = 0; s < TOP_TILE / 256; s++) {
    const uint64_t j = base + (uint64_t)s * 256 + threadIdx.x;
    if (j < n) {
      const uint64_t i = listed ? list[j] : j;  // (a list entry is a row number < N)
      const Key k = top_key<W>(c, i);
      if (key_eq(key_trunc(k, b + 1), p)) {
        atomicAdd(&my_bins[key_byte(k, b)], 1u);
        mine++;
      }
    }
  }
  __syncthreads();
  const uint32_t sum = s_bins[threadIdx.x] + s_bins[256 + threadIdx.x] + s_bins[512 + threadIdx.x] + s_bins[768 + threadIdx.x];
  if (sum) atomicAdd(&hist[threadIdx.x], sum);
  if (!listed) {
    mine = wave_total_u32(mine);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) tile_count[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
  }
}

// One workgroup.  hist: the bins of the pass over byte b.  n_tiles: entries of tile_count.
__global__ __launch_bounds__(256) void k_top_pick(uint64_t *w, const uint32_t *__restrict__ hist, int b, int pass, uint64_t N,
                                                  uint32_t floor, uint32_t *tile_count, uint64_t n_tiles) {
  __shared__ uint32_t s_w[4];
  if (w[TW_DONE]) return;
  const uint64_t state0 = w[TW_STATE], k = w[TW_K];
  const uint32_t h = hist[threadIdx.x];
  uint32_t all;
  const uint32_t incl = block_scan_incl(h, s_w, &all);  // (its barriers stand between the reads above and the writes below)
  const uint32_t excl = incl - h;
  if (h && excl < k && k <= incl) {  // the one bin that holds the rank (the bins sum to the candidates, k is among them)
    const uint64_t below = k - excl;
    w[b >> 3] |= (uint64_t)threadIdx.x << ((b & 7) * 8);  // (TW_P0..TW_P2 are words 0..2)
    w[TW_K] = below;
    w[TW_LOW] = (uint64_t)b;
    w[TW_PASSES] += 1;
    if (below == h)
      w[TW_DONE] = 1;  // every candidate left is in
    else if (state0 == TS_ROWS && h <= floor && 2 * (uint64_t)h <= N)
      w[TW_STATE] = TS_COUNTING;
  }
  if (state0 == TS_COUNTING) {  // this pass counted its candidates per tile: their exclusive prefix, in place
    uint32_t run = 0;
    for (uint64_t at = 0; at < n_tiles; at += 256) {
      const uint64_t i = at + threadIdx.x;
      const uint32_t v = i < n_tiles ? tile_count[i] : 0;
      uint32_t tot;
      const uint32_t in = block_scan_incl(v, s_w, &tot);
      if (i < n_tiles) tile_count[i] = run + in - v;
      run += tot;
    }
    if (threadIdx.x == 0) w[TW_NLIST] = run, w[TW_CPASS] = (uint64_t)pass, w[TW_STATE] = TS_LISTED;
  }
}

// the flag of row j: MODE 0 a candidate of the pass over byte b (matches the prefix above it), MODE 1 a survivor
template <int MODE>
__device__ __forceinline__ bool top_flag(const TopCols &c, uint64_t j, const Key &p, int low) {
  const Key k = key_trunc(top_key<0>(c, j), low);
  return MODE == 0 ? key_eq(k, p) : !key_less(p, k);
}

// tile_count[t] = the survivors of tile t
__global__ __launch_bounds__(256) void k_top_count(TopCols c, uint64_t N, const uint64_t *__restrict__ w,
                                                   uint32_t *__restrict__ tile_count) {
  __shared__ uint32_t s_cnt[4];
  const int low = (int)w[TW_LOW];
  const Key p = key_trunc(top_prefix(w), low);
  const uint64_t base = (uint64_t)blockIdx.x * TOP_TILE;
  uint32_t mine = 0;
  for (int s = 0; s < TOP_TILE / 256; s++) {
    const uint64_t j = base + (uint64_t)s * 256 + threadIdx.x;
    if (j < N) mine += top_flag<1>(c, j, p, low);
  }
  mine = wave_total_u32(mine);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0) tile_count[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// tile_base: the exclusive prefix of the tile counts.  out[place] = row number, in input order; cap: entries of out.
template <int MODE>
__global__ __launch_bounds__(256) void k_top_place(TopCols c, uint64_t N, int b, int pass, const uint64_t *__restrict__ w,
                                                   const uint32_t *__restrict__ tile_base, uint32_t *__restrict__ out,
                                                   uint64_t cap, unsigned long long *__restrict__ listed) {
  __shared__ uint32_t s_w[4];
  if (MODE == 0 && (w[TW_DONE] || w[TW_STATE] != TS_LISTED || w[TW_CPASS] != (uint64_t)pass)) return;
  if (MODE == 0 && blockIdx.x == 0 && threadIdx.x == 0) *listed = w[TW_NLIST];  // (diagnostics: a list was written)
  const int low = MODE == 0 ? b + 1 : (int)w[TW_LOW];
  const Key p = key_trunc(top_prefix(w), low);
  const uint64_t base = (uint64_t)blockIdx.x * TOP_TILE;
  uint64_t run = tile_base[blockIdx.x];
  for (int s = 0; s < TOP_TILE / 256; s++) {  // (the bound is uniform: every thread reaches the scan's barriers)
    const uint64_t j = base + (uint64_t)s * 256 + threadIdx.x;
    const bool f = j < N && top_flag<MODE>(c, j, p, low);
    uint32_t tot;
    const uint32_t incl = block_scan_incl(f ? 1u : 0u, s_w, &tot);
    const uint64_t at = run + incl - 1;
    if (f && at < cap) out[at] = (uint32_t)j;
    run += tot;
  }
}

__global__ __launch_bounds__(256) void k_top_iota(uint32_t *__restrict__ out, uint64_t n) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    out[i] = (uint32_t)i;
}

// m <= TOP_LDS_ROWS survivors (perm_in: their row numbers): perm_out[rank] = row number
__global__ __launch_bounds__(256) void k_top_sort_lds(TopCols c, const uint32_t *__restrict__ perm_in, uint32_t m,
                                                      uint32_t *__restrict__ perm_out) {
  __shared__ uint64_t s2[TOP_LDS_ROWS], s1[TOP_LDS_ROWS], s0[TOP_LDS_ROWS];
  constexpr int PER = TOP_LDS_ROWS / 256;
  Key mine[PER];
  uint32_t row[PER], rank[PER];
#pragma unroll
  for (int e = 0; e < PER; e++) {
    const uint32_t j = threadIdx.x + e * 256;
    mine[e] = Key{0, 0, 0};
    row[e] = 0, rank[e] = 0;
    if (j < m) {
      row[e] = perm_in[j];
      mine[e] = top_key<0>(c, row[e]);
      s2[j] = mine[e].w2, s1[j] = mine[e].w1, s0[j] = mine[e].w0;
    }
  }
  __syncthreads();
  for (uint32_t j = 0; j < m; j++) {  // (every lane reads the same address: a broadcast)
    const Key kj{s2[j], s1[j], s0[j]};
#pragma unroll
    for (int e = 0; e < PER; e++) rank[e] += key_less(kj, mine[e]);
  }
#pragma unroll
  for (int e = 0; e < PER; e++)
    if (threadIdx.x + e * 256 < m && rank[e] < m) perm_out[rank[e]] = row[e];
}

// piece[j] = 24-bit piece `chunk` of the key of row perm[j]
__global__ __launch_bounds__(256) void k_top_chunk(TopCols c, const uint32_t *__restrict__ perm, uint64_t m, int chunk,
                                                   uint32_t *__restrict__ piece) {
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (uint64_t)gridDim.x * blockDim.x)
    piece[j] = key_chunk24(top_key<0>(c, perm[j]), chunk);
}

__global__ __launch_bounds__(256) void k_top_gather(TopCols c, const uint32_t *__restrict__ perm, uint64_t m,
                                                    int64_t *__restrict__ out_id, int64_t *__restrict__ out_walks,
                                                    int64_t *__restrict__ out_lo, int64_t *__restrict__ out_hi) {
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t i = perm[j];  // (a row number < N)
    out_id[j] = c.id[i];
    out_walks[j] = c.walks[i];
    out_lo[j] = c.lo[i];
    out_hi[j] = c.hi[i];
  }
}

int top_hist_launch(gg_ctx *ctx, unsigned tiles, const TopCols &c, uint64_t N, int b, const uint64_t *w, const uint32_t *list,
                    uint32_t *hist, uint32_t *tile_count) {
  switch (b >> 3) {
  case 2:
    GG_LAUNCH(ctx, "top_hist", (k_top_hist<2>), dim3(tiles), dim3(256), 0, c, N, b, w, list, hist, tile_count);
    break;
  case 1:
    GG_LAUNCH(ctx, "top_hist", (k_top_hist<1>), dim3(tiles), dim3(256), 0, c, N, b, w, list, hist, tile_count);
    break;
  default:
    GG_LAUNCH(ctx, "top_hist", (k_top_hist<0>), dim3(tiles), dim3(256), 0, c, N, b, w, list, hist, tile_count);
  }
  return GG_OK;
}

}  // namespace
}  // namespace gg

extern "C" int gg_khop_aggregate_top(gg_ctx *ctx, const gg_result *agg, int hops, int order_by, int descending, uint64_t n,
                                     const gg_csr *csr_c, const int64_t *bias, gg_top_stats *stats,
                                     gg_result **out_result) {
  if (out_result) *out_result = nullptr;
  if (stats) memset(stats, 0, sizeof(*stats));
  if (!ctx || !agg || !out_result || agg->ctx != ctx || (csr_c && csr_c->ctx != ctx)) {
    set_error("gg_khop_aggregate_top: bad context / result / csr / out_result argument");
    return GG_ERR_INVALID_ARG;
  }
  GG_TRY(expect_kind(agg, ResultKind::AGGREGATE, "gg_khop_aggregate_top"));
  if (hops < agg->k_min || hops > agg->k_max) {
    set_error("gg_khop_aggregate_top: level %d outside the result's %d..%d", hops, agg->k_min, agg->k_max);
    return GG_ERR_INVALID_ARG;
  }
  if (order_by != GG_TOP_BY_TOTAL && order_by != GG_TOP_BY_WALKS) {
    set_error("gg_khop_aggregate_top: order_by %d (0: the total, 1: the walks)", order_by);
    return GG_ERR_INVALID_ARG;
  }
  if (bias && (!csr_c || order_by == GG_TOP_BY_WALKS)) {
    set_error("gg_khop_aggregate_top: a bias needs the csr of its vertices and is added to the total only");
    return GG_ERR_INVALID_ARG;
  }
  if (csr_c && csr_c->n_parts > 1) {
    set_error("gg_khop_aggregate_top needs a whole CSR, not a shard (gg_csr_build_shard)");
    return GG_ERR_STATE;
  }
  ApiScope scope(ctx);
  GG_HIP(hipSetDevice(ctx->device));
  const uint64_t N = agg->rows[hops], m = n < N ? n : N;
  ResultOwner res = make_result(ctx, ResultKind::AGGREGATE, hops, hops);
  res->rows[hops] = m;
  if (stats) stats->rows_in = N, stats->rows_out = m;
  if (m == 0) {
    *out_result = res.release();
    return GG_OK;
  }
  hipStream_t st = ctx->stream;
  const bool by_walks = order_by == GG_TOP_BY_WALKS;
  uint64_t *w = nullptr;
  GG_TRY(ctx->dev_alloc((void **)&w, TW_WORDS * sizeof(uint64_t)));
  GG_HIP(hipMemsetAsync(w, 0, TW_WORDS * sizeof(uint64_t), st));
  unsigned long long *listed = nullptr;  // entries of the list the selection compacted its candidates to (0: it did not)
  GG_TRY(ctx->dev_alloc((void **)&listed, sizeof(unsigned long long)));
  GG_HIP(hipMemsetAsync(listed, 0, sizeof(unsigned long long), st));

  TopCols c{agg->cols[hops][0], agg->cols[hops][1], agg->cols[hops][2], agg->cols[hops][3], nullptr, (int)by_walks,
            descending != 0};
  if (bias) {
    gg_csr *csr = const_cast<gg_csr *>(csr_c);
    uint32_t *dense = nullptr;
    int64_t *bias_dev = nullptr, *brow = nullptr;
    GG_TRY(ctx->dev_alloc((void **)&dense, N * sizeof(uint32_t)));
    GG_TRY(ctx->dev_alloc((void **)&bias_dev, (csr->V ? csr->V : 1) * sizeof(int64_t)));
    GG_TRY(ctx->dev_alloc((void **)&brow, N * sizeof(int64_t)));
    GG_TRY(lookup_ids(ctx, csr, c.id, N, dense));
    // (caller memory: the read_back below synchronises the stream before this call returns)
    if (csr->V) GG_HIP(hipMemcpyAsync(bias_dev, bias, csr->V * sizeof(int64_t), hipMemcpyHostToDevice, st));
    GG_LAUNCH(ctx, "top_bias", k_top_bias, stride_grid(ctx, N), dim3(256), 0, (const uint32_t *)dense,
              (const int64_t *)bias_dev, N, brow, (unsigned long long *)(w + TW_BAD));
    c.brow = brow;
  }

  const uint64_t n_tiles = (N + TOP_TILE - 1) / TOP_TILE;
  const unsigned tiles = (unsigned)n_tiles;
  uint32_t *perm = nullptr;  // the survivors' row numbers in input order
  GG_TRY(ctx->dev_alloc((void **)&perm, m * sizeof(uint32_t)));
  if (m < N) {
    const int n_pass = by_walks ? 16 : 24;  // (walks: the top word of every key is 0)
    const uint32_t floor = ctx->agg_top_floor ? ctx->agg_top_floor : TOP_CANDIDATE_FLOOR;
    uint32_t *hist = nullptr, *tile_count = nullptr, *list = nullptr;
    GG_TRY(ctx->dev_alloc((void **)&hist, (size_t)n_pass * 256 * sizeof(uint32_t)));
    GG_TRY(ctx->dev_alloc((void **)&tile_count, n_tiles * sizeof(uint32_t)));
    GG_TRY(ctx->dev_alloc((void **)&list, N * sizeof(uint32_t)));
    GG_HIP(hipMemsetAsync(hist, 0, (size_t)n_pass * 256 * sizeof(uint32_t), st));
    GG_LAUNCH(ctx, "top_init", k_top_init, dim3(1), dim3(64), 0, w, m);
    for (int pass = 0; pass < n_pass; pass++) {
      const int b = n_pass - 1 - pass;
      GG_TRY(top_hist_launch(ctx, tiles, c, N, b, w, list, hist + pass * 256, tile_count));
      GG_LAUNCH(ctx, "top_pick", k_top_pick, dim3(1), dim3(256), 0, w, (const uint32_t *)(hist + pass * 256), b, pass, N,
                floor, tile_count, n_tiles);
      GG_LAUNCH(ctx, "top_compact", (k_top_place<0>), dim3(tiles), dim3(256), 0, c, N, b, pass, (const uint64_t *)w,
                (const uint32_t *)tile_count, list, N, listed);
    }
    GG_LAUNCH(ctx, "top_count", k_top_count, dim3(tiles), dim3(256), 0, c, N, (const uint64_t *)w, tile_count);
    GG_TRY(scan_exclusive_u32(ctx, tile_count, tile_count, n_tiles, w + TW_NSURV));
    GG_LAUNCH(ctx, "top_place", (k_top_place<1>), dim3(tiles), dim3(256), 0, c, N, 0, 0, (const uint64_t *)w,
              (const uint32_t *)tile_count, perm, m, listed);
  } else {
    GG_LAUNCH(ctx, "top_iota", k_top_iota, stride_grid(ctx, m), dim3(256), 0, perm, m);
  }

  // order the survivors
  int route = 0;
  const uint32_t *ordered = perm;
  if (m > 1) {
    route = (ctx->agg_top_route != 2 && m <= TOP_LDS_ROWS) ? 1 : 2;
    if (route == 1) {
      uint32_t *out = nullptr;
      GG_TRY(ctx->dev_alloc((void **)&out, m * sizeof(uint32_t)));
      GG_LAUNCH(ctx, "top_sort_lds", k_top_sort_lds, dim3(1), dim3(256), 0, c, (const uint32_t *)perm, (uint32_t)m, out);
      ordered = out;
    } else {
      uint32_t *piece = nullptr, *piece_out = nullptr, *other = nullptr;
      GG_TRY(ctx->dev_alloc((void **)&piece, m * sizeof(uint32_t)));
      GG_TRY(ctx->dev_alloc((void **)&piece_out, m * sizeof(uint32_t)));
      GG_TRY(ctx->dev_alloc((void **)&other, m * sizeof(uint32_t)));
      uint32_t *cur = perm, *nxt = other;
      const int chunks = by_walks ? 6 : 8;  // 24-bit pieces, least significant first
      for (int ch = 0; ch < chunks; ch++) {
        GG_LAUNCH(ctx, "top_chunk", k_top_chunk, stride_grid(ctx, m), dim3(256), 0, c, (const uint32_t *)cur, m, ch, piece);
        GG_TRY(sort_pairs_by_key(ctx, piece, cur, m, 24, piece_out, nxt));
        uint32_t *t = cur;
        cur = nxt, nxt = t;
      }
      ordered = cur;
    }
  }
  for (int col = 0; col < 4; col++) {
    GG_TRY(ctx->dev_alloc((void **)&res->cols[hops][col], m * sizeof(int64_t)));
    ctx->keep(res->cols[hops][col]);
  }
  GG_LAUNCH(ctx, "top_gather", k_top_gather, stride_grid(ctx, m), dim3(256), 0, c, ordered, m, res->cols[hops][0],
            res->cols[hops][1], res->cols[hops][2], res->cols[hops][3]);

  uint64_t hw[3], n_listed = 0;  // passes run, ids unknown, survivors; the compaction's list
  GG_TRY(read_back(ctx, {{w + TW_PASSES, sizeof(hw), hw}, {listed, sizeof(n_listed), &n_listed}}));
  ctx->agg_top_listed = n_listed;
  if (hw[1]) {
    set_error("gg_khop_aggregate_top: %llu groups hold an id that is no vertex of the csr", (unsigned long long)hw[1]);
    return GG_ERR_STATE;
  }
  if (m < N && hw[2] != m) {
    set_error("internal: gg_khop_aggregate_top selected %llu rows, not %llu", (unsigned long long)hw[2],
              (unsigned long long)m);
    return GG_ERR_STATE;
  }
  if (stats) stats->select_passes = (uint32_t)hw[0], stats->sort_route = (uint32_t)route;
  *out_result = res.release();
  return GG_OK;
}

extern "C" int gg_debug_aggregate_top_listed(gg_ctx *ctx, uint64_t *list_entries) {
  if (!ctx || !list_entries) return GG_ERR_INVALID_ARG;
  *list_entries = ctx->agg_top_listed;
  return GG_OK;
}

extern "C" int gg_debug_aggregate_top(gg_ctx *ctx, int sort_route, uint32_t candidate_floor) {
  if (!ctx || sort_route < 0 || sort_route > 2) return GG_ERR_INVALID_ARG;
  ctx->agg_top_route = sort_route;
  ctx->agg_top_floor = candidate_floor;
  return GG_OK;
}
