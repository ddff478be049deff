// gg_top.h — the selection and ordering passes of a device top-n, shared by gg_aggregate_top.hip (the best groups of an
// aggregate) and gg_value.hip (the best rows of a walk table).  Not part of the C-ABI.
//
// Every row has one 192-bit unsigned key in which smaller is better, three words (w2, w1, w0), never stored.  Where the
// words come from is the business of a key source Src, a struct of device pointers passed by value with two members:
//   template <int NEED> Key key(uint64_t i)   the key of row i; NEED is the lowest word the caller looks at (words below it
//                                             may be left 0 and their columns unread)
//   bool live(uint64_t i)                     whether row i takes part at all (a row that is not live is never a candidate)
// Keys of live rows must be unique: then the n-th smallest exists and exactly n rows are not above it.
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
//   k_top_count / scan / k_top_place<1>   the survivors (live rows whose key, cut to the bytes fixed, is not above the
//                   prefix), in input order: the permutation to order
//   k_top_sort_lds  up to GG_CHUNK_ROWS survivors: one workgroup, keys in LDS (24 KB), each row's rank is the number of
//                   smaller keys (keys are unique, so the ranks are a permutation)
//   k_top_chunk + sort_pairs_by_key   more survivors: stable LSD passes over 24-bit pieces of the key, on the permutation
//                   (24, not 32 bits: the shared radix sort keeps 0xFFFFFFFF for "no element")
// A caller that knows the number of survivors only on the device (gg_value.hip: min(n, candidates)) hands the kernels that
// word (m_dev) next to the host's upper bound; the aggregate passes NULL and its bound is exact.
// Every kernel after the decisive pass checks one device word and returns.
#pragma once
#include "gg_internal.h"

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

// the rank to select: `rank`, or min(rank, *limit) where the number of live rows is a device word; nothing to select
// (rank 0) is decided at once, and then no live row survives
__global__ __launch_bounds__(64) void k_top_init(uint64_t *__restrict__ w, uint64_t rank, const uint64_t *__restrict__ limit) {
  if (threadIdx.x == 0) {
    if (limit && *limit < rank) rank = *limit;
    w[TW_K] = rank, w[TW_LOW] = 24;
    if (rank == 0) w[TW_DONE] = 1;
  }
}

// One digit pass over byte b (of word W).  hist: this pass's 256 bins, zero before the pass.  tile_count[blockIdx.x] =
// the tile's candidates, while the passes still read every row.
template <typename Src, int W>
__global__ __launch_bounds__(256) void k_top_hist(Src c, uint64_t N, int b, const uint64_t *__restrict__ w,
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
      const uint64_t i = listed ? list[j] : j;  // (a list entry is the row number < N of a live row)
      if (listed || c.live(i)) {
        const Key k = c.template key<W>(i);
        if (key_eq(key_trunc(k, b + 1), p)) {
          atomicAdd(&my_bins[key_byte(k, b)], 1u);
          mine++;
        }
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
template <int MODE, typename Src>
__device__ __forceinline__ bool top_flag(const Src &c, uint64_t j, const Key &p, int low) {
  if (!c.live(j)) return false;
  const Key k = key_trunc(c.template key<0>(j), low);
  return MODE == 0 ? key_eq(k, p) : !key_less(p, k);
}

// tile_count[t] = the survivors of tile t
template <typename Src>
__global__ __launch_bounds__(256) void k_top_count(Src c, uint64_t N, const uint64_t *__restrict__ w,
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
template <int MODE, typename Src>
__global__ __launch_bounds__(256) void k_top_place(Src c, uint64_t N, int b, int pass, const uint64_t *__restrict__ w,
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

// min(m, *m_dev) <= TOP_LDS_ROWS survivors (perm_in: their row numbers; m_dev null: m of them): perm_out[rank] = row number
template <typename Src>
__global__ __launch_bounds__(256) void k_top_sort_lds(Src c, const uint32_t *__restrict__ perm_in, uint32_t m,
                                                      const uint64_t *__restrict__ m_dev, uint32_t *__restrict__ perm_out) {
  __shared__ uint64_t s2[TOP_LDS_ROWS], s1[TOP_LDS_ROWS], s0[TOP_LDS_ROWS];
  constexpr int PER = TOP_LDS_ROWS / 256;
  if (m_dev && *m_dev < m) m = (uint32_t)*m_dev;
  Key mine[PER];
  uint32_t row[PER], rank[PER];
#pragma unroll
  for (int e = 0; e < PER; e++) {
    const uint32_t j = threadIdx.x + e * 256;
    mine[e] = Key{0, 0, 0};
    row[e] = 0, rank[e] = 0;
    if (j < m) {
      row[e] = perm_in[j];
      mine[e] = c.template key<0>(row[e]);
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

// piece[j] = 24-bit piece `chunk` of the key of row perm[j]; past *m_dev (m_dev null: nowhere) "no element" to the sort
template <typename Src>
__global__ __launch_bounds__(256) void k_top_chunk(Src c, const uint32_t *__restrict__ perm, uint64_t m,
                                                   const uint64_t *__restrict__ m_dev, int chunk,
                                                   uint32_t *__restrict__ piece) {
  const uint64_t have = m_dev && *m_dev < m ? *m_dev : m;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (uint64_t)gridDim.x * blockDim.x)
    piece[j] = j < have ? key_chunk24(c.template key<0>(perm[j]), chunk) : INVALID_U32;
}

template <typename Src>
int top_hist_launch(gg_ctx *ctx, unsigned tiles, const Src &c, uint64_t N, int b, const uint64_t *w, const uint32_t *list,
                    uint32_t *hist, uint32_t *tile_count) {
  switch (b >> 3) {
  case 2:
    GG_LAUNCH(ctx, "top_hist", (k_top_hist<Src, 2>), dim3(tiles), dim3(256), 0, c, N, b, w, list, hist, tile_count);
    break;
  case 1:
    GG_LAUNCH(ctx, "top_hist", (k_top_hist<Src, 1>), dim3(tiles), dim3(256), 0, c, N, b, w, list, hist, tile_count);
    break;
  default:
    GG_LAUNCH(ctx, "top_hist", (k_top_hist<Src, 0>), dim3(tiles), dim3(256), 0, c, N, b, w, list, hist, tile_count);
  }
  return GG_OK;
}

// What a caller's keys need of the passes: the key bytes to select over, most significant first (bytes that are zero in
// every key are left out: their prefix byte stays zero), and the 24-bit pieces to sort by, least significant first.
struct TopPlan {
  int n_bytes = 0, bytes[24];
  int n_chunks = 0, chunks[8];
};

// Selects the `rank` best live rows of the N (rank, or min(rank, *limit) if limit is a device word) and orders them:
// *ordered (from the pool) holds their row numbers in rank order, w[TW_NSURV] their number, w[TW_PASSES] the digit passes
// that ran.  rank >= 1, N < 2^32.  route_forced / floor: the caller's testing knob.  Nothing is read back.
template <typename Src>
int top_select_order(gg_ctx *ctx, const Src &c, uint64_t N, uint64_t rank, const uint64_t *limit, const TopPlan &plan,
                     int route_forced, uint32_t floor, uint64_t *w, unsigned long long *listed, const uint32_t **ordered,
                     int *route_out) {
  hipStream_t st = ctx->stream;
  const uint64_t n_tiles = (N + TOP_TILE - 1) / TOP_TILE;
  const unsigned tiles = (unsigned)n_tiles;
  const uint64_t *m_dev = limit ? w + TW_NSURV : nullptr;
  uint32_t *perm = nullptr;  // the survivors' row numbers in input order
  GG_TRY(ctx->dev_alloc((void **)&perm, rank * sizeof(uint32_t)));
  if (rank < N || limit) {
    const int n_pass = plan.n_bytes;
    if (!floor) floor = TOP_CANDIDATE_FLOOR;
    uint32_t *hist = nullptr, *tile_count = nullptr, *list = nullptr;
    GG_TRY(ctx->dev_alloc((void **)&hist, (size_t)n_pass * 256 * sizeof(uint32_t)));
    GG_TRY(ctx->dev_alloc((void **)&tile_count, n_tiles * sizeof(uint32_t)));
    GG_TRY(ctx->dev_alloc((void **)&list, N * sizeof(uint32_t)));
    GG_HIP(hipMemsetAsync(hist, 0, (size_t)n_pass * 256 * sizeof(uint32_t), st));
    GG_LAUNCH(ctx, "top_init", k_top_init, dim3(1), dim3(64), 0, w, rank, limit);
    for (int pass = 0; pass < n_pass; pass++) {
      const int b = plan.bytes[pass];
      GG_TRY(top_hist_launch(ctx, tiles, c, N, b, w, list, hist + pass * 256, tile_count));
      GG_LAUNCH(ctx, "top_pick", k_top_pick, dim3(1), dim3(256), 0, w, (const uint32_t *)(hist + pass * 256), b, pass, N,
                floor, tile_count, n_tiles);
      GG_LAUNCH(ctx, "top_compact", (k_top_place<0, Src>), dim3(tiles), dim3(256), 0, c, N, b, pass, (const uint64_t *)w,
                (const uint32_t *)tile_count, list, N, listed);
    }
    GG_LAUNCH(ctx, "top_count", (k_top_count<Src>), dim3(tiles), dim3(256), 0, c, N, (const uint64_t *)w, tile_count);
    GG_TRY(scan_exclusive_u32(ctx, tile_count, tile_count, n_tiles, w + TW_NSURV));
    GG_LAUNCH(ctx, "top_place", (k_top_place<1, Src>), dim3(tiles), dim3(256), 0, c, N, 0, 0, (const uint64_t *)w,
              (const uint32_t *)tile_count, perm, rank, listed);
  } else {
    GG_LAUNCH(ctx, "top_iota", k_top_iota, stride_grid(ctx, rank), dim3(256), 0, perm, rank);
  }

  // order the survivors
  int route = 0;
  *ordered = perm;
  if (rank > 1) {
    route = (route_forced != 2 && rank <= TOP_LDS_ROWS) ? 1 : 2;
    if (route == 1) {
      uint32_t *out = nullptr;
      GG_TRY(ctx->dev_alloc((void **)&out, rank * sizeof(uint32_t)));
      GG_LAUNCH(ctx, "top_sort_lds", (k_top_sort_lds<Src>), dim3(1), dim3(256), 0, c, (const uint32_t *)perm, (uint32_t)rank,
                m_dev, out);
      *ordered = out;
    } else {
      uint32_t *piece = nullptr, *piece_out = nullptr, *other = nullptr;
      GG_TRY(ctx->dev_alloc((void **)&piece, rank * sizeof(uint32_t)));
      GG_TRY(ctx->dev_alloc((void **)&piece_out, rank * sizeof(uint32_t)));
      GG_TRY(ctx->dev_alloc((void **)&other, rank * sizeof(uint32_t)));
      uint32_t *cur = perm, *nxt = other;
      for (int ci = 0; ci < plan.n_chunks; ci++) {
        GG_LAUNCH(ctx, "top_chunk", (k_top_chunk<Src>), stride_grid(ctx, rank), dim3(256), 0, c, (const uint32_t *)cur, rank,
                  m_dev, plan.chunks[ci], piece);
        GG_TRY(sort_pairs_by_key(ctx, piece, cur, rank, 24, piece_out, nxt));
        uint32_t *t = cur;
        cur = nxt, nxt = t;
      }
      *ordered = cur;
    }
  }
  *route_out = route;
  return GG_OK;
}

}  // namespace
}  // namespace gg
