// gg_cheapest.hip — the cheapest walks over weighted edge rows from 64 sources a pass: one row (source, vertex, cost, hops).
//
// The reference answers cheapest_path_length / ANY SHORTEST ... COST, and a hand-written statement answers it with a
// recursive CTE under min(cost): one hash join of the working table with the edge table per round
// (PhysicalRecursiveCTE::GetData, src/execution/operator/set/physical_recursive_cte.cpp, above JoinHashTable::Probe,
// src/execution/join_hashtable.cpp:304-476) and a two-key hash aggregate over every walk row it formed
// (src/execution/operator/aggregate/physical_hash_aggregate.cpp:152-266).  The answer is a min-plus matrix product run to a
// fixpoint.  With cost_0 = 0 at the lane's source and nothing elsewhere,
//     cost_r(x) = min(cost_{r-1}(x), min over the entries u -> x of x's reverse row of cost_{r-1}(u) (+) w(entry))
// (+) adding with saturation at INT64_MAX.  One wavefront lane carries one source (gg_pairs.hip's organisation).
//   cost[v * 64 + lane]    u64, ~0 = unreached; read and written in place by the one wavefront that owns v
//   fresh[2][v * 64 + lane] the values lowered in the last round, swapped per round; a cell is only read where its mask bit
//                          is set, so neither buffer is ever cleared
//   mask[2][v]             the lanes of v lowered in the last round; written for every vertex by every round
//   hops[v * 64 + lane]    u32, the round that wrote cost; read only where cost is not ~0
//   reach[v]               the lanes of v that have a cost (what the row placement walks)
// A neighbour is read through `fresh`, and only where its mask bit is set: a cell that did not change in round r - 1 had
// its candidate considered in round r - 1 already.  That is what makes the rounds exact Jacobi rounds over ONE cost array:
// nobody but the owner reads cost, and fresh[cur] is not written while it is read.
//   k_cp_permute     the caller's weights into reverse-entry order (rnbr_by_src's, through rpos_by_src); one reduction
//                    says whether a rowid fell outside the column or a weight is negative
//   k_cp_seed        cost = fresh0 = hops = 0 at (source, lane); the only atomics on state words (mask, reach; none on cost)
//   k_cp_long_flag / scan / k_cp_long_list   the in-rows longer than the threshold, once per call — a private copy of
//                    gg_pairs.hip's three steps: sharing them would have changed that file's launches
//   k_cp_pull        one wavefront per vertex of up to `threshold` in-entries: 64 entries, their masks and their weights
//                    a lane each, the entries with a mask taken four at a time (four independent 512-byte gathers in
//                    flight), best = min(best, fresh[u] (+) w); lowered = ballot(best < own), the stores gated by it.
//                    The own row is read only if some lane found a candidate
//   k_cp_pull_long   one workgroup of 256 per listed row, four partial minima folded through LDS; min commutes: same bits
//   k_cp_targets / k_cp_count / scan / k_cp_write   gg_pairs.hip's placement with a cost and a hops column
// Bytes per round (model): E * (4 B entry + 8 B mask + 8 B weight of a live chunk) + rows_gathered * 512 B + V * (8 B
// offsets + 8 B mask) + per vertex with a candidate 512 B of cost read + per lowered row 2 x 512 B + 256 B written.
//
// The cheapest paths themselves (gg_cheapest64_paths; the relation is pinned in include/gg.h): the batch runs to its
// fixpoint (cp_solve, the rounds above with no bound), then each pair is read backwards off cost and hops while they are
// still on the device.  For a vertex x of lane s with hops h >= 1 and cost c < INT64_MAX, pred(s, x) is the first entry
// u -> x of x's reverse row by source (rnbr_by_src: ascending (source, forward position)) with cost(s, u) (+) w(entry) == c
// and hops(s, u) == h - 1; the entry is the step's edge, its rowid found through rpos_by_src.  h falls by one per step, so
// a zero-weight cycle cannot hold a walk.
//   k_cpp_len      per pair hops + 1 (0: unreached, not a vertex, or saturated) and whether the pair has a cost at all
//   k_cpp_pairs    the pair table (pair index, cost, hops, traced) of the reached pairs, placed by a scan of those flags
//   k_cpp_trace    GG_CPP_LANES lanes per pair walk from t back to s (gg_paths.hip's organisation, with one phase only):
//                  per trip a chunk of the reverse row — entry and weight coalesced, the cost cell of each entry gathered,
//                  the hops cell only where the cost matched (a hops cell is defined only where the cost cell is not ~0)
// Bytes per step (model, not traffic): entries looked at x (4 B entry + 8 B weight + one 64-byte line of cost, plus one of
// hops where it was read) + 4 B rpos + 8 B rowid + 36 B of result row.  The serial depth of a pair is its hops.
#include "gg_internal.h"

#ifndef GG_CPP_LANES
#define GG_CPP_LANES 16  // lanes per pair in k_cpp_trace.  Inherited from the BFS trace (GG_PATH_LANES) and then measured for this
                         // kernel: 64 sources, weights hash(rowid) in 1..100, cpp_trace per batch, every vertex as target —
                         // SF10 (4.2 M pairs, 32 M rows) 8 lanes 50.7 ms, 16: 48.7 / 48.5, 64: 50.4; SF100 (28.7 M pairs,
                         // 244 M rows) 8: 810.2, 16: 772.0 / 771.1, 64: 821.5; 10^4 sampled targets SF100 8: 21.08, 16: 18.83,
                         // 64: 18.91 (profiles/r23_cheapest_paths_*_l{8,16,64}.json; two 16-lane runs differ by <= 0.4 %)
#endif

using namespace gg;

struct gg_edge_weights {
  gg_ctx *ctx = nullptr;
  const gg_csr *csr = nullptr;
  uint64_t E = 0;
  uint64_t *w = nullptr;  // E weights in the order of csr->rnbr_by_src, device
};

namespace gg {
namespace {

constexpr uint32_t CP_LONG_ROW = 512;  // default: rows of more entries go to a whole workgroup
constexpr int CP_LANES = GG_BFS_LANES;
static_assert(CP_LANES == 64, "one wavefront lane per source");
constexpr uint64_t CP_NONE = ~0ull;                 // unreached
constexpr uint64_t CP_MAX = (uint64_t)INT64_MAX;    // costs saturate here

// c <= CP_MAX and w <= CP_MAX: the sum cannot wrap
__device__ __forceinline__ uint64_t cp_add(uint64_t c, uint64_t w) {
  const uint64_t s = c + w;
  return s > CP_MAX ? CP_MAX : s;
}
__device__ __forceinline__ uint64_t cp_min(uint64_t a, uint64_t b) { return a < b ? a : b; }

__device__ __forceinline__ uint64_t cp_readlane_u64(uint64_t x, int j) {  // j wave-uniform
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, j);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), j);
  return ((uint64_t)hi << 32) | lo;
}

// flags[0] != 0: a kept edge's rowid lies outside [0, n_weights); flags[1] != 0: a weight that is read is negative
__global__ __launch_bounds__(256) void k_cp_permute(const uint32_t *__restrict__ rpos, const int64_t *__restrict__ eid,
                                                    const uint32_t *__restrict__ epos, const int64_t *__restrict__ weights,
                                                    uint64_t n_weights, int by_entry, uint64_t E,
                                                    uint64_t *__restrict__ wrev, unsigned long long *__restrict__ flags) {
  bool outside = false, negative = false;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < E; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t p = rpos[i];  // (p < E)
    const int64_t r = by_entry ? (int64_t)p : (eid ? eid[p] : (int64_t)epos[p]);
    int64_t w = 0;
    if (r < 0 || (uint64_t)r >= n_weights)
      outside = true;
    else
      w = weights[r];
    if (w < 0) negative = true;
    wrev[i] = (uint64_t)w;
  }
  const uint64_t o = __ballot(outside), n = __ballot(negative);
  if ((threadIdx.x & 63) == 0) {
    if (o) atomicOr(&flags[0], 1ull);
    if (n) atomicOr(&flags[1], 1ull);
  }
}

__global__ __launch_bounds__(64) void k_cp_seed(const uint32_t *__restrict__ dense, int n_src, uint64_t *__restrict__ cost,
                                                uint64_t *__restrict__ fresh, uint32_t *__restrict__ hops,
                                                unsigned long long *__restrict__ mask, unsigned long long *__restrict__ reach,
                                                unsigned long long *__restrict__ reached_total) {
  const int i = threadIdx.x;
  const bool ok = i < n_src && dense[i] != INVALID_U32;
  if (ok) {  // (dense[i] < V: the cell arrays have 64 V entries, mask and reach V)
    const uint64_t c = (uint64_t)dense[i] * CP_LANES + i;
    cost[c] = 0;
    fresh[c] = 0;
    hops[c] = 0;
    atomicOr(&mask[dense[i]], 1ull << i);
    atomicOr(&reach[dense[i]], 1ull << i);
  }
  const uint64_t seeded = __ballot(ok);
  if (i == 0) *reached_total = (unsigned long long)__popcll(seeded);
}

__global__ __launch_bounds__(256) void k_cp_long_flag(const uint32_t *__restrict__ off, uint64_t V, uint32_t threshold,
                                                      uint32_t *__restrict__ flag) {
  for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (uint64_t)gridDim.x * blockDim.x)
    flag[v] = off[v + 1] - off[v] > threshold ? 1u : 0u;
}

// pos: the exclusive prefix of the flags
__global__ __launch_bounds__(256) void k_cp_long_list(const uint32_t *__restrict__ off, uint64_t V, uint32_t threshold,
                                                      const uint32_t *__restrict__ pos, uint32_t *__restrict__ list) {
  for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (uint64_t)gridDim.x * blockDim.x)
    if (off[v + 1] - off[v] > threshold) list[pos[v]] = (uint32_t)v;  // (pos[v] < number of long rows <= V)
}

// The calling wavefront's share of the reverse row [lo, hi): the 64-entry chunks that start at lo + first, lo + first +
// stride, ...  Every argument but `lane` is wave-uniform.  Returns the lane's cheapest candidate (CP_NONE: none);
// *gathered += the entries whose state row was read.
__device__ __forceinline__ uint64_t cp_pull_span(const uint32_t *__restrict__ rnbr, const uint64_t *__restrict__ wrev,
                                                 const unsigned long long *__restrict__ mask,
                                                 const uint64_t *__restrict__ F, uint64_t lo, uint64_t hi, uint32_t first,
                                                 uint32_t stride, bool all, int lane, uint64_t *gathered) {
  uint64_t best = CP_NONE;
  for (uint64_t c = lo + first; c < hi; c += stride) {
    const uint64_t i = c + lane;
    uint32_t un = 0;
    uint64_t mk = 0, wt = 0;
    if (i < hi) {  // (i < hi <= E)
      un = rnbr[i];
      mk = mask[un];  // (un < V)
      wt = wrev[i];
    }
    uint64_t live = __ballot(all ? i < hi : mk != 0);
    *gathered += (uint64_t)__popcll(live);
    while (live) {
      uint32_t u[4];
      uint64_t m[4], w[4], x[4];
#pragma unroll
      for (int q = 0; q < 4; q++) {
        u[q] = 0, m[q] = 0, w[q] = 0;
        if (live) {
          const int j = __builtin_ctzll(live);
          live &= live - 1;
          u[q] = (uint32_t)__builtin_amdgcn_readlane((int)un, j);
          m[q] = cp_readlane_u64(mk, j);
          w[q] = cp_readlane_u64(wt, j);
        }
      }
      // (a lane whose bit is not set never uses the cell: nobody wrote it last round)
#pragma unroll
      for (int q = 0; q < 4; q++) x[q] = (m[q] >> lane) & 1 ? cp_add(F[(uint64_t)u[q] * CP_LANES + lane], w[q]) : CP_NONE;
      best = cp_min(best, cp_min(cp_min(x[0], x[1]), cp_min(x[2], x[3])));
    }
  }
  return best;
}

// what the owner of v does with its lanes' candidates; called by a whole wavefront.  counters[0] cells lowered,
// counters[2] cells reached for the first time
__device__ __forceinline__ void cp_commit(uint64_t v, uint64_t best, uint32_t round, int lane, uint64_t *__restrict__ cost,
                                          uint64_t *__restrict__ Fn, uint32_t *__restrict__ hops,
                                          unsigned long long *__restrict__ new_mask, unsigned long long *__restrict__ reach,
                                          uint64_t *lowered, uint64_t *reached) {
  uint64_t nm = 0;
  if (__ballot(best != CP_NONE)) {  // (no candidate in any lane: the own row is not read)
    const uint64_t cell = v * CP_LANES + lane;
    const uint64_t own = cost[cell];
    const bool low = best < own;
    nm = __ballot(low);
    if (low) {
      cost[cell] = best;
      Fn[cell] = best;
      hops[cell] = round;
    }
    *lowered += (uint64_t)__popcll(nm);
    *reached += (uint64_t)__popcll(__ballot(low && own == CP_NONE));
  }
  if (lane == 0) {
    new_mask[v] = nm;
    if (nm) reach[v] |= nm;  // (only this wavefront writes reach[v] after the seed kernel)
  }
}

// one wavefront per vertex; rows longer than the threshold are left to k_cp_pull_long
__global__ __launch_bounds__(256) void k_cp_pull(const uint32_t *__restrict__ roff, const uint32_t *__restrict__ rnbr,
                                                 const uint64_t *__restrict__ wrev,
                                                 const unsigned long long *__restrict__ mask,
                                                 const uint64_t *__restrict__ F, uint64_t V, uint32_t threshold, int all,
                                                 uint32_t round, uint64_t *__restrict__ cost, uint64_t *__restrict__ Fn,
                                                 uint32_t *__restrict__ hops, unsigned long long *__restrict__ new_mask,
                                                 unsigned long long *__restrict__ reach,
                                                 unsigned long long *__restrict__ counters) {
  const int lane = threadIdx.x & 63;
  uint64_t gathered = 0, lowered = 0, reached = 0;
  for (uint64_t v = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); v < V; v += (uint64_t)gridDim.x * 4) {
    const uint32_t lo = roff[v], hi = roff[v + 1];
    if (hi - lo > threshold) continue;
    const uint64_t best = cp_pull_span(rnbr, wrev, mask, F, lo, hi, 0, 64, all != 0, lane, &gathered);
    cp_commit(v, best, round, lane, cost, Fn, hops, new_mask, reach, &lowered, &reached);
  }
  if (lane == 0) {
    if (lowered) atomicAdd(&counters[0], (unsigned long long)lowered);
    if (gathered) atomicAdd(&counters[1], (unsigned long long)gathered);
    if (reached) atomicAdd(&counters[2], (unsigned long long)reached);
  }
}

// one workgroup per listed row (workgroups stride over the list: its length is a device word, no host round trip)
__global__ __launch_bounds__(256) void k_cp_pull_long(const uint32_t *__restrict__ roff, const uint32_t *__restrict__ rnbr,
                                                      const uint64_t *__restrict__ wrev,
                                                      const unsigned long long *__restrict__ mask,
                                                      const uint64_t *__restrict__ F, const uint32_t *__restrict__ list,
                                                      const uint64_t *__restrict__ n_list, int all, uint32_t round,
                                                      uint64_t *__restrict__ cost, uint64_t *__restrict__ Fn,
                                                      uint32_t *__restrict__ hops, unsigned long long *__restrict__ new_mask,
                                                      unsigned long long *__restrict__ reach,
                                                      unsigned long long *__restrict__ counters) {
  __shared__ uint64_t s_part[4][CP_LANES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t n = *n_list;
  uint64_t gathered = 0, lowered = 0, reached = 0;
  for (uint64_t r = blockIdx.x; r < n; r += gridDim.x) {
    const uint32_t v = list[r];
    const uint32_t lo = roff[v], hi = roff[v + 1];
    s_part[wave][lane] = cp_pull_span(rnbr, wrev, mask, F, lo, hi, (uint32_t)wave * 64, 256, all != 0, lane, &gathered);
    __syncthreads();
    if (wave == 0) {
      const uint64_t best = cp_min(cp_min(s_part[0][lane], s_part[1][lane]), cp_min(s_part[2][lane], s_part[3][lane]));
      cp_commit(v, best, round, lane, cost, Fn, hops, new_mask, reach, &lowered, &reached);
    }
    __syncthreads();  // (s_part is written again by the next row)
  }
  if (lane == 0) {
    if (lowered) atomicAdd(&counters[0], (unsigned long long)lowered);
    if (gathered) atomicAdd(&counters[1], (unsigned long long)gathered);
    if (reached) atomicAdd(&counters[2], (unsigned long long)reached);
  }
}

__global__ __launch_bounds__(256) void k_cp_targets(const uint32_t *__restrict__ dense, uint64_t n,
                                                    uint8_t *__restrict__ flag) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    if (dense[i] != INVALID_U32) flag[dense[i]] = 1;  // (dense[i] < V; duplicates write the same byte)
}

// the reach words of tile `tile` that pass the target filter, one vertex a lane (0 past V)
__device__ __forceinline__ uint64_t cp_tile_mask(const unsigned long long *__restrict__ reach,
                                                 const uint8_t *__restrict__ tflag, uint64_t V, uint64_t tile, int lane) {
  const uint64_t v = tile * 64 + lane;
  uint64_t mk = v < V ? reach[v] : 0;
  if (mk && tflag && !tflag[v]) mk = 0;
  return mk;
}

// cnt[lane * n_tiles + tile] = rows of source lane `lane` in the tile
__global__ __launch_bounds__(256) void k_cp_count(const unsigned long long *__restrict__ reach,
                                                  const uint8_t *__restrict__ tflag, uint64_t V, uint64_t n_tiles,
                                                  uint32_t *__restrict__ cnt) {
  const int lane = threadIdx.x & 63;
  for (uint64_t tile = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); tile < n_tiles; tile += (uint64_t)gridDim.x * 4) {
    const uint64_t mk = cp_tile_mask(reach, tflag, V, tile, lane);
    uint64_t live = __ballot(mk != 0);
    uint32_t c = 0;
    while (live) {
      const int j = __builtin_ctzll(live);
      live &= live - 1;
      c += (uint32_t)((cp_readlane_u64(mk, j) >> lane) & 1);
    }
    cnt[(uint64_t)lane * n_tiles + tile] = c;
  }
}

// pos: the exclusive prefix of cnt; its total (< 2^32, checked by the caller) is the columns' length
__global__ __launch_bounds__(256) void k_cp_write(const unsigned long long *__restrict__ reach,
                                                  const uint64_t *__restrict__ cost, const uint32_t *__restrict__ hops,
                                                  const uint8_t *__restrict__ tflag, uint64_t V, uint64_t n_tiles,
                                                  const uint32_t *__restrict__ pos, const int64_t *__restrict__ vid,
                                                  int64_t *__restrict__ out_src, int64_t *__restrict__ out_id,
                                                  int64_t *__restrict__ out_cost, int32_t *__restrict__ out_hops) {
  const int lane = threadIdx.x & 63;
  for (uint64_t tile = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); tile < n_tiles; tile += (uint64_t)gridDim.x * 4) {
    const uint64_t mk = cp_tile_mask(reach, tflag, V, tile, lane);
    uint64_t live = __ballot(mk != 0);
    uint32_t at = pos[(uint64_t)lane * n_tiles + tile];
    while (live) {
      const int j = __builtin_ctzll(live);
      live &= live - 1;
      if ((cp_readlane_u64(mk, j) >> lane) & 1) {  // (at < pos of the next (lane, tile) <= the total)
        const uint64_t v = tile * 64 + j;           // (v < V: its reach word is not 0)
        out_src[at] = lane;
        out_id[at] = vid[v];
        out_cost[at] = (int64_t)cost[v * CP_LANES + lane];  // (a reached cell: <= INT64_MAX)
        out_hops[at] = (int32_t)hops[v * CP_LANES + lane];
        at++;
      }
    }
  }
}

// ---- the paths: a backward trace off the fixpoint's cost and hops

// len[p] = rows of pair p's path (hops + 1; 0: the target is unreached, no vertex, or its cost is saturated);
// listed[p] = 1 if the target has a cost in the pair's lane (a row of the pair table); *n_saturated += the saturated ones
__global__ __launch_bounds__(256) void k_cpp_len(const uint64_t *__restrict__ cost, const uint32_t *__restrict__ hops,
                                                 const uint32_t *__restrict__ pair_lane,
                                                 const uint32_t *__restrict__ dst_dense, uint64_t n_pairs,
                                                 uint32_t *__restrict__ len, uint32_t *__restrict__ listed,
                                                 unsigned long long *__restrict__ n_saturated) {
  uint64_t saturated = 0;
  for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_pairs; p += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t t = dst_dense[p];
    uint32_t n = 0, have = 0;
    if (t != INVALID_U32) {
      const uint64_t cell = (uint64_t)t * CP_LANES + pair_lane[p];  // (t < V, pair_lane[p] < n_src <= 64)
      const uint64_t c = cost[cell];
      if (c != CP_NONE) {
        have = 1;
        if (c == CP_MAX)
          saturated++;  // "at least": listed, never traced
        else
          n = hops[cell] + 1u;  // (hops <= V - 1)
      }
    }
    len[p] = n;
    listed[p] = have;
  }
  saturated = wave_reduce_add_u64(saturated);  // (the whole wave is back together behind the loop)
  if ((threadIdx.x & 63) == 0 && saturated) atomicAdd(n_saturated, (unsigned long long)saturated);
}

// pos: the exclusive prefix of listed; its total is the table's length
__global__ __launch_bounds__(256) void k_cpp_pairs(const uint64_t *__restrict__ cost, const uint32_t *__restrict__ hops,
                                                   const uint32_t *__restrict__ pair_lane,
                                                   const uint32_t *__restrict__ dst_dense, uint64_t n_pairs,
                                                   const uint32_t *__restrict__ len, const uint32_t *__restrict__ listed,
                                                   const uint32_t *__restrict__ pos, int64_t *__restrict__ out_pair,
                                                   int64_t *__restrict__ out_cost, int32_t *__restrict__ out_hops,
                                                   int32_t *__restrict__ out_traced) {
  for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_pairs; p += (uint64_t)gridDim.x * blockDim.x) {
    if (!listed[p]) continue;
    const uint64_t cell = (uint64_t)dst_dense[p] * CP_LANES + pair_lane[p];  // (listed: the target is a vertex with a cost)
    const uint32_t at = pos[p];                                              // (at < the total)
    out_pair[at] = (int64_t)p;
    out_cost[at] = (int64_t)cost[cell];
    out_hops[at] = (int32_t)hops[cell];
    out_traced[at] = len[p] ? 1 : 0;
  }
}

// One lane group of L lanes per pair (grid-strided), the groups of a wavefront advancing in lockstep: each trip of the
// loop every group reads one chunk of L entries of the reverse row of its x and ballots for the first entry that
// qualifies; it either commits the step and moves to the predecessor or moves its cursor.  All state is uniform inside a
// group and every cross-lane operation is executed by the whole wavefront.  There is never a loop over vertices: i, the
// hops still to go, falls by one per committed step and a search that passes the end of its row ends the pair (`bad`).
// *scanned += per step the entries of the row up to and including the one taken (a function of the input alone).
template <int L>
__global__ __launch_bounds__(256) void k_cpp_trace(const uint64_t *__restrict__ cost, const uint32_t *__restrict__ hops,
                                                   const uint32_t *__restrict__ pair_lane,
                                                   const uint32_t *__restrict__ dst_dense, uint64_t n_pairs,
                                                   const uint32_t *__restrict__ base /* exclusive scan of len */,
                                                   const uint32_t *__restrict__ len, const uint32_t *__restrict__ roff,
                                                   const uint32_t *__restrict__ rnbr, const uint64_t *__restrict__ wrev,
                                                   const uint32_t *__restrict__ rpos, const uint32_t *__restrict__ epos,
                                                   const int64_t *__restrict__ eid, const int64_t *__restrict__ vid,
                                                   int64_t *__restrict__ out_pair, int32_t *__restrict__ out_step,
                                                   int64_t *__restrict__ out_vtx, int64_t *__restrict__ out_edge /* nullable */,
                                                   int64_t *__restrict__ out_cost, unsigned long long *__restrict__ scanned,
                                                   uint32_t *__restrict__ bad /* != 0: cost state and CSR disagree */) {
  constexpr int GPW = 64 / L;  // groups per wavefront
  constexpr uint64_t GMASK = L == 64 ? ~0ULL : ((1ULL << (L % 64)) - 1ULL);
  const int lane = threadIdx.x & 63, gbase = (lane / L) * L, gl = lane % L;
  const uint64_t wave0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  const bool want_edges = out_edge != nullptr;
  uint64_t looked = 0;  // (counted by the group's first lane)
  for (uint64_t pbase = wave0 * GPW; pbase < n_pairs; pbase += nwaves * GPW) {
    const uint64_t p = pbase + (uint64_t)(lane / L);
    const uint32_t n = p < n_pairs ? len[p] : 0u;
    const uint64_t row0 = n ? base[p] : 0;
    const uint32_t bl = n ? pair_lane[p] : 0u;
    uint32_t x = n ? dst_dense[p] : 0u;                          // the vertex of step i
    uint32_t i = n ? n - 1 : 0u;                                 // hops(s, x): the steps still to take
    uint64_t cx = n ? cost[(uint64_t)x * CP_LANES + bl] : 0ull;  // cost(s, x)
    if (n && i == 0 && gl == 0) {                                // s == t: the row of step 0
      out_pair[row0] = (int64_t)p;
      out_step[row0] = 0;
      out_vtx[row0] = vid[x];
      if (want_edges) out_edge[row0] = -1;
      out_cost[row0] = (int64_t)cx;
    }
    bool active = n && i >= 1;
    uint32_t c = 0, e = 0, c0 = 0;  // cursor, end and start of x's reverse row
    if (active) {
      c = c0 = roff[x];
      e = roff[x + 1];
    }
    while (__any(active)) {
      const uint32_t idx = c + (uint32_t)gl;
      const bool inb = active && idx < e;  // (c < e <= E <= 2^32 - 2 and gl < 64: no wrap that passes the test)
      uint32_t u = 0;
      uint64_t cu = CP_NONE;
      bool hit = false;
      if (inb) {
        u = rnbr[idx];                                        // (idx < e <= E; u < V)
        const uint64_t w = wrev[idx];
        const uint64_t cell = (uint64_t)u * CP_LANES + bl;
        cu = cost[cell];
        if (cu != CP_NONE && cp_add(cu, w) == cx) hit = hops[cell] == i - 1;  // (a hops cell only behind its cost cell)
      }
      const uint64_t g = (__ballot(hit) >> gbase) & GMASK;
      const int first = g ? __ffsll((long long)g) - 1 : 0;
      const uint32_t sel_u = (uint32_t)__shfl((int)u, gbase + first, 64);
      const uint64_t sel_c = (uint64_t)__shfl((unsigned long long)cu, gbase + first, 64);
      if (active) {
        if (g) {
          const uint32_t at = c + (uint32_t)first;  // the entry taken: pred(s, x) -> x
          if (gl == 0) {
            looked += (uint64_t)(at - c0) + 1;
            int64_t rowid = -1;
            if (want_edges) {
              const uint32_t fp = rpos[at];  // (fp < E)
              rowid = eid ? eid[fp] : (int64_t)epos[fp];
              out_edge[row0 + i] = rowid;
            }
            out_pair[row0 + i] = (int64_t)p;  // (row0 + i < row0 + len[p] <= the total)
            out_step[row0 + i] = (int32_t)i;
            out_vtx[row0 + i] = vid[x];
            out_cost[row0 + i] = (int64_t)cx;
          }
          x = sel_u;
          cx = sel_c;
          i -= 1;
          if (i >= 1) {
            c = c0 = roff[x];
            e = roff[x + 1];
          } else {  // hops 0 with a cost: the lane's source
            if (gl == 0) {
              out_pair[row0] = (int64_t)p;
              out_step[row0] = 0;
              out_vtx[row0] = vid[x];
              if (want_edges) out_edge[row0] = -1;
              out_cost[row0] = (int64_t)cx;
            }
            active = false;
          }
        } else if (e - c <= (uint32_t)L) {  // (c <= e; the chunk was the row's last, or the row is empty)
          // no entry qualifies: never at the fixpoint of an unsaturated cell
          if (gl == 0) atomicOr(bad, 1u);
          active = false;
        } else {
          c += L;
        }
      }
    }
  }
  looked = wave_reduce_add_u64(looked);  // (pbase is wave-uniform: the whole wave leaves the loop together)
  if (lane == 0 && looked) atomicAdd(scanned, (unsigned long long)looked);
}

inline dim3 cp_wave_grid(gg_ctx *ctx, uint64_t n) {  // 256-thread workgroups, a wavefront per item, striding
  uint64_t want = (n + 3) / 4, cap = (uint64_t)ctx->num_cus * 32;
  if (ctx->max_grid_tiles && ctx->max_grid_tiles < cap) cap = ctx->max_grid_tiles;
  return dim3((unsigned)(want < cap ? (want ? want : 1) : cap));
}

using WeightsOwner = Owner<gg_edge_weights, gg_edge_weights_destroy>;

// What a finished batch leaves on the device for its caller (pool blocks of the caller's ApiScope).
struct CpSolved {
  uint64_t *words = nullptr;  // device words: cells lowered, rows gathered, cells reached, rows, the number of long rows
  uint64_t *cost = nullptr, *F[2] = {nullptr, nullptr};
  uint32_t *hops = nullptr;
  unsigned long long *mask[2] = {nullptr, nullptr}, *reach = nullptr;
  uint64_t rounds = 0;  // the pull rounds that ran
};
constexpr int CP_WORDS = 5;

// The batch of gg_cheapest64 (V >= 1): state, seeds and the rounds up to max_hops (< 0: to the fixpoint).
int cp_solve(gg_ctx *ctx, gg_csr *csr, const gg_edge_weights *weights, const int64_t *src_ids, int n_src, int64_t max_hops,
             CpSolved *s) {
  const uint64_t V = csr->V, E = csr->E;
  hipStream_t st = ctx->stream;
  const uint32_t threshold = ctx->cp_long_row ? ctx->cp_long_row : CP_LONG_ROW;
  const int all = ctx->cp_gather_mode == 1;

  uint64_t *words = nullptr;
  GG_TRY(ctx->dev_alloc((void **)&words, CP_WORDS * sizeof(uint64_t)));
  GG_HIP(hipMemsetAsync(words, 0, CP_WORDS * sizeof(uint64_t), st));
  uint64_t *d_nlong = words + 4;
  s->words = words;

  // the state: 3 x 512 V + 256 V + 24 V bytes (GG_ERR_OOM from the pool if they do not fit)
  uint64_t *cost = nullptr, *F[2] = {nullptr, nullptr};
  uint32_t *hops = nullptr;
  unsigned long long *mask[2] = {nullptr, nullptr}, *reach = nullptr;
  GG_TRY(ctx->dev_alloc((void **)&cost, V * CP_LANES * sizeof(uint64_t)));
  GG_TRY(ctx->dev_alloc((void **)&hops, V * CP_LANES * sizeof(uint32_t)));
  GG_TRY(ctx->dev_alloc((void **)&reach, V * sizeof(uint64_t)));
  for (int b = 0; b < 2; b++) {
    GG_TRY(ctx->dev_alloc((void **)&F[b], V * CP_LANES * sizeof(uint64_t)));
    GG_TRY(ctx->dev_alloc((void **)&mask[b], V * sizeof(uint64_t)));
  }
  GG_HIP(hipMemsetAsync(cost, 0xFF, V * CP_LANES * sizeof(uint64_t), st));
  GG_HIP(hipMemsetAsync(mask[0], 0, V * sizeof(uint64_t), st));
  GG_HIP(hipMemsetAsync(reach, 0, V * sizeof(uint64_t), st));
  s->cost = cost, s->hops = hops, s->reach = reach;
  for (int b = 0; b < 2; b++) s->F[b] = F[b], s->mask[b] = mask[b];

  const dim3 vgrid = stride_grid(ctx, V);
  const uint32_t *list = nullptr;
  if (E && threshold != UINT32_MAX) {
    uint32_t *flag = nullptr, *l = nullptr;
    GG_TRY(ctx->dev_alloc((void **)&flag, V * sizeof(uint32_t)));
    GG_TRY(ctx->dev_alloc((void **)&l, V * sizeof(uint32_t)));
    GG_LAUNCH(ctx, "cp_long_flag", k_cp_long_flag, vgrid, dim3(256), 0, (const uint32_t *)csr->roff, V, threshold, flag);
    GG_TRY(scan_exclusive_u32(ctx, flag, flag, V, d_nlong));
    GG_LAUNCH(ctx, "cp_long_list", k_cp_long_list, vgrid, dim3(256), 0, (const uint32_t *)csr->roff, V, threshold,
              (const uint32_t *)flag, l);
    ctx->dev_free(flag);
    list = l;
  }

  uint32_t *dense = nullptr;
  GG_TRY(upload_ids(ctx, csr, src_ids, (uint64_t)n_src, &dense));
  GG_LAUNCH(ctx, "cp_seed", k_cp_seed, dim3(1), dim3(64), 0, (const uint32_t *)dense, n_src, cost, F[0], hops, mask[0],
            reach, (unsigned long long *)(words + 2));

  // The rounds.  Round V cannot lower a cell (a cheapest walk of non-negative weights has at most V - 1 edges), so
  // a larger bound changes nothing; a round that lowers nothing ends the loop, bounded or not (the fixpoint).
  const uint64_t limit = E == 0 ? 0 : (max_hops < 0 || (uint64_t)max_hops > V ? V : (uint64_t)max_hops);
  const dim3 pull_grid = cp_wave_grid(ctx, V);
  uint64_t long_grid = (uint64_t)ctx->num_cus * 8;
  if (V < long_grid) long_grid = V;
  if (ctx->max_grid_tiles && ctx->max_grid_tiles < long_grid) long_grid = ctx->max_grid_tiles;
  uint64_t rounds = 0, lowered_before = 0;
  int cur = 0;
  for (uint64_t r = 1; r <= limit; r++) {
    const int nxt = cur ^ 1;
    GG_LAUNCH(ctx, "cp_pull", k_cp_pull, pull_grid, dim3(256), 0, (const uint32_t *)csr->roff,
              (const uint32_t *)csr->rnbr_by_src, (const uint64_t *)weights->w, (const unsigned long long *)mask[cur],
              (const uint64_t *)F[cur], V, threshold, all, (uint32_t)r, cost, F[nxt], hops, mask[nxt], reach,
              (unsigned long long *)words);
    if (list)
      GG_LAUNCH(ctx, "cp_pull_long", k_cp_pull_long, dim3((unsigned)long_grid), dim3(256), 0, (const uint32_t *)csr->roff,
                (const uint32_t *)csr->rnbr_by_src, (const uint64_t *)weights->w, (const unsigned long long *)mask[cur],
                (const uint64_t *)F[cur], list, (const uint64_t *)d_nlong, all, (uint32_t)r, cost, F[nxt], hops,
                mask[nxt], reach, (unsigned long long *)words);
    cur = nxt;
    rounds = r;
    uint64_t lowered = 0;  // the round's one look at the device: did it lower a cell
    GG_TRY(read_back(ctx, {{words, sizeof(uint64_t), &lowered}}));
    if (lowered == lowered_before) break;
    lowered_before = lowered;
  }
  s->rounds = rounds;
  return GG_OK;
}

// hw: the first three device words of the batch
inline void cp_fill_stats(gg_cheapest_stats *stats, uint64_t rounds, uint64_t E, const uint64_t *hw) {
  stats->rounds = rounds;
  stats->reached_pairs = hw[2];
  stats->cells_lowered = hw[0];
  stats->entries_pulled = rounds * E;
  stats->rows_gathered = hw[1];
}

}  // namespace
}  // namespace gg

extern "C" int gg_edge_weights_create(gg_ctx *ctx, const gg_csr *csr_c, const int64_t *weights, uint64_t n_weights, int by,
                                      gg_edge_weights **out) {
  if (out) *out = nullptr;
  if (!ctx || !csr_c || csr_c->ctx != ctx || !out || (!weights && n_weights)) {
    set_error("gg_edge_weights_create: bad context / csr / weights / out argument");
    return GG_ERR_INVALID_ARG;
  }
  if (by != GG_WEIGHTS_BY_ROWID && by != GG_WEIGHTS_BY_ENTRY) {
    set_error("gg_edge_weights_create: by = %d is neither GG_WEIGHTS_BY_ROWID nor GG_WEIGHTS_BY_ENTRY", by);
    return GG_ERR_INVALID_ARG;
  }
  if (csr_c->n_parts > 1) {
    set_error("gg_edge_weights_create needs a whole CSR, not a shard (gg_csr_build_shard)");
    return GG_ERR_STATE;
  }
  if (by == GG_WEIGHTS_BY_ROWID && !csr_c->has_rowid) {
    set_error("gg_edge_weights_create: GG_WEIGHTS_BY_ROWID needs a CSR built with edge rowids (gg_ctx_set_edge_rowid)");
    return GG_ERR_STATE;
  }
  const uint64_t E = csr_c->E;
  if (by == GG_WEIGHTS_BY_ENTRY && n_weights != E) {
    set_error("gg_edge_weights_create: %llu weights for %llu CSR entries", (unsigned long long)n_weights,
              (unsigned long long)E);
    return GG_ERR_INVALID_ARG;
  }
  if (E && !n_weights) {
    set_error("gg_edge_weights_create: an edge row's rowid lies outside the 0 weights given");
    return GG_ERR_INVALID_ARG;
  }
  ApiScope scope(ctx);
  GG_HIP(hipSetDevice(ctx->device));
  gg_csr *csr = const_cast<gg_csr *>(csr_c);
  WeightsOwner w(new gg_edge_weights());
  w->ctx = ctx, w->csr = csr_c, w->E = E;
  GG_TRY(ctx->dev_alloc((void **)&w->w, (E ? E : 1) * sizeof(uint64_t)));
  ctx->keep(w->w);
  if (E) {
    GG_TRY(ensure_reverse_by_source(ctx, csr));
    GG_TRY(ensure_reverse_pos_by_source(ctx, csr));
    int64_t *given = nullptr;
    unsigned long long *flags = nullptr;
    GG_TRY(ctx->dev_alloc((void **)&given, n_weights * sizeof(int64_t)));
    GG_TRY(ctx->dev_alloc((void **)&flags, 2 * sizeof(unsigned long long)));
    GG_HIP(hipMemcpyAsync(given, weights, n_weights * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    GG_HIP(hipMemsetAsync(flags, 0, 2 * sizeof(unsigned long long), ctx->stream));
    GG_LAUNCH(ctx, "cp_permute", k_cp_permute, stride_grid(ctx, E), dim3(256), 0, (const uint32_t *)csr->rpos_by_src,
              (const int64_t *)csr->eid, (const uint32_t *)csr->epos, (const int64_t *)given, n_weights,
              by == GG_WEIGHTS_BY_ENTRY ? 1 : 0, E, w->w, flags);
    uint64_t hf[2] = {0, 0};
    GG_TRY(read_back(ctx, {{flags, sizeof(hf), hf}}));  // (the copy of the caller's weights has read them by now)
    if (hf[0]) {
      set_error("gg_edge_weights_create: an edge row's rowid lies outside the %llu weights given",
                (unsigned long long)n_weights);
      return GG_ERR_INVALID_ARG;
    }
    if (hf[1]) {
      set_error("gg_edge_weights_create: a weight is negative");
      return GG_ERR_INVALID_ARG;
    }
  }
  *out = w.release();
  return GG_OK;
}

extern "C" void gg_edge_weights_destroy(gg_edge_weights *w) {
  if (!w) return;
  if (w->ctx) w->ctx->dev_free(w->w);  // (no synchronisation: gg_result_destroy's argument)
  delete w;
}

extern "C" int gg_cheapest64(gg_ctx *ctx, const gg_csr *csr_c, const gg_edge_weights *weights, const int64_t *src_ids,
                             int n_src, int64_t max_hops, const int64_t *dst_ids, uint64_t n_dst, gg_cheapest_stats *stats,
                             gg_result **out_result) {
  if (out_result) *out_result = nullptr;
  if (stats) memset(stats, 0, sizeof(*stats));
  if (!ctx || !csr_c || csr_c->ctx != ctx || !weights || !src_ids) {
    set_error("gg_cheapest64: bad context / csr / weights / source argument");
    return GG_ERR_INVALID_ARG;
  }
  if (n_src < 1 || n_src > GG_BFS_LANES) {
    set_error("gg_cheapest64: %d sources outside 1..%d (one wavefront lane each)", n_src, GG_BFS_LANES);
    return GG_ERR_INVALID_ARG;
  }
  if (!dst_ids && n_dst) {
    set_error("gg_cheapest64: %llu targets without a list", (unsigned long long)n_dst);
    return GG_ERR_INVALID_ARG;
  }
  if (!stats && !out_result) {
    set_error("gg_cheapest64: neither stats nor out_result is asked for");
    return GG_ERR_INVALID_ARG;
  }
  if (csr_c->n_parts > 1) {
    set_error("gg_cheapest64 needs a whole CSR, not a shard (gg_csr_build_shard)");
    return GG_ERR_STATE;
  }
  if (weights->ctx != ctx || weights->csr != csr_c || weights->E != csr_c->E) {
    set_error("gg_cheapest64: the weights were made for another CSR or context");
    return GG_ERR_INVALID_ARG;
  }
  ApiScope scope(ctx);
  GG_HIP(hipSetDevice(ctx->device));
  gg_csr *csr = const_cast<gg_csr *>(csr_c);
  const uint64_t V = csr->V, E = csr->E;
  ResultOwner res;
  if (out_result) res = make_result(ctx, ResultKind::CHEAPEST);
  if (V) {
    hipStream_t st = ctx->stream;
    CpSolved sv;
    GG_TRY(cp_solve(ctx, csr, weights, src_ids, n_src, max_hops, &sv));
    uint64_t *words = sv.words, *d_rows = words + 3;
    const uint64_t *cost = sv.cost;
    const uint32_t *hops = sv.hops;
    const unsigned long long *reach = sv.reach;
    const uint64_t rounds = sv.rounds;

    uint8_t *tflag = nullptr;  // null: every vertex may end a row
    if (dst_ids) {
      uint32_t *tdense = nullptr;
      GG_TRY(ctx->dev_alloc((void **)&tflag, V));
      GG_HIP(hipMemsetAsync(tflag, 0, V, st));
      GG_TRY(upload_ids(ctx, csr, dst_ids, n_dst, &tdense));
      if (n_dst)
        GG_LAUNCH(ctx, "cp_targets", k_cp_targets, stride_grid(ctx, n_dst), dim3(256), 0, (const uint32_t *)tdense, n_dst,
                  tflag);
    }

    const uint64_t n_tiles = (V + 63) / 64;
    uint32_t *cnt = nullptr;  // 64 x n_tiles, lane-major
    GG_TRY(ctx->dev_alloc((void **)&cnt, CP_LANES * n_tiles * sizeof(uint32_t)));
    const dim3 tile_grid = cp_wave_grid(ctx, n_tiles);
    GG_LAUNCH(ctx, "cp_count", k_cp_count, tile_grid, dim3(256), 0, (const unsigned long long *)reach,
              (const uint8_t *)tflag, V, n_tiles, cnt);
    GG_TRY(scan_exclusive_u32(ctx, cnt, cnt, CP_LANES * n_tiles, d_rows));
    uint64_t hw[4];
    GG_TRY(read_back(ctx, {{words, sizeof(hw), hw}}));
    const uint64_t n_rows = hw[3];
    if (n_rows >= (1ull << 32)) {
      set_error("gg_cheapest64: %llu rows (2^32 or more): ask for fewer sources or targets", (unsigned long long)n_rows);
      return GG_ERR_TOO_LARGE;
    }
    if (res) {
      res->rows[0] = n_rows;
      if (n_rows) {
        for (int c = 0; c < 4; c++) {
          GG_TRY(ctx->dev_alloc((void **)&res->cols[0][c], n_rows * (c == 3 ? sizeof(int32_t) : sizeof(int64_t))));
          ctx->keep(res->cols[0][c]);
        }
        GG_LAUNCH(ctx, "cp_write", k_cp_write, tile_grid, dim3(256), 0, (const unsigned long long *)reach,
                  (const uint64_t *)cost, (const uint32_t *)hops, (const uint8_t *)tflag, V, n_tiles, (const uint32_t *)cnt,
                  (const int64_t *)csr->vid, res->cols[0][0], res->cols[0][1], res->cols[0][2],
                  reinterpret_cast<int32_t *>(res->cols[0][3]));
      }
    }
    if (stats) cp_fill_stats(stats, rounds, E, hw);
  }
  if (out_result) *out_result = res.release();
  return GG_OK;
}

extern "C" int gg_cheapest64_rows(const gg_result *res, uint64_t *n_rows) {
  if (!res || !n_rows) return GG_ERR_INVALID_ARG;
  GG_TRY(expect_kind(res, ResultKind::CHEAPEST, "gg_cheapest64_rows"));
  *n_rows = res->rows[0];
  return GG_OK;
}

extern "C" int gg_cheapest64_fetch(const gg_result *res, uint64_t offset, uint32_t max_rows, int64_t *src_index,
                                   int64_t *vertex_id, int64_t *cost, int32_t *hops, uint32_t *n_out) {
  if (!res || !n_out) return GG_ERR_INVALID_ARG;
  GG_TRY(expect_kind(res, ResultKind::CHEAPEST, "gg_cheapest64_fetch"));
  int64_t *const *col = res->cols[0];
  return fetch_slice(res->ctx, res->rows[0], offset, max_rows,
                     {{src_index, col[0]}, {vertex_id, col[1]}, {cost, col[2]}, {hops, col[3], sizeof(int32_t)}}, n_out);
}

extern "C" int gg_cheapest64_paths(gg_ctx *ctx, const gg_csr *csr_c, const gg_edge_weights *weights, const int64_t *src_ids,
                                   int n_src, const uint32_t *pair_lane, const int64_t *pair_dst_ids, uint64_t n_pairs,
                                   int want_edges, gg_cheapest_paths_stats *stats, gg_result **out_result) {
  if (out_result) *out_result = nullptr;
  if (stats) memset(stats, 0, sizeof(*stats));
  if (!ctx || !csr_c || csr_c->ctx != ctx || !weights || !src_ids || !out_result) {
    set_error("gg_cheapest64_paths: bad context / csr / weights / source / out_result argument");
    return GG_ERR_INVALID_ARG;
  }
  if (n_src < 1 || n_src > GG_BFS_LANES) {
    set_error("gg_cheapest64_paths: %d sources outside 1..%d (one wavefront lane each)", n_src, GG_BFS_LANES);
    return GG_ERR_INVALID_ARG;
  }
  if (n_pairs >= (1ull << 32)) {  // (before the arrays are looked at)
    set_error("gg_cheapest64_paths: %llu pairs do not fit a 32-bit pair index", (unsigned long long)n_pairs);
    return GG_ERR_TOO_LARGE;
  }
  if (n_pairs && (!pair_lane || !pair_dst_ids)) {
    set_error("gg_cheapest64_paths: %llu pairs without their lane or target list", (unsigned long long)n_pairs);
    return GG_ERR_INVALID_ARG;
  }
  if (csr_c->n_parts > 1) {
    set_error("gg_cheapest64_paths needs a whole CSR, not a shard (gg_csr_build_shard)");
    return GG_ERR_STATE;
  }
  if (weights->ctx != ctx || weights->csr != csr_c || weights->E != csr_c->E) {
    set_error("gg_cheapest64_paths: the weights were made for another CSR or context");
    return GG_ERR_INVALID_ARG;
  }
  if (want_edges && !csr_c->has_rowid) {
    set_error("gg_cheapest64_paths with edges needs a CSR built with edge rowids (gg_ctx_set_edge_rowid(ctx, 1))");
    return GG_ERR_STATE;
  }
  for (uint64_t i = 0; i < n_pairs; i++)
    if (pair_lane[i] >= (uint32_t)n_src) {
      set_error("gg_cheapest64_paths: pair %llu names source %u of %d", (unsigned long long)i, pair_lane[i], n_src);
      return GG_ERR_INVALID_ARG;
    }
  ApiScope scope(ctx);
  GG_HIP(hipSetDevice(ctx->device));
  gg_csr *csr = const_cast<gg_csr *>(csr_c);
  const uint64_t V = csr->V, E = csr->E, n = n_pairs;
  ResultOwner res = make_result(ctx, ResultKind::CHEAPEST_PATHS);
  if (V) {
    hipStream_t st = ctx->stream;
    CpSolved sv;
    GG_TRY(cp_solve(ctx, csr, weights, src_ids, n_src, -1, &sv));
    for (int b = 0; b < 2; b++) {  // about 1 KiB per vertex, back to the pool before the rows are allocated
      ctx->dev_free(sv.F[b]);
      ctx->dev_free(sv.mask[b]);
    }
    // device words: path rows, reached pairs, saturated pairs, entries scanned, then (32 bits) the lost-search flag
    uint64_t *pw = nullptr, hw[3] = {0, 0, 0}, hp[3] = {0, 0, 0};
    constexpr int NPW = 5;
    GG_TRY(ctx->dev_alloc((void **)&pw, NPW * sizeof(uint64_t)));
    GG_HIP(hipMemsetAsync(pw, 0, NPW * sizeof(uint64_t), st));
    uint32_t *lane_dev = nullptr, *dst_dense = nullptr, *len = nullptr, *base = nullptr, *listed = nullptr, *pos = nullptr;
    if (n) {
      GG_TRY(ctx->dev_alloc((void **)&lane_dev, n * sizeof(uint32_t)));
      GG_TRY(ctx->dev_alloc((void **)&len, n * sizeof(uint32_t)));
      GG_TRY(ctx->dev_alloc((void **)&base, n * sizeof(uint32_t)));
      GG_TRY(ctx->dev_alloc((void **)&listed, n * sizeof(uint32_t)));
      GG_TRY(ctx->dev_alloc((void **)&pos, n * sizeof(uint32_t)));
      GG_HIP(hipMemcpyAsync(lane_dev, pair_lane, n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
      GG_TRY(upload_ids(ctx, csr, pair_dst_ids, n, &dst_dense));
      GG_LAUNCH(ctx, "cpp_len", k_cpp_len, stride_grid(ctx, n), dim3(256), 0, (const uint64_t *)sv.cost,
                (const uint32_t *)sv.hops, (const uint32_t *)lane_dev, (const uint32_t *)dst_dense, n, len, listed,
                (unsigned long long *)(pw + 2));
      GG_TRY(scan_exclusive_u32(ctx, len, base, n, pw));
      GG_TRY(scan_exclusive_u32(ctx, listed, pos, n, pw + 1));
    }
    GG_TRY(read_back(ctx, {{sv.words, sizeof(hw), hw}, {pw, sizeof(hp), hp}}));  // (the pair arrays have been read by now)
    const uint64_t rows = hp[0], reached = hp[1];
    if (rows >= (1ull << 32)) {  // (the bases are 32-bit and have wrapped: nothing is traced)
      set_error("gg_cheapest64_paths: %llu path rows in one batch (2^32 or more): ask for fewer pairs",
                (unsigned long long)rows);
      return GG_ERR_TOO_LARGE;
    }
    if (reached) {
      int64_t **col = res->cols[CPP_PAIRS_TABLE];
      for (int c = 0; c < 4; c++)
        GG_TRY(ctx->dev_alloc((void **)&col[c], reached * (c >= 2 ? sizeof(int32_t) : sizeof(int64_t))));
      for (int c = 0; c < 4; c++) ctx->keep(col[c]);
      GG_LAUNCH(ctx, "cpp_pairs", k_cpp_pairs, stride_grid(ctx, n), dim3(256), 0, (const uint64_t *)sv.cost,
                (const uint32_t *)sv.hops, (const uint32_t *)lane_dev, (const uint32_t *)dst_dense, n, (const uint32_t *)len,
                (const uint32_t *)listed, (const uint32_t *)pos, col[0], col[1], reinterpret_cast<int32_t *>(col[2]),
                reinterpret_cast<int32_t *>(col[3]));
      res->rows[CPP_PAIRS_TABLE] = reached;
    }
    uint64_t scanned = 0;
    if (rows) {
      int64_t **col = res->cols[CPP_ROWS_TABLE];  // pair, step (int32), vertex, edge if asked for, cost
      for (int c = 0; c < 5; c++)
        if (c != 3 || want_edges) GG_TRY(ctx->dev_alloc((void **)&col[c], rows * (c == 1 ? sizeof(int32_t) : sizeof(int64_t))));
      constexpr int L = GG_CPP_LANES, GPW = 64 / L;
      static_assert(L == 64 || L == 32 || L == 16 || L == 8 || L == 4, "GG_CPP_LANES divides the wavefront");
      const uint64_t waves = (n + GPW - 1) / GPW, max_waves = (uint64_t)ctx->num_cus * 32;
      const unsigned grid = (unsigned)(((waves < max_waves ? waves : max_waves) * 64 + 255) / 256);
      GG_LAUNCH(ctx, "cpp_trace", (k_cpp_trace<L>), dim3(grid), dim3(256), 0, (const uint64_t *)sv.cost,
                (const uint32_t *)sv.hops, (const uint32_t *)lane_dev, (const uint32_t *)dst_dense, n, (const uint32_t *)base,
                (const uint32_t *)len, (const uint32_t *)csr->roff, (const uint32_t *)csr->rnbr_by_src,
                (const uint64_t *)weights->w, (const uint32_t *)csr->rpos_by_src, (const uint32_t *)csr->epos,
                (const int64_t *)csr->eid, (const int64_t *)csr->vid, col[0], reinterpret_cast<int32_t *>(col[1]), col[2],
                col[3], col[4], (unsigned long long *)(pw + 3), reinterpret_cast<uint32_t *>(pw + 4));
      uint32_t n_bad = 0;
      GG_TRY(read_back(ctx, {{pw + 3, sizeof(uint64_t), &scanned}, {pw + 4, sizeof(uint32_t), &n_bad}}));
      if (n_bad) {
        set_error("gg_cheapest64_paths: a reached vertex has no reverse entry that explains its cost one hop earlier "
                  "(cost state and CSR disagree)");
        for (int c = 0; c < 5; c++) col[c] = nullptr;  // (not kept: the ApiScope frees them)
        return GG_ERR_STATE;
      }
      for (int c = 0; c < 5; c++)
        if (col[c]) ctx->keep(col[c]);
      res->rows[CPP_ROWS_TABLE] = rows;
    }
    if (stats) {
      cp_fill_stats(&stats->search, sv.rounds, E, hw);
      stats->pairs_reached = reached;
      stats->pairs_saturated = hp[2];
      stats->rows = rows;
      stats->entries_scanned = scanned;
    }
  }
  *out_result = res.release();
  return GG_OK;
}

extern "C" int gg_cheapest64_paths_rows(const gg_result *res, int table, uint64_t *n_rows) {
  if (!res || !n_rows) return GG_ERR_INVALID_ARG;
  GG_TRY(expect_kind(res, ResultKind::CHEAPEST_PATHS, "gg_cheapest64_paths_rows"));
  if (table != CPP_PAIRS_TABLE && table != CPP_ROWS_TABLE) {
    set_error("gg_cheapest64_paths_rows: table %d is neither 0 (pairs) nor 1 (path rows)", table);
    return GG_ERR_INVALID_ARG;
  }
  *n_rows = res->rows[table];
  return GG_OK;
}

extern "C" int gg_cheapest64_paths_fetch_pairs(const gg_result *res, uint64_t offset, uint32_t max_rows, int64_t *pair_index,
                                               int64_t *cost, int32_t *hops, int32_t *traced, uint32_t *n_out) {
  if (!res || !n_out) return GG_ERR_INVALID_ARG;
  GG_TRY(expect_kind(res, ResultKind::CHEAPEST_PATHS, "gg_cheapest64_paths_fetch_pairs"));
  int64_t *const *col = res->cols[CPP_PAIRS_TABLE];
  return fetch_slice(res->ctx, res->rows[CPP_PAIRS_TABLE], offset, max_rows,
                     {{pair_index, col[0]}, {cost, col[1]}, {hops, col[2], sizeof(int32_t)}, {traced, col[3], sizeof(int32_t)}},
                     n_out);
}

extern "C" int gg_cheapest64_paths_fetch(const gg_result *res, uint64_t offset, uint32_t max_rows, int64_t *pair_index,
                                         int32_t *step, int64_t *vertex_id, int64_t *edge_rowid, int64_t *cost,
                                         uint32_t *n_out) {
  if (!res || !n_out) return GG_ERR_INVALID_ARG;
  GG_TRY(expect_kind(res, ResultKind::CHEAPEST_PATHS, "gg_cheapest64_paths_fetch"));
  if (!pair_index || !step || !vertex_id) return GG_ERR_INVALID_ARG;
  int64_t *const *col = res->cols[CPP_ROWS_TABLE];
  GG_TRY(fetch_slice(res->ctx, res->rows[CPP_ROWS_TABLE], offset, max_rows,
                     {{pair_index, col[0]}, {vertex_id, col[2]}, {edge_rowid, col[3]}, {cost, col[4]},
                      {step, col[1], sizeof(int32_t)}},
                     n_out));
  if (!col[3] && edge_rowid)
    for (uint32_t r = 0; r < *n_out; r++) edge_rowid[r] = -1;  // traced without edges
  return GG_OK;
}

extern "C" int gg_debug_cheapest(gg_ctx *ctx, uint32_t long_row_entries, int gather_mode) {
  if (!ctx || gather_mode < 0 || gather_mode > 1) return GG_ERR_INVALID_ARG;
  ctx->cp_long_row = long_row_entries;
  ctx->cp_gather_mode = gather_mode;
  return GG_OK;
}
