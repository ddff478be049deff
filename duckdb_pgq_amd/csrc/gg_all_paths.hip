// gg_all_paths.hip — how many shortest paths a pair has, and all of them (ALL SHORTEST), off a finished 64-lane BFS
// (gg_bfs.hip).
//
// With the reference's operators ALL SHORTEST is a recursive UNION ALL CTE over friends_shortest joined with knows once
// per level (PhysicalRecursiveCTE::GetData, src/execution/operator/set/physical_recursive_cte.cpp:60-139, probing
// JoinHashTable::Probe / ScanStructure::NextInnerJoin, src/execution/join_hashtable.cpp:304-476), and the count is a hash
// aggregate above that CTE (src/execution/operator/aggregate/physical_hash_aggregate.cpp:152-266): every path row is formed
// on the CPU just to be folded away.  Here the distance cells dist[V][64] are still on the device when the batch ends, and
// the number of shortest paths is one recurrence over the shortest-path DAG they describe.
//
// The relation (include/gg.h, gg_bfs64_all_paths): for lane s and vertex x at distance d,
//   sigma(s, s) = 1,   sigma(s, x) = SUM over the entries u -> x of x's reverse row with dist(s, u) == d - 1 of sigma(s, u),
// every sum saturating at 2^64 - 1, and path number r of a pair is unranked from the target backwards over x's reverse row
// in csr->rnbr_by_src order (gg_paths.hip): an entry one level closer is taken if r < sigma(s, u), else r -= sigma(s, u).
//
//   sigma[v * 64 + lane]  u64, 512 V bytes.  Never cleared: a cell is read only where dist says it was written.
//   k_ap_seed      sigma[s * 64 + i] = 1 for lane i with dense index s
//   k_ap_count     one pass per BFS level L, one wavefront per vertex x, lane = BFS lane.  mask = the lanes with
//                  dist[x][lane] == L; 0: the vertex cost its distance row.  Else 64 entries of x's reverse row a trip, a
//                  lane each: the lane reads the entry's whole distance row (64 / 128 B) and folds it into the mask of the
//                  BFS lanes that stand at L - 1 there; the entries whose mask meets x's are taken four at a time — four
//                  512-B gathers in flight, as k_pc_pull (gg_pairs.hip) — each lane adding sigma[u * 64 + lane] where its
//                  bit is set.  One store of the row's masked lanes; no atomics on sigma.
//   k_ap_pair      per pair d, sigma, kept = min(sigma, path_limit), kept * (d + 1); the saturating totals per workgroup,
//                  folded by k_ap_totals (one workgroup, no atomics)
//   scans          exclusive u32 prefixes of reached (table 0 positions), kept (path bases), kept * (d + 1) (row bases),
//                  the last two clamped to 2^32 - 1 on the way in; the totals that decide are the saturating ones
//   k_ap_pairs_write  table 0
//   k_ap_unrank    GG_PATH_LANES lanes per output path: the pair by binary search of the path index in the path bases, then
//                  per step chunks of GG_PATH_LANES entries of the reverse row — distance cell, sigma where one level closer,
//                  a saturating inclusive prefix over the group, the first lane whose prefix exceeds r is taken, else r -=
//                  the group's total.  As k_path_trace: every cross-lane operation is executed by the whole wavefront, the
//                  state is uniform per group, and a device flag is set instead of a spin.
// Bytes per count pass (model): V * 64 * cell bytes (every distance row) + for the vertices with lanes at the level 8 B of
// offsets + per entry (sigma_entries) 4 B + one distance row of 64 / 128 B + per gathered entry (sigma_gathered) 512 B + up
// to 512 B stored.  Bytes per unranked step (model): per entry looked at 4 B + one 64 / 128-byte distance line (a gather:
// the cells of one lane lie 64 cells apart) + 8 B of sigma (its own 64-byte line) where the entry is one level closer; per
// step taken 4 B position + 8 B rowid + 36 B of result row.  The serial depth of a path is its length; no forward row is
// searched (the rowid is eid[rpos_by_src[entry]]).
#include "gg_internal.h"

#ifndef GG_PATH_LANES
#define GG_PATH_LANES 16  // as gg_paths.hip
#endif

using namespace gg;

namespace gg {
namespace {

constexpr int AP_LANES = GG_BFS_LANES;
static_assert(AP_LANES == 64, "one wavefront lane per source");
constexpr uint64_t AP_SAT = ~0ull;
enum { AP_W_PATHS = 0, AP_W_KEPT, AP_W_ROWS, AP_W_ENTRIES, AP_W_GATHERED, AP_W_REACHED, AP_W_BAD, AP_WORDS };

__host__ __device__ __forceinline__ uint64_t sat_add(uint64_t a, uint64_t b) {
  const uint64_t s = a + b;
  return s < a ? AP_SAT : s;
}
__host__ __device__ __forceinline__ uint64_t sat_mul(uint64_t a, uint64_t b) {  // b >= 1 (once per pair: the division is no cost)
  return a > AP_SAT / b ? AP_SAT : a * b;
}
__device__ __forceinline__ uint64_t wave_reduce_sat(uint64_t v) {  // call with the whole wave active
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = sat_add(v, (uint64_t)__shfl_xor((unsigned long long)v, o, 64));
  return v;
}
__device__ __forceinline__ uint64_t ap_readlane_u64(uint64_t x, int j) {  // j wave-uniform
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, j);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), j);
  return ((uint64_t)hi << 32) | lo;
}

// the fields of w that equal `want`, one bit a field, field 0 in bit 0 (exact zero-field test, no carries between fields)
__host__ __device__ __forceinline__ uint32_t eq_fields(uint64_t w, uint8_t want) {
  const uint64_t lo7 = 0x7F7F7F7F7F7F7F7FULL;
  const uint64_t x = w ^ (0x0101010101010101ULL * want);
  const uint64_t z = ~(((x & lo7) + lo7) | x | lo7);  // 0x80 in every zero byte
  return (uint32_t)(((z >> 7) * 0x0102040810204080ULL) >> 56);
}
__host__ __device__ __forceinline__ uint32_t eq_fields(uint64_t w, uint16_t want) {
  const uint64_t lo15 = 0x7FFF7FFF7FFF7FFFULL;
  const uint64_t x = w ^ (0x0001000100010001ULL * want);
  const uint64_t z = ~(((x & lo15) + lo15) | x | lo15);  // 0x8000 in every zero field
  return (uint32_t)((((z >> 15) * ((1ULL << 45) | (1ULL << 30) | (1ULL << 15) | 1ULL)) >> 45) & 0xF);
}

// bit l set iff row[l] == want: the 64 cells of one vertex, read as 16-byte pieces by ONE lane
template <typename DistT>
__device__ __forceinline__ uint64_t level_mask(const DistT *__restrict__ row, DistT want) {
  constexpr int PER_WORD = 8 / (int)sizeof(DistT), PIECES = AP_LANES * (int)sizeof(DistT) / 16;
  const uint4 *p = reinterpret_cast<const uint4 *>(row);
  uint64_t m = 0;
#pragma unroll
  for (int k = 0; k < PIECES; k++) {
    const uint4 q = p[k];
    const uint64_t w0 = ((uint64_t)q.y << 32) | q.x, w1 = ((uint64_t)q.w << 32) | q.z;
    m |= (uint64_t)eq_fields(w0, want) << (k * 2 * PER_WORD);
    m |= (uint64_t)eq_fields(w1, want) << ((k * 2 + 1) * PER_WORD);
  }
  return m;
}

__global__ __launch_bounds__(64) void k_ap_seed(const uint32_t *__restrict__ dense, int n_src,
                                                uint64_t *__restrict__ sigma) {
  const int i = threadIdx.x;
  if (i < n_src && dense[i] != INVALID_U32) sigma[(uint64_t)dense[i] * AP_LANES + i] = 1;  // (dense[i] < V)
}

template <typename DistT>
__global__ __launch_bounds__(256) void k_ap_count(const DistT *__restrict__ dist, const uint32_t *__restrict__ roff,
                                                  const uint32_t *__restrict__ rnbr, uint64_t V, uint32_t level,
                                                  uint64_t *__restrict__ sigma, unsigned long long *__restrict__ words) {
  const int lane = threadIdx.x & 63;
  const DistT at = (DistT)level, before = (DistT)(level - 1);
  uint64_t entries = 0, gathered = 0;
  for (uint64_t v = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); v < V; v += (uint64_t)gridDim.x * 4) {
    const bool mine = dist[v * AP_LANES + lane] == at;
    const uint64_t vmask = __ballot(mine);
    if (!vmask) continue;
    const uint32_t lo = roff[v], hi = roff[v + 1];
    entries += hi - lo;
    uint64_t acc = 0;
    for (uint64_t c = lo; c < hi; c += 64) {
      const uint64_t i = c + lane;
      uint32_t un = 0;
      uint64_t mk = 0;
      if (i < hi) {  // (i < hi <= E)
        un = rnbr[i];
        mk = level_mask<DistT>(dist + (uint64_t)un * AP_LANES, before) & vmask;  // (un < V)
      }
      uint64_t live = __ballot(mk != 0);
      gathered += (uint64_t)__popcll(live);
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
            m[q] = ap_readlane_u64(mk, j);
          }
        }
#pragma unroll
        for (int q = 0; q < 4; q++) x[q] = (m[q] >> lane) & 1 ? sigma[(uint64_t)u[q] * AP_LANES + lane] : 0;
        acc = sat_add(sat_add(acc, sat_add(x[0], x[1])), sat_add(x[2], x[3]));
      }
    }
    if (mine) sigma[v * AP_LANES + lane] = acc;
  }
  if (lane == 0 && entries) {
    atomicAdd(&words[AP_W_ENTRIES], (unsigned long long)entries);
    if (gathered) atomicAdd(&words[AP_W_GATHERED], (unsigned long long)gathered);
  }
}

// per pair: hops (-1: no row), sigma, kept, and the scans' inputs; the saturating totals into words
template <typename DistT>
__global__ __launch_bounds__(256) void k_ap_pair(const DistT *__restrict__ dist, const uint64_t *__restrict__ sigma,
                                                 const uint32_t *__restrict__ pair_lane,
                                                 const uint32_t *__restrict__ dst_dense, uint64_t n_pairs,
                                                 uint64_t path_limit, int32_t *__restrict__ hops,
                                                 uint64_t *__restrict__ paths, uint64_t *__restrict__ kept,
                                                 uint32_t *__restrict__ reached, uint32_t *__restrict__ kept32,
                                                 uint32_t *__restrict__ rows32,
                                                 uint64_t *__restrict__ partial /* 3 per workgroup */) {
  __shared__ uint64_t s_part[4][3];
  uint64_t t_paths = 0, t_kept = 0, t_rows = 0;
  for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_pairs; p += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t t = dst_dense[p];
    int32_t h = -1;
    uint64_t sg = 0, kp = 0, rw = 0;
    if (t != INVALID_U32) {
      const uint64_t cell = (uint64_t)t * AP_LANES + pair_lane[p];
      const DistT d = dist[cell];
      if (d != (DistT)~(DistT)0) {
        h = (int32_t)d;
        sg = sigma[cell];
        kp = path_limit && sg > path_limit ? path_limit : sg;
        rw = sat_mul(kp, (uint64_t)d + 1);
      }
    }
    hops[p] = h;
    paths[p] = sg;
    kept[p] = kp;
    reached[p] = h >= 0 ? 1u : 0u;
    kept32[p] = kp > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)kp;  // clamped, not wrapped (the totals below decide)
    rows32[p] = rw > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)rw;
    t_paths = sat_add(t_paths, sg);
    t_kept = sat_add(t_kept, kp);
    t_rows = sat_add(t_rows, rw);
  }
  t_paths = wave_reduce_sat(t_paths);  // (saturating addition is associative and commutative: the same bits by any route)
  t_kept = wave_reduce_sat(t_kept);
  t_rows = wave_reduce_sat(t_rows);
  if ((threadIdx.x & 63) == 0) {
    s_part[threadIdx.x >> 6][0] = t_paths;
    s_part[threadIdx.x >> 6][1] = t_kept;
    s_part[threadIdx.x >> 6][2] = t_rows;
  }
  __syncthreads();
  if (threadIdx.x < 3)  // no atomics: 10^4 waves exchanging on one word take longer than everything else in the call
    partial[(uint64_t)blockIdx.x * 3 + threadIdx.x] = sat_add(sat_add(s_part[0][threadIdx.x], s_part[1][threadIdx.x]),
                                                               sat_add(s_part[2][threadIdx.x], s_part[3][threadIdx.x]));
}

// one workgroup: words[AP_W_PATHS / KEPT / ROWS] = the saturating sums of the workgroups' partials
__global__ __launch_bounds__(256) void k_ap_totals(const uint64_t *__restrict__ partial, uint32_t n_blocks,
                                                   unsigned long long *__restrict__ words) {
  __shared__ uint64_t s_part[4][3];
  uint64_t t[3] = {0, 0, 0};
  for (uint32_t b = threadIdx.x; b < n_blocks; b += blockDim.x)
    for (int k = 0; k < 3; k++) t[k] = sat_add(t[k], partial[(uint64_t)b * 3 + k]);
  for (int k = 0; k < 3; k++) t[k] = wave_reduce_sat(t[k]);
  if ((threadIdx.x & 63) == 0)
    for (int k = 0; k < 3; k++) s_part[threadIdx.x >> 6][k] = t[k];
  __syncthreads();
  if (threadIdx.x < 3)
    words[AP_W_PATHS + threadIdx.x] = sat_add(sat_add(s_part[0][threadIdx.x], s_part[1][threadIdx.x]),
                                              sat_add(s_part[2][threadIdx.x], s_part[3][threadIdx.x]));
}

__global__ __launch_bounds__(256) void k_ap_pairs_write(const int32_t *__restrict__ hops, const uint64_t *__restrict__ paths,
                                                        const uint64_t *__restrict__ kept, const uint32_t *__restrict__ pos,
                                                        uint64_t n_pairs, int64_t *__restrict__ out_pair,
                                                        int32_t *__restrict__ out_hops, uint64_t *__restrict__ out_paths,
                                                        uint64_t *__restrict__ out_kept) {
  for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_pairs; p += (uint64_t)gridDim.x * blockDim.x)
    if (hops[p] >= 0) {  // (pos[p] < pairs reached = the columns' length)
      const uint32_t at = pos[p];
      out_pair[at] = (int64_t)p;
      out_hops[at] = hops[p];
      out_paths[at] = paths[p];
      out_kept[at] = kept[p];
    }
}

// One lane group per output path (grid-strided), n_paths = the sum of kept < 2^32 and n_rows = the sum of kept * (d + 1)
// < 2^32, so pbase / rbase are exact.  All state is uniform inside a group; a group that has finished, or has none, idles
// through the trips of the others.  (c += L cannot wrap: c < e <= E <= 2^32 - 2 and a trip past e ends the search.)
template <typename DistT, int L>
__global__ __launch_bounds__(256) void k_ap_unrank(const DistT *__restrict__ dist, const uint64_t *__restrict__ sigma,
                                                   const uint32_t *__restrict__ pair_lane,
                                                   const uint32_t *__restrict__ dst_dense, const int32_t *__restrict__ hops,
                                                   const uint32_t *__restrict__ pbase, const uint32_t *__restrict__ rbase,
                                                   uint64_t n_pairs, uint64_t n_paths, const uint32_t *__restrict__ roff,
                                                   const uint32_t *__restrict__ rnbr /* sources ascending */,
                                                   const uint32_t *__restrict__ rpos /* nullable: no edges */,
                                                   const uint32_t *__restrict__ epos, const int64_t *__restrict__ eid,
                                                   const int64_t *__restrict__ vid, int64_t *__restrict__ out_pair,
                                                   int64_t *__restrict__ out_path, int32_t *__restrict__ out_step,
                                                   int64_t *__restrict__ out_vtx, int64_t *__restrict__ out_edge /* nullable */,
                                                   unsigned long long *__restrict__ bad) {
  constexpr int GPW = 64 / L;  // groups per wavefront
  constexpr uint64_t GMASK = L == 64 ? ~0ULL : ((1ULL << (L % 64)) - 1ULL);
  const int lane = threadIdx.x & 63, gbase = (lane / L) * L, gl = lane % L;
  const uint64_t wave0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  const bool want_edges = out_edge != nullptr;
  for (uint64_t qbase = wave0 * GPW; qbase < n_paths; qbase += nwaves * GPW) {
    const uint64_t q = qbase + (uint64_t)(lane / L);
    const bool have = q < n_paths;
    uint64_t p = 0;
    if (have) {  // the last pair whose base is <= q: pairs that keep nothing share the base of the next one that does
      uint64_t lo = 0, hi = n_pairs;
      while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (pbase[mid] <= q) lo = mid; else hi = mid;
      }
      p = lo;
    }
    const uint64_t rank = have ? q - pbase[p] : 0;
    uint32_t i = have ? (uint32_t)hops[p] : 0u;  // steps still to take; the vertex x is that of step i
    const uint64_t row0 = have ? (uint64_t)rbase[p] + rank * ((uint64_t)i + 1) : 0;
    const uint32_t bl = have ? pair_lane[p] : 0u;
    uint32_t x = have ? dst_dense[p] : 0u;
    uint64_t r = rank;
    if (have && i == 0 && gl == 0) {  // s == t: the row of step 0
      out_pair[row0] = (int64_t)p;
      out_path[row0] = (int64_t)rank;
      out_step[row0] = 0;
      out_vtx[row0] = vid[x];
      if (want_edges) out_edge[row0] = -1;
    }
    bool active = have && i >= 1;
    uint32_t c = 0, e = 0;  // cursor and end of x's reverse row
    if (active) {
      c = roff[x];
      e = roff[x + 1];
    }
    while (__any(active)) {
      const uint32_t idx = c + (uint32_t)gl;
      const bool inb = active && idx < e;
      const uint32_t un = inb ? rnbr[idx] : 0u;
      uint64_t sg = 0;
      if (inb && dist[(uint64_t)un * AP_LANES + bl] == (DistT)(i - 1)) sg = sigma[(uint64_t)un * AP_LANES + bl];
      uint64_t pre = sg;  // saturating inclusive prefix over the group
#pragma unroll
      for (int o = 1; o < L; o <<= 1) {
        const uint64_t up = (uint64_t)__shfl_up((unsigned long long)pre, (unsigned)o, L);
        if (gl >= o) pre = sat_add(pre, up);
      }
      const bool hit = inb && pre > r;
      const uint64_t g = (__ballot(hit) >> gbase) & GMASK;
      const int first = g ? __ffsll((long long)g) - 1 : 0;
      const uint64_t total = (uint64_t)__shfl((unsigned long long)pre, gbase + L - 1, 64);
      // the prefix below the lane taken: exact, because it does not exceed r < 2^64 - 1
      const uint64_t below = (uint64_t)__shfl((unsigned long long)pre, gbase + (first > 0 ? first - 1 : 0), 64);
      const uint32_t sel = (uint32_t)__shfl((int)un, gbase + first, 64);
      if (active) {
        if (g) {
          if (first > 0) r -= below;
          if (gl == 0) {
            int64_t rowid = -1;
            if (want_edges) {
              const uint32_t at = rpos[c + (uint32_t)first];
              rowid = eid ? eid[at] : (int64_t)epos[at];
            }
            out_pair[row0 + i] = (int64_t)p;
            out_path[row0 + i] = (int64_t)rank;
            out_step[row0 + i] = (int32_t)i;
            out_vtx[row0 + i] = vid[x];
            if (want_edges) out_edge[row0 + i] = rowid;
          }
          x = sel;
          i -= 1;
          if (i >= 1) {
            c = roff[x];
            e = roff[x + 1];
          } else {
            if (gl == 0) {
              out_pair[row0] = (int64_t)p;
              out_path[row0] = (int64_t)rank;
              out_step[row0] = 0;
              out_vtx[row0] = vid[x];
              if (want_edges) out_edge[row0] = -1;
            }
            active = false;
          }
        } else {
          r -= total;  // (total <= r)
          c += L;
          if (c >= e) {  // the row ended below the rank: never with a consistent BFS, sigma and CSR
            if (gl == 0) atomicOr(bad, 1ull);
            active = false;
          }
        }
      }
    }
  }
}

template <typename DistT>
int all_paths_emit_t(gg_ctx *ctx, gg_csr *csr, const DistT *dist, uint32_t levels, const AllPathsRequest &rq) {
  const uint64_t V = csr->V, n = rq.n_pairs;
  hipStream_t s = ctx->stream;
  gg_all_paths_stats st;
  memset(&st, 0, sizeof(st));
  uint64_t *sigma = nullptr;
  unsigned long long *words = nullptr;
  uint32_t *src_dense = nullptr;
  GG_TRY(ctx->dev_alloc((void **)&sigma, V * AP_LANES * sizeof(uint64_t)));  // (GG_ERR_OOM if it does not fit)
  GG_TRY(ctx->dev_alloc((void **)&words, AP_WORDS * sizeof(uint64_t)));
  GG_HIP(hipMemsetAsync(words, 0, AP_WORDS * sizeof(uint64_t), s));
  GG_TRY(upload_ids(ctx, csr, rq.src_ids, (uint64_t)rq.n_src, &src_dense));
  GG_LAUNCH(ctx, "ap_seed", k_ap_seed, dim3(1), dim3(64), 0, (const uint32_t *)src_dense, rq.n_src, sigma);
  {
    const uint64_t want = (V + 3) / 4, cap = (uint64_t)ctx->num_cus * 32;  // four vertices (wavefronts) per workgroup
    const dim3 grid((unsigned)(want < cap ? want : cap));
    if (levels) GG_TRY(ensure_reverse(ctx, csr));  // (returns at once: a BFS of one level or more wrote the rows)
    for (uint32_t level = 1; level <= levels; level++)
      GG_LAUNCH(ctx, "ap_count", (k_ap_count<DistT>), grid, dim3(256), 0, dist, (const uint32_t *)csr->roff,
                (const uint32_t *)csr->rnbr_rows, V, level, sigma, words);
  }

  uint32_t *lane_dev = nullptr, *dst_dense = nullptr, *reached = nullptr, *kept32 = nullptr, *rows32 = nullptr;
  int32_t *hops = nullptr;
  uint64_t *paths = nullptr, *kept = nullptr;
  const uint64_t n1 = n ? n : 1;
  if (n) {
    GG_TRY(ctx->dev_alloc((void **)&lane_dev, n1 * sizeof(uint32_t)));
    GG_TRY(ctx->dev_alloc((void **)&reached, n1 * sizeof(uint32_t)));
    GG_TRY(ctx->dev_alloc((void **)&kept32, n1 * sizeof(uint32_t)));
    GG_TRY(ctx->dev_alloc((void **)&rows32, n1 * sizeof(uint32_t)));
    GG_TRY(ctx->dev_alloc((void **)&hops, n1 * sizeof(int32_t)));
    GG_TRY(ctx->dev_alloc((void **)&paths, n1 * sizeof(uint64_t)));
    GG_TRY(ctx->dev_alloc((void **)&kept, n1 * sizeof(uint64_t)));
    GG_HIP(hipMemcpyAsync(lane_dev, rq.pair_lane, n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    GG_TRY(upload_ids(ctx, csr, rq.pair_dst_ids, n, &dst_dense));
    const dim3 pgrid = stride_grid(ctx, n);
    uint64_t *partial = nullptr;
    GG_TRY(ctx->dev_alloc((void **)&partial, (size_t)pgrid.x * 3 * sizeof(uint64_t)));
    GG_LAUNCH(ctx, "ap_pair", (k_ap_pair<DistT>), pgrid, dim3(256), 0, dist, (const uint64_t *)sigma,
              (const uint32_t *)lane_dev, (const uint32_t *)dst_dense, n, rq.path_limit, hops, paths, kept, reached, kept32,
              rows32, partial);
    GG_LAUNCH(ctx, "ap_totals", k_ap_totals, dim3(1), dim3(256), 0, (const uint64_t *)partial, (uint32_t)pgrid.x, words);
    GG_TRY(scan_exclusive_u32(ctx, reached, reached, n, (uint64_t *)(words + AP_W_REACHED)));
    if (rq.materialise) {
      GG_TRY(scan_exclusive_u32(ctx, kept32, kept32, n, nullptr));
      GG_TRY(scan_exclusive_u32(ctx, rows32, rows32, n, nullptr));
    }
  }
  uint64_t hw[AP_WORDS];
  GG_TRY(read_back(ctx, {{words, sizeof(hw), hw}}));  // every total in one look
  st.pairs_reached = hw[AP_W_REACHED];
  st.paths = hw[AP_W_PATHS];
  st.paths_kept = hw[AP_W_KEPT];
  st.rows = hw[AP_W_ROWS];
  st.sigma_entries = hw[AP_W_ENTRIES];
  st.sigma_gathered = hw[AP_W_GATHERED];
  if (rq.materialise && (st.paths_kept >= (1ull << 32) || st.rows >= (1ull << 32))) {  // (nothing is written)
    set_error("gg_bfs64_all_paths: %llu paths of %llu rows in one batch (2^32 or more; 2^64 - 1: or more than that): set "
              "a path_limit or ask for fewer pairs",
              (unsigned long long)st.paths_kept, (unsigned long long)st.rows);
    return GG_ERR_TOO_LARGE;
  }

  gg_result *res = rq.res;
  int64_t *t0[4] = {nullptr, nullptr, nullptr, nullptr}, *t1[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  const int n1cols = rq.want_edges ? 5 : 4;  // pair, path, step (int32), vertex, edge
  if (res && st.pairs_reached) {
    for (int c = 0; c < 4; c++)  // pair, hops (int32), paths, kept
      GG_TRY(ctx->dev_alloc((void **)&t0[c], st.pairs_reached * (c == 1 ? sizeof(int32_t) : sizeof(int64_t))));
    GG_LAUNCH(ctx, "ap_pairs_write", k_ap_pairs_write, stride_grid(ctx, n), dim3(256), 0, (const int32_t *)hops,
              (const uint64_t *)paths, (const uint64_t *)kept, (const uint32_t *)reached, n, t0[0],
              reinterpret_cast<int32_t *>(t0[1]), reinterpret_cast<uint64_t *>(t0[2]), reinterpret_cast<uint64_t *>(t0[3]));
  }
  if (res && rq.materialise && st.rows) {
    GG_TRY(ensure_reverse_by_source(ctx, csr));
    if (rq.want_edges) GG_TRY(ensure_reverse_pos_by_source(ctx, csr));
    for (int c = 0; c < n1cols; c++)
      GG_TRY(ctx->dev_alloc((void **)&t1[c], st.rows * (c == 2 ? sizeof(int32_t) : sizeof(int64_t))));
    constexpr int L = GG_PATH_LANES, GPW = 64 / L;
    static_assert(L == 64 || L == 32 || L == 16 || L == 8 || L == 4, "GG_PATH_LANES divides the wavefront");
    const uint64_t waves = (st.paths_kept + GPW - 1) / GPW, max_waves = (uint64_t)ctx->num_cus * 32;
    const unsigned grid = (unsigned)(((waves < max_waves ? waves : max_waves) * 64 + 255) / 256);
    GG_LAUNCH(ctx, "ap_unrank", (k_ap_unrank<DistT, L>), dim3(grid), dim3(256), 0, dist, (const uint64_t *)sigma,
              (const uint32_t *)lane_dev, (const uint32_t *)dst_dense, (const int32_t *)hops, (const uint32_t *)kept32,
              (const uint32_t *)rows32, n, st.paths_kept, (const uint32_t *)csr->roff, (const uint32_t *)csr->rnbr_by_src,
              rq.want_edges ? (const uint32_t *)csr->rpos_by_src : (const uint32_t *)nullptr, (const uint32_t *)csr->epos,
              (const int64_t *)csr->eid, (const int64_t *)csr->vid, t1[0], t1[1], reinterpret_cast<int32_t *>(t1[2]), t1[3],
              rq.want_edges ? t1[4] : (int64_t *)nullptr, words + AP_W_BAD);
  }
  if (res) {
    uint64_t n_bad = 0;
    GG_TRY(read_back(ctx, {{words + AP_W_BAD, sizeof(uint64_t), &n_bad}}));
    if (n_bad) {  // (nothing was kept: the caller's ApiScope frees the columns)
      set_error("gg_bfs64_all_paths: a reverse row ended below a path's rank (distances and CSR disagree)");
      return GG_ERR_STATE;
    }
    for (int c = 0; c < 4; c++)
      if (t0[c]) ctx->keep(t0[c]), res->cols[AP_PAIRS_TABLE][c] = t0[c];
    for (int c = 0; c < 5; c++)
      if (t1[c]) ctx->keep(t1[c]), res->cols[AP_ROWS_TABLE][c] = t1[c];
    res->rows[AP_PAIRS_TABLE] = st.pairs_reached;
    res->rows[AP_ROWS_TABLE] = t1[0] ? st.rows : 0;
  }
  if (rq.stats) {
    const gg_bfs_stats bfs = rq.stats->bfs;  // (bfs_run fills it after this returns)
    *rq.stats = st;
    rq.stats->bfs = bfs;
  }
  return GG_OK;
}

}  // namespace

int all_paths_emit(gg_ctx *ctx, gg_csr *csr, const void *dist, size_t cell_bytes, uint32_t levels,
                   const AllPathsRequest &rq) {
  return cell_bytes == 1 ? all_paths_emit_t<uint8_t>(ctx, csr, (const uint8_t *)dist, levels, rq)
                         : all_paths_emit_t<uint16_t>(ctx, csr, (const uint16_t *)dist, levels, rq);
}

}  // namespace gg

extern "C" int gg_bfs64_all_paths(gg_ctx *ctx, const gg_csr *csr, const int64_t *src_ids, int n_src, int max_hops,
                                  const uint32_t *pair_lane, const int64_t *pair_dst_ids, uint64_t n_pairs,
                                  uint64_t path_limit, int want_edges, int materialise, gg_all_paths_stats *stats,
                                  gg_result **out_result) {
  if (out_result) *out_result = nullptr;
  if (stats) memset(stats, 0, sizeof(*stats));
  if (!ctx || !csr || csr->ctx != ctx || (n_pairs && (!pair_lane || !pair_dst_ids))) return GG_ERR_INVALID_ARG;
  if (materialise ? !out_result : (!out_result && !stats)) {
    set_error("gg_bfs64_all_paths: %s", materialise ? "materialising needs out_result" : "neither stats nor out_result is asked for");
    return GG_ERR_INVALID_ARG;
  }
  if (csr->n_parts > 1) {
    set_error("gg_bfs64_all_paths needs a whole CSR, not a shard");
    return GG_ERR_STATE;
  }
  if (materialise && want_edges && !csr->has_rowid) {
    set_error("gg_bfs64_all_paths with edges needs a CSR built with edge rowids (gg_ctx_set_edge_rowid(ctx, 1))");
    return GG_ERR_STATE;
  }
  if (n_pairs >= (1ull << 32)) {
    set_error("gg_bfs64_all_paths: %llu pairs do not fit a 32-bit pair index", (unsigned long long)n_pairs);
    return GG_ERR_TOO_LARGE;
  }
  for (uint64_t i = 0; i < n_pairs; i++)
    if (n_src < 0 || pair_lane[i] >= (uint32_t)n_src) {
      set_error("gg_bfs64_all_paths: pair %llu names source %u of %d", (unsigned long long)i, pair_lane[i], n_src);
      return GG_ERR_INVALID_ARG;
    }
  ResultOwner res;
  if (out_result) res = make_result(ctx, ResultKind::ALL_PATHS);
  const AllPathsRequest rq{src_ids, n_src, pair_lane, pair_dst_ids, n_pairs, path_limit, materialise && want_edges,
                           materialise != 0, stats, res.get()};
  GG_TRY(bfs64_all_paths_run(ctx, csr, src_ids, n_src, max_hops, stats ? &stats->bfs : nullptr, rq));
  if (out_result) *out_result = res.release();
  return GG_OK;
}

extern "C" int gg_bfs64_all_paths_rows(const gg_result *res, int table, uint64_t *n_rows) {
  if (!res || !n_rows) return GG_ERR_INVALID_ARG;
  GG_TRY(expect_kind(res, ResultKind::ALL_PATHS, "gg_bfs64_all_paths_rows"));
  if (table < 0 || table > 1) return GG_ERR_INVALID_ARG;
  *n_rows = res->rows[table];
  return GG_OK;
}

extern "C" int gg_bfs64_all_paths_fetch_pairs(const gg_result *res, uint64_t offset, uint32_t max_rows,
                                              int64_t *pair_index, int32_t *hops, uint64_t *paths, uint64_t *kept,
                                              uint32_t *n_out) {
  if (!res || !n_out) return GG_ERR_INVALID_ARG;
  GG_TRY(expect_kind(res, ResultKind::ALL_PATHS, "gg_bfs64_all_paths_fetch_pairs"));
  int64_t *const *col = res->cols[AP_PAIRS_TABLE];
  return fetch_slice(res->ctx, res->rows[AP_PAIRS_TABLE], offset, max_rows,
                     {{pair_index, col[0]}, {paths, col[2]}, {kept, col[3]}, {hops, col[1], sizeof(int32_t)}}, n_out);
}

extern "C" int gg_bfs64_all_paths_fetch(const gg_result *res, uint64_t offset, uint32_t max_rows, int64_t *pair_index,
                                        int64_t *path_index, int32_t *step, int64_t *vertex_id, int64_t *edge_rowid,
                                        uint32_t *n_out) {
  if (!res || !n_out) return GG_ERR_INVALID_ARG;
  GG_TRY(expect_kind(res, ResultKind::ALL_PATHS, "gg_bfs64_all_paths_fetch"));
  if (!pair_index || !path_index || !step || !vertex_id) return GG_ERR_INVALID_ARG;
  int64_t *const *col = res->cols[AP_ROWS_TABLE];
  GG_TRY(fetch_slice(res->ctx, res->rows[AP_ROWS_TABLE], offset, max_rows,
                     {{pair_index, col[0]}, {path_index, col[1]}, {vertex_id, col[3]}, {edge_rowid, col[4]},
                      {step, col[2], sizeof(int32_t)}}, n_out));
  if (edge_rowid && !col[4])
    for (uint32_t r = 0; r < *n_out; r++) edge_rowid[r] = -1;  // searched without edges
  return GG_OK;
}
