// gg_aggregate.hip — count(*) and sum(weight) over the h-hop walks, grouped by their start or their end vertex.
//
// The reference answers `SELECT p.id, count(*), sum(f.score) FROM person p, knows k, ..., person f GROUP BY p.id`
// (benchmark/ldbc/queries/bi-8.sql:41-53 has the 1-hop shape) with PhysicalHashAggregate above a chain of
// PhysicalHashJoin (src/execution/operator/aggregate/physical_hash_aggregate.cpp:152-266 fed by
// ScanStructure::NextInnerJoin, src/execution/join_hashtable.cpp:442-476): every walk row is formed and folded away again.
// The answer has at most V rows and is k passes over the CSR.  With a_0(v) = (1, weight(v)) and
//     a_h(u) = sum over the entries v of u's row of a_{h-1}(v)
// a_h(u) is (count, sum of the END vertices' weights) over all h-walks from u when the rows are the forward rows, and
// (count, sum of the START vertices' weights) over all h-walks into u when they are the reverse rows.  A source list
// seeds level 0 with (m, m * weight) for END (m: how often the vertex is listed) and multiplies the final a_h(u) by m
// for START.  Counts are u64 and wrap; sums are 128-bit two's complement (the reference's HUGEINT) and wrap.
//   k_agg_seed        m[v] += 1 per listed vertex (u64 atomics)
//   k_agg_seed_state  END with a list: level 0 as explicit states (m, m * weight)
//   k_agg_long_flag / scan / k_agg_long_list   the rows longer than the threshold, once per call and direction
//   k_agg_pull        16 lanes per row of up to `threshold` entries: per-lane (count, lo, hi) partials with the carry
//                     hi += (lo < addend), folded across the 16 lanes by xor shuffles that carry the same way
//   k_agg_pull_long   one workgroup of 256 per listed row: lanes, then waves through LDS, the same arithmetic
//   k_agg_flag        per vertex: has the level a group here (final count != 0)?  + the level's walks
//   scan              exclusive prefix of the flags: the groups' places, their number
//   k_agg_write       (vertex id, walks, lo, hi) of every group at its place: ascending dense index
// Both pull kernels take three forms of the level below: FORM_ONES (level 0 implicit: the 8-byte weight is gathered and
// sign-extended, the count is the row length read off the offsets), FORM_STATE (24-byte states) and FORM_COUNT (no
// weights: u64 counts only, the sums are never formed).  Addition mod 2^64 / 2^128 is associative and commutative, so
// every route and every lane order gives the same bits.
// Bytes per pass (model, levels >= 2 with weights): E * (4 B entry + 24 B gathered state) + V * (8 B of offsets +
// 24 B written).  The gathered table is 24 V bytes; whether its lines are served from L2 / Infinity Cache is not
// measured here.
#include "gg_internal.h"
#include "gg_walk_table.h"

using namespace gg;

namespace gg {
namespace {

constexpr uint32_t AGG_LONG_ROW = 512;  // default: rows of more entries go to a whole workgroup

struct AggState {  // 24 bytes
  uint64_t cnt, lo;
  int64_t hi;
};

enum AggForm { FORM_ONES = 0, FORM_STATE = 1, FORM_COUNT = 2 };

__device__ __forceinline__ void agg_add(AggState &a, uint64_t cnt, uint64_t lo, int64_t hi) {
  a.cnt += cnt;
  a.lo += lo;
  a.hi += hi + (int64_t)(a.lo < lo);  // the carry out of the low half
}

// (lo, hi) * m mod 2^128
__device__ __forceinline__ void mul128(uint64_t lo, int64_t hi, uint64_t m, uint64_t *out_lo, int64_t *out_hi) {
  *out_lo = lo * m;
  *out_hi = (int64_t)(__umul64hi(lo, m) + (uint64_t)hi * m);
}

template <int FORM>
__device__ __forceinline__ void agg_gather(AggState &a, const void *__restrict__ in, uint32_t v) {
  if (FORM == FORM_ONES) {
    const int64_t w = static_cast<const int64_t *>(in)[v];
    agg_add(a, 0, (uint64_t)w, w >> 63);  // sign-extended; the count is the row length
  } else if (FORM == FORM_STATE) {
    const AggState s = static_cast<const AggState *>(in)[v];
    agg_add(a, s.cnt, s.lo, s.hi);
  } else {
    a.cnt += static_cast<const uint64_t *>(in)[v];
  }
}

template <int FORM>
__device__ __forceinline__ void agg_store(void *__restrict__ out, uint32_t u, AggState a, uint32_t len) {
  if (FORM == FORM_ONES) a.cnt = len;
  if (FORM == FORM_COUNT)
    static_cast<uint64_t *>(out)[u] = a.cnt;
  else
    static_cast<AggState *>(out)[u] = a;
}

__device__ __forceinline__ AggState agg_shfl_xor(const AggState &a, int o) {
  AggState b;
  b.cnt = __shfl_xor((unsigned long long)a.cnt, o, 64);
  b.lo = __shfl_xor((unsigned long long)a.lo, o, 64);
  b.hi = (int64_t)__shfl_xor((unsigned long long)a.hi, o, 64);
  return b;
}

__global__ __launch_bounds__(256) void k_agg_seed(const uint32_t *__restrict__ dense, uint64_t n,
                                                  unsigned long long *__restrict__ mult) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && dense[i] != INVALID_U32) atomicAdd(&mult[dense[i]], 1ULL);
}

// level 0 of END with a source list and weights: (m, m * weight)  (without weights level 0 is the array m itself)
__global__ __launch_bounds__(256) void k_agg_seed_state(const unsigned long long *__restrict__ mult,
                                                        const int64_t *__restrict__ weights, uint64_t V,
                                                        AggState *__restrict__ st) {
  for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t m = mult[v];
    const int64_t w = weights[v];
    AggState s;
    s.cnt = m;
    mul128((uint64_t)w, w >> 63, m, &s.lo, &s.hi);
    st[v] = s;
  }
}

// count-only level 1 off an implicit level 0: the row lengths
__global__ __launch_bounds__(256) void k_agg_rowlen(const uint32_t *__restrict__ off, uint64_t V,
                                                    uint64_t *__restrict__ cnt) {
  for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (uint64_t)gridDim.x * blockDim.x)
    cnt[v] = (uint64_t)(off[v + 1] - off[v]);
}

__global__ __launch_bounds__(256) void k_agg_long_flag(const uint32_t *__restrict__ off, uint64_t V, uint32_t threshold,
                                                       uint32_t *__restrict__ flag) {
  for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (uint64_t)gridDim.x * blockDim.x)
    flag[v] = off[v + 1] - off[v] > threshold ? 1u : 0u;
}

// pos: the exclusive prefix of the flags (pos[V] does not exist: a row is long iff its length says so)
__global__ __launch_bounds__(256) void k_agg_long_list(const uint32_t *__restrict__ off, uint64_t V, uint32_t threshold,
                                                       const uint32_t *__restrict__ pos, uint32_t *__restrict__ list) {
  for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (uint64_t)gridDim.x * blockDim.x)
    if (off[v + 1] - off[v] > threshold) list[pos[v]] = (uint32_t)v;  // (pos[v] < number of long rows <= V)
}

// 16 lanes per row; rows longer than the threshold are left to k_agg_pull_long.  The loop bound is uniform over the
// workgroup, so all 16 lanes of a group reach the shuffles together.
template <int FORM>
__global__ __launch_bounds__(256) void k_agg_pull(const uint32_t *__restrict__ off, const uint32_t *__restrict__ nbr,
                                                  const void *__restrict__ in, uint64_t V, uint32_t threshold,
                                                  void *__restrict__ out) {
  const int sub = threadIdx.x & 15;
  for (uint64_t v0 = (uint64_t)blockIdx.x * 16; v0 < V; v0 += (uint64_t)gridDim.x * 16) {
    const uint64_t v = v0 + (threadIdx.x >> 4);
    AggState acc{0, 0, 0};
    uint32_t lo = 0, hi = 0;
    if (v < V) lo = off[v], hi = off[v + 1];
    const uint32_t len = hi - lo;
    const bool mine = v < V && len <= threshold;
    if (mine)
      for (uint32_t i = lo + sub; i < hi; i += 16) agg_gather<FORM>(acc, in, nbr[i]);  // (i < hi <= E)
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
      const AggState b = agg_shfl_xor(acc, o);
      agg_add(acc, b.cnt, b.lo, b.hi);
    }
    if (mine && sub == 0) agg_store<FORM>(out, (uint32_t)v, acc, len);
  }
}

// one workgroup per listed row (workgroups stride over the list: its length is a device word, no host round trip)
template <int FORM>
__global__ __launch_bounds__(256) void k_agg_pull_long(const uint32_t *__restrict__ off, const uint32_t *__restrict__ nbr,
                                                       const void *__restrict__ in, const uint32_t *__restrict__ list,
                                                       const uint64_t *__restrict__ n_list, void *__restrict__ out) {
  __shared__ AggState s_red[4];
  const uint64_t n = *n_list;
  for (uint64_t r = blockIdx.x; r < n; r += gridDim.x) {
    const uint32_t u = list[r];
    const uint32_t lo = off[u], hi = off[u + 1];
    AggState acc{0, 0, 0};
    for (uint64_t i = (uint64_t)lo + threadIdx.x; i < hi; i += 256) agg_gather<FORM>(acc, in, nbr[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const AggState b = agg_shfl_xor(acc, o);
      agg_add(acc, b.cnt, b.lo, b.hi);
    }
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 1; w < 4; w++) agg_add(acc, s_red[w].cnt, s_red[w].lo, s_red[w].hi);
      agg_store<FORM>(out, u, acc, hi - lo);
    }
    __syncthreads();  // (s_red is written again by the next row)
  }
}

// the final (walks, lo, hi) of vertex v at a level: the state, times the START multiplicity if there is a list
__device__ __forceinline__ AggState agg_final(const void *__restrict__ st, bool weighted,
                                              const unsigned long long *__restrict__ mult, uint64_t v) {
  AggState s;
  if (weighted) {
    s = static_cast<const AggState *>(st)[v];
  } else {
    s.cnt = static_cast<const uint64_t *>(st)[v];
    s.lo = s.cnt, s.hi = 0;
  }
  if (mult) {
    const uint64_t m = mult[v];
    s.cnt *= m;
    if (weighted)
      mul128(s.lo, s.hi, m, &s.lo, &s.hi);
    else
      s.lo = s.cnt;
  }
  return s;
}

// flag[v] = the level has a group at v; *walks += the groups' walks (mod 2^64)
__global__ __launch_bounds__(256) void k_agg_flag(const void *__restrict__ st, int weighted,
                                                  const unsigned long long *__restrict__ mult, uint64_t V,
                                                  uint32_t *__restrict__ flag, unsigned long long *__restrict__ walks) {
  __shared__ uint64_t s_red[4];
  uint64_t acc = 0;
  for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t c = agg_final(st, weighted != 0, mult, v).cnt;
    flag[v] = c != 0 ? 1u : 0u;
    acc += c;
  }
  acc = wave_reduce_add_u64(acc);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint64_t all = s_red[0] + s_red[1] + s_red[2] + s_red[3];
    if (all) atomicAdd(walks, (unsigned long long)all);
  }
}

// pos: the exclusive prefix of the flags
__global__ __launch_bounds__(256) void k_agg_write(const void *__restrict__ st, int weighted,
                                                   const unsigned long long *__restrict__ mult, uint64_t V,
                                                   const uint32_t *__restrict__ pos, const int64_t *__restrict__ vid,
                                                   int64_t *__restrict__ out_id, int64_t *__restrict__ out_walks,
                                                   int64_t *__restrict__ out_lo, int64_t *__restrict__ out_hi) {
  for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (uint64_t)gridDim.x * blockDim.x) {
    const AggState s = agg_final(st, weighted != 0, mult, v);
    if (s.cnt) {  // (pos[v] < groups of the level <= V: the columns have V entries)
      const uint32_t p = pos[v];
      out_id[p] = vid[v];
      out_walks[p] = (int64_t)s.cnt;
      out_lo[p] = (int64_t)s.lo;
      out_hi[p] = s.hi;
    }
  }
}

struct PullArgs {
  const uint32_t *off, *nbr;
  uint64_t V;
  uint32_t threshold;
  const uint32_t *list;      // the long rows (null: none can exist)
  const uint64_t *n_list;
};

template <int FORM>
int agg_pull(gg_ctx *ctx, const PullArgs &p, const void *in, void *out) {
  const uint64_t want = (p.V + 15) / 16;
  const unsigned grid = (unsigned)(want < (1u << 20) ? want : (1u << 20));
  GG_LAUNCH(ctx, "agg_pull", (k_agg_pull<FORM>), dim3(grid), dim3(256), 0, p.off, p.nbr, in, p.V, p.threshold, out);
  if (p.list) {
    const uint64_t cap = (uint64_t)ctx->num_cus * 8;
    GG_LAUNCH(ctx, "agg_pull_long", (k_agg_pull_long<FORM>), dim3((unsigned)(p.V < cap ? p.V : cap)), dim3(256), 0,
              p.off, p.nbr, in, p.list, p.n_list, out);
  }
  return GG_OK;
}

}  // namespace
}  // namespace gg

extern "C" int gg_khop_aggregate(gg_ctx *ctx, const gg_csr *csr_c, const int64_t *src_ids, uint64_t n_src, int k_min,
                                 int k_max, int group_by, const int64_t *weights, gg_agg_stats *stats,
                                 gg_result **out_result) {
  if (out_result) *out_result = nullptr;
  if (stats) memset(stats, 0, sizeof(*stats));
  if (!ctx || !csr_c || csr_c->ctx != ctx) {
    set_error("gg_khop_aggregate: bad context / csr argument");
    return GG_ERR_INVALID_ARG;
  }
  if (k_min < 1 || k_max > GG_MAX_HOPS || k_min > k_max) {
    set_error("gg_khop_aggregate: hops %d..%d outside 1..%d", k_min, k_max, GG_MAX_HOPS);
    return GG_ERR_INVALID_ARG;
  }
  if (group_by != GG_GROUP_START && group_by != GG_GROUP_END) {
    set_error("gg_khop_aggregate: group_by %d (0: the start vertex, 1: the end vertex)", group_by);
    return GG_ERR_INVALID_ARG;
  }
  if (!stats && !out_result) {
    set_error("gg_khop_aggregate: neither stats nor out_result is asked for");
    return GG_ERR_INVALID_ARG;
  }
  if (csr_c->n_parts > 1) {
    set_error("gg_khop_aggregate needs a whole CSR, not a shard (gg_csr_build_shard)");
    return GG_ERR_STATE;
  }
  ApiScope scope(ctx);
  GG_HIP(hipSetDevice(ctx->device));
  gg_csr *csr = const_cast<gg_csr *>(csr_c);
  const uint64_t V = csr->V, E = csr->E;
  const bool all = src_ids == nullptr, weighted = weights != nullptr, end = group_by == GG_GROUP_END;
  ResultOwner res;
  if (out_result) res = make_result(ctx, ResultKind::AGGREGATE, k_min, k_max);
  if (V && E && (all || n_src)) {
    hipStream_t st = ctx->stream;
    if (end) GG_TRY(ensure_reverse(ctx, csr));
    PullArgs p{};
    p.off = end ? csr->roff : csr->off, p.nbr = end ? csr->rnbr_rows : csr->nbr;
    p.V = V;
    p.threshold = ctx->agg_long_row ? ctx->agg_long_row : AGG_LONG_ROW;

    // device words: groups[h], walks[h], then the number of long rows
    uint64_t *words = nullptr;
    constexpr int NW = 2 * (GG_MAX_HOPS + 1) + 1;
    GG_TRY(ctx->dev_alloc((void **)&words, NW * sizeof(uint64_t)));
    GG_HIP(hipMemsetAsync(words, 0, NW * sizeof(uint64_t), st));
    uint64_t *d_groups = words, *d_walks = words + GG_MAX_HOPS + 1, *d_nlong = words + 2 * (GG_MAX_HOPS + 1);

    uint32_t *flag = nullptr;  // V u32: the long-row flags, then every level's group flags / places
    GG_TRY(ctx->dev_alloc((void **)&flag, V * sizeof(uint32_t)));
    const dim3 vgrid = stride_grid(ctx, V);
    if (p.threshold != UINT32_MAX) {
      uint32_t *list = nullptr;
      GG_TRY(ctx->dev_alloc((void **)&list, V * sizeof(uint32_t)));
      GG_LAUNCH(ctx, "agg_long_flag", k_agg_long_flag, vgrid, dim3(256), 0, p.off, V, p.threshold, flag);
      GG_TRY(scan_exclusive_u32(ctx, flag, flag, V, d_nlong));
      GG_LAUNCH(ctx, "agg_long_list", k_agg_long_list, vgrid, dim3(256), 0, p.off, V, p.threshold,
                (const uint32_t *)flag, list);
      p.list = list, p.n_list = d_nlong;
    }

    int64_t *w_dev = nullptr;
    if (weighted) {
      GG_TRY(ctx->dev_alloc((void **)&w_dev, V * sizeof(int64_t)));
      // (caller memory: the read_back below synchronises the stream before this call returns)
      GG_HIP(hipMemcpyAsync(w_dev, weights, V * sizeof(int64_t), hipMemcpyHostToDevice, st));
    }
    unsigned long long *mult = nullptr;
    if (!all) {
      uint32_t *dense = nullptr;
      GG_TRY(upload_ids(ctx, csr, src_ids, n_src, &dense));
      GG_TRY(ctx->dev_alloc((void **)&mult, V * sizeof(unsigned long long)));
      GG_HIP(hipMemsetAsync(mult, 0, V * sizeof(unsigned long long), st));
      GG_LAUNCH(ctx, "agg_seed", k_agg_seed, dim3((unsigned)((n_src + 255) / 256)), dim3(256), 0,
                (const uint32_t *)dense, n_src, mult);
    }

    const size_t st_bytes = V * (weighted ? sizeof(AggState) : sizeof(uint64_t));
    // level 0 is implicit, (1, weight), unless END starts from a list
    const bool implicit0 = !end || all;
    void *sa = nullptr, *sb = nullptr;
    GG_TRY(ctx->dev_alloc(&sa, st_bytes));
    if (k_max > 1 || !implicit0) GG_TRY(ctx->dev_alloc(&sb, st_bytes));  // (an explicit level 0 is a state of its own)
    const void *cur = nullptr;
    if (!implicit0) {
      if (weighted)
        GG_LAUNCH(ctx, "agg_seed_state", k_agg_seed_state, vgrid, dim3(256), 0, (const unsigned long long *)mult,
                  (const int64_t *)w_dev, V, (AggState *)sa);
      else
        GG_HIP(hipMemcpyAsync(sa, mult, V * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
      cur = sa;
    }
    const unsigned long long *final_mult = (!end && !all) ? mult : nullptr;
    uint64_t passes = 0;
    for (int h = 1; h <= k_max; h++) {
      void *nxt = cur == sa ? sb : sa;
      if (h == 1 && implicit0) {
        if (weighted) {
          GG_TRY(agg_pull<FORM_ONES>(ctx, p, w_dev, nxt));
          passes++;
        } else {
          GG_LAUNCH(ctx, "agg_rowlen", k_agg_rowlen, vgrid, dim3(256), 0, p.off, V, (uint64_t *)nxt);
        }
      } else {
        if (weighted)
          GG_TRY(agg_pull<FORM_STATE>(ctx, p, cur, nxt));
        else
          GG_TRY(agg_pull<FORM_COUNT>(ctx, p, cur, nxt));
        passes++;
      }
      cur = nxt;
      if (h < k_min) continue;
      GG_LAUNCH(ctx, "agg_flag", k_agg_flag, vgrid, dim3(256), 0, cur, (int)weighted, final_mult, V, flag,
                (unsigned long long *)(d_walks + h));
      GG_TRY(scan_exclusive_u32(ctx, flag, flag, V, d_groups + h));
      if (res) {
        // V entries per column: a level has at most V groups, and their number stays on the device until the call's
        // one read-back
        GG_TRY(alloc_kept_columns(ctx, res->cols[h], 4, V));
        GG_LAUNCH(ctx, "agg_write", k_agg_write, vgrid, dim3(256), 0, cur, (int)weighted, final_mult, V,
                  (const uint32_t *)flag, (const int64_t *)csr->vid, res->cols[h][0], res->cols[h][1], res->cols[h][2],
                  res->cols[h][3]);
      }
    }
    uint64_t hw[2 * (GG_MAX_HOPS + 1)];
    GG_TRY(read_back(ctx, {{words, sizeof(hw), hw}}));
    for (int h = k_min; h <= k_max; h++) {
      if (res) res->rows[h] = hw[h];
      if (stats) stats->groups[h] = hw[h], stats->walks[h] = hw[GG_MAX_HOPS + 1 + h];
    }
    if (stats) stats->entries_pulled = passes * E;
  }
  if (out_result) *out_result = res.release();
  return GG_OK;
}

extern "C" int gg_khop_aggregate_rows(const gg_result *res, int hops, uint64_t *n_rows) {
  if (!res || !n_rows) return GG_ERR_INVALID_ARG;
  GG_TRY(expect_kind(res, ResultKind::AGGREGATE, "gg_khop_aggregate_rows"));
  if (hops < res->k_min || hops > res->k_max) return GG_ERR_INVALID_ARG;
  *n_rows = res->rows[hops];
  return GG_OK;
}

extern "C" int gg_khop_aggregate_fetch(const gg_result *res, int hops, uint64_t offset, uint32_t max_rows,
                                       int64_t *vertex_id, uint64_t *walks, uint64_t *sum_lo, int64_t *sum_hi,
                                       uint32_t *n_out) {
  if (!res || !n_out || !vertex_id || !walks) return GG_ERR_INVALID_ARG;
  GG_TRY(expect_kind(res, ResultKind::AGGREGATE, "gg_khop_aggregate_fetch"));
  if (hops < res->k_min || hops > res->k_max) return GG_ERR_INVALID_ARG;
  int64_t *const *col = res->cols[hops];
  return fetch_slice(res->ctx, res->rows[hops], offset, max_rows,
                     {{vertex_id, col[0]}, {walks, col[1]}, {sum_lo, col[2]}, {sum_hi, col[3]}}, n_out);
}

extern "C" int gg_debug_aggregate_long_row(gg_ctx *ctx, uint32_t entries) {
  if (!ctx) return GG_ERR_INVALID_ARG;
  ctx->agg_long_row = entries;
  return GG_OK;
}
