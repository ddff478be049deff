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
//   gg_top.h        the radix select (k_top_hist / k_top_pick / k_top_compact), the survivors' permutation (k_top_count /
//                   scan / k_top_place) and the two sort routes (k_top_sort_lds; k_top_chunk + sort_pairs_by_key), shared
//                   with gg_value.hip; TopCols below is their key source, and every group is live
//   k_top_gather    (id, walks, lo, hi) through the permutation into the exact-size result columns
// The host enqueues every pass; nothing is read back until the call's one read_back (passes run, ids unknown, survivors, and
// the length of the list if one was written: gg_debug_aggregate_top_listed).
// Bytes per pass (model): before compaction N rows x (8 B per key word the pass needs: 8 in the top word, 16 in the
// middle one, 24 with the id; + 8 B with a bias); after it candidates x (4 B list entry + the same, gathered).
#include "gg_internal.h"
#include "gg_top.h"

using namespace gg;

namespace gg {
namespace {

struct TopCols {  // the level's columns, the gathered bias (null: none) and the order: the key source of gg_top.h
  const int64_t *id, *walks, *lo, *hi, *brow;
  int by_walks, desc;

  // NEED: the lowest key word the caller looks at (words below it are left 0 and their columns unread)
  template <int NEED>
  __device__ __forceinline__ Key key(uint64_t i) const {
    Key k{0, 0, 0};
    if (by_walks) {
      if (NEED <= 1) k.w1 = (uint64_t)walks[i];
      if (desc) k.w1 = ~k.w1;
    } else {
      uint64_t h = (uint64_t)hi[i], l = 0;
      if (NEED <= 1 || brow) l = (uint64_t)lo[i];
      if (brow) {  // + the sign-extended bias, mod 2^128
        const int64_t b = brow[i];
        const uint64_t s = l + (uint64_t)b;
        h += (uint64_t)(b >> 63) + (uint64_t)(s < l);
        l = s;
      }
      k.w2 = h ^ (1ull << 63);
      k.w1 = l;
      if (desc) k.w2 = ~k.w2, k.w1 = ~k.w1;
    }
    if (NEED == 0) k.w0 = (uint64_t)id[i] ^ (1ull << 63);
    return k;
  }
  __device__ __forceinline__ bool live(uint64_t) const { return true; }  // every group is a candidate
};

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

  TopPlan plan;  // (walks: the top word of every key is 0)
  for (int b = (by_walks ? 16 : 24) - 1; b >= 0; b--) plan.bytes[plan.n_bytes++] = b;
  for (int ch = 0; ch < (by_walks ? 6 : 8); ch++) plan.chunks[plan.n_chunks++] = ch;
  int route = 0;
  const uint32_t *ordered = nullptr;
  GG_TRY(top_select_order(ctx, c, N, m, nullptr, plan, ctx->agg_top_route, ctx->agg_top_floor, w, listed, &ordered, &route));
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
