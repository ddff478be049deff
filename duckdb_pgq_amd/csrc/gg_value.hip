// gg_value.hip — a value predicate over the rows of a walk table, and the best n rows by that value.
//
// The LDBC statements carry a predicate on a payload column of the joined row and two of them end in an ORDER BY on it:
// `m_creationdate < :date ... ORDER BY m_creationdate DESC, m_messageid ASC LIMIT 20`
// (benchmark/ldbc/queries/interactive-complex-2.sql:5,8-9, interactive-complex-9.sql:16-18), a half-open date range before
// the GROUP BY (interactive-complex-4.sql:9,18, interactive-complex-3.sql:20,27), `k2.k_person2id <> :person`
// (interactive-complex-9.sql:12).  The reference runs them as a filter inside the scan and PhysicalTopN
// (src/execution/operator/order/physical_top_n.cpp:238-293, 421-454) above the last hash join.  Here the joined rows are
// columns in HBM (gg_result_extend_edge), so both are done where they lie and only the answer crosses the link.
//
// The value of a row: the cell of value_col looked up in value_csr's id dictionary (ht_lookup, as gg_csr_lookup); the row
// has the value values[d] iff the cell is a vertex d and d's valid bit is set.  A row without a value passes nothing.
//   k_value_probe   one thread per row, striding by workgroups of 256 rows: the cell, one dictionary probe, the value and
//                   the valid word; the row's pass flag is one bit of a 64-row mask word — the wavefront's __ballot, stored
//                   by lane 0 — and the valued and passing rows are counted per wavefront.  For the top it also writes the
//                   value to an 8 B/row scratch column, so the digit passes never probe the dictionary again.
// Filter (gg_result_filter_value), count, scan, write (gg_rows.h, shared with gg_distinct.hip):
//   k_value_groups  one thread per group of 256 rows: the popcount of its four mask words
//   scan            exclusive prefix of the groups' rows
//   k_value_write   a row's place is the group's prefix + the popcounts of the group's mask words below its wavefront +
//                   the popcount of its own word below its lane: no LDS, no barrier.  It copies the hops + 1 id cells and
//                   the edge cells; the kept lanes of a wavefront write consecutive cells of every column, in input order,
//                   at the same places on every run.
// Top (gg_result_top_rows): the 192-bit key of gg_top.h is (value with the sign bit flipped, complemented if descending;
// tie id with the sign bit flipped; row number), live rows are those whose mask bit is set, and the selection, the
// compaction and the two sort routes are gg_top.h's.  The row number makes the key unique among duplicate rows.  Digit
// passes over bytes that are zero in every key are not run: the row number has ceil(bits_for(rows) / 8) bytes, the tie word
// none without a tie column.  The survivors come out of the selection in input order and the sorts are stable, so the global
// route never sorts by the row number at all.  The number of candidates stays on the device until the call's one
// read_back: the rank to select is min(n, candidates) there, the buffers are sized by min(n, rows) here.
//   k_value_gather  id and edge cells through the permutation into the result columns
// Bytes per row (model): probe 8 B cell + one 16-byte slot + 8 B value + 1/8 B valid + 1/8 B mask (+ 8 B scratch for the
// top); write 1/8 B mask + 8 (columns) B read per kept row + 8 (columns) B written; a digit pass before compaction 1/8 B
// mask + 8 B per key word it needs for rows that are live, after it 4 B list entry + the same, gathered.
#include "gg_internal.h"
#include "gg_rows.h"
#include "gg_top.h"

using namespace gg;

namespace gg {
namespace {

struct ProbeArgs {
  ValueColumn v;  // the value of a row (gg_walk_table.h)
  uint64_t n_rows;
  int64_t lo, hi;
  int negate;
  uint64_t *mask;         // ceil(n_rows / 64) words
  int64_t *xs;            // null: not wanted
  unsigned long long *counts;  // [0] rows with a value, [1] rows that pass
};

// Workgroup g owns rows [256 g, 256 g + 256) and wavefront w of it mask word 4 g + w; the grid strides over the groups.
__global__ __launch_bounds__(256) void k_value_probe(ProbeArgs a) {
  const int lane = threadIdx.x & 63;
  const uint64_t groups = (a.n_rows + 255) / 256;
  uint64_t valued = 0, passed = 0;  // (uniform over the wavefront)
  for (uint64_t g = blockIdx.x; g < groups; g += gridDim.x) {
    const uint64_t r = g * 256 + threadIdx.x;
    bool has = false, pass = false;
    int64_t x = 0;
    if (r < a.n_rows && row_value(a.v, r, x)) {
      has = true;
      const bool in = a.lo <= x && x <= a.hi;
      pass = in != (a.negate != 0);
    }
    if (a.xs && r < a.n_rows) a.xs[r] = x;
    const uint64_t hm = __ballot(has), pm = __ballot(pass);
    valued += (uint64_t)__popcll(hm), passed += (uint64_t)__popcll(pm);
    if (lane == 0 && (r & ~63ull) < a.n_rows) a.mask[r >> 6] = pm;  // (r >> 6 < ceil(n_rows / 64))
  }
  if (lane == 0) {
    if (valued) atomicAdd(&a.counts[0], (unsigned long long)valued);
    if (passed) atomicAdd(&a.counts[1], (unsigned long long)passed);
  }
}

struct ValueKeys {  // the key source of gg_top.h: the rows' values, the tie column (null: none) and the pass mask
  const int64_t *xs, *tie;
  const uint64_t *mask;
  int desc;

  template <int NEED>
  __device__ __forceinline__ Key key(uint64_t i) const {
    Key k{0, 0, 0};
    k.w2 = (uint64_t)xs[i] ^ (1ull << 63);
    if (desc) k.w2 = ~k.w2;
    if (NEED <= 1 && tie) k.w1 = (uint64_t)tie[i] ^ (1ull << 63);
    if (NEED == 0) k.w0 = i;
    return k;
  }
  __device__ __forceinline__ bool live(uint64_t i) const { return (mask[i >> 6] >> (i & 63)) & 1ull; }
};

// out column c, row j = in column c, row perm[j], for the first min(m, *m_dev) entries of perm; c = blockIdx.y (a column
// per grid row: two pointers in scalar registers, not 2 x VAL_MAX_COLS, at 4 B of perm read again per cell)
__global__ __launch_bounds__(256) void k_value_gather(ValIn in, const uint32_t *__restrict__ perm, uint64_t m,
                                                      const uint64_t *__restrict__ m_dev, ValOut out) {
  const uint64_t have = *m_dev < m ? *m_dev : m;
  const int64_t *__restrict__ src = in.c[blockIdx.y];
  int64_t *__restrict__ dst = out.c[blockIdx.y];
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < have; j += (uint64_t)gridDim.x * blockDim.x)
    dst[j] = src[perm[j]];  // (a row number < n_rows)
}

// the checks both entry points share; *edges: the input carries walk edge columns e1..e_hops
int value_check(const char *fn, gg_ctx *ctx, const gg_result *res, int hops, int value_col, const gg_csr *csr,
                const int64_t *values, int mode, bool *edges) {
  GG_TRY(result_arg(fn, ctx, res));
  if (!values) {
    set_error("%s: NULL values", fn);
    return GG_ERR_INVALID_ARG;
  }
  GG_TRY(whole_csr_arg(fn, ctx, csr, "the values' table"));
  GG_TRY(walk_kind_arg(fn, res, KindRule::STATE));
  GG_TRY(hops_arg(fn, res, hops));
  GG_TRY(column_arg(fn, "value", value_col, 0, hops));
  if (mode != GG_VALUE_IN && mode != GG_VALUE_NOT_IN) {
    set_error("%s: mode %d (0: in the range, 1: outside it)", fn, mode);
    return GG_ERR_INVALID_ARG;
  }
  GG_TRY(id_columns_present(fn, res, hops, nullptr, hops + 1));
  // (a triangle table's e1..e3 are no walk edge columns: dropped, as by every filter)
  *edges = !res->tri_edges && walk_edge_columns(res, hops);
  return GG_OK;
}

// uploads the value column and enqueues the probe over table `hops`: *mask, *xs (if want_xs) and *counts from the pool
int value_probe(gg_ctx *ctx, const gg_result *res, int hops, int value_col, gg_csr *csr, const int64_t *values,
                const uint64_t *valid, int64_t lo, int64_t hi, int mode, bool want_xs, uint64_t **mask, int64_t **xs,
                unsigned long long **counts) {
  hipStream_t st = ctx->stream;
  const uint64_t n_rows = res->rows[hops], n_words = (n_rows + 63) / 64;
  ProbeArgs a{};
  GG_TRY(value_column(ctx, csr, res->cols[hops][value_col], values, valid, &a.v));
  a.n_rows = n_rows;
  a.lo = lo, a.hi = hi, a.negate = mode == GG_VALUE_NOT_IN;
  GG_TRY(ctx->dev_alloc((void **)&a.mask, n_words * sizeof(uint64_t)));
  if (want_xs) GG_TRY(ctx->dev_alloc((void **)&a.xs, n_rows * sizeof(int64_t)));
  GG_TRY(ctx->dev_alloc((void **)&a.counts, 2 * sizeof(unsigned long long)));
  GG_HIP(hipMemsetAsync(a.counts, 0, 2 * sizeof(unsigned long long), st));
  dim3 grid = stride_grid(ctx, n_rows);
  if (ctx->max_grid_tiles && ctx->max_grid_tiles < grid.x) grid.x = (unsigned)ctx->max_grid_tiles;
  GG_LAUNCH(ctx, "k_value_probe", k_value_probe, grid, dim3(256), 0, a);
  *mask = a.mask, *xs = a.xs, *counts = a.counts;
  return GG_OK;
}

int value_columns(const gg_result *res, int hops, bool edges, ValIn *in) {
  int n = 0;
  for (int c = 0; c <= hops; c++) in->c[n++] = res->cols[hops][c];
  if (edges)
    for (int c = 0; c < hops; c++) in->c[n++] = res->ecols[hops][c];
  return n;
}

// the kept columns of `rows` rows each for table hops of o, in value_columns' order
int value_alloc_out(gg_ctx *ctx, gg_result *o, int hops, bool edges, uint64_t rows, ValOut *out) {
  int n = 0;
  GG_TRY(alloc_kept_columns(ctx, o->cols[hops], hops + 1, rows));
  for (int c = 0; c <= hops; c++) out->c[n++] = o->cols[hops][c];
  if (edges) {
    GG_TRY(alloc_kept_columns(ctx, o->ecols[hops], hops, rows));
    for (int c = 0; c < hops; c++) out->c[n++] = o->ecols[hops][c];
  }
  return GG_OK;
}

}  // namespace
}  // namespace gg

extern "C" int gg_result_filter_value(gg_ctx *ctx, const gg_result *res, int hops, int value_col, const gg_csr *value_csr,
                                      const int64_t *values, const uint64_t *valid, int64_t lo, int64_t hi, int mode,
                                      int materialise, gg_value_filter_stats *stats, gg_result **out_result) {
  if (out_result) *out_result = nullptr;
  if (stats) memset(stats, 0, sizeof(*stats));
  bool edges = false;
  GG_TRY(value_check("gg_result_filter_value", ctx, res, hops, value_col, value_csr, values, mode, &edges));
  if (materialise && !out_result) {
    set_error("gg_result_filter_value: materialise without out_result");
    return GG_ERR_INVALID_ARG;
  }
  ApiScope scope(ctx);
  GG_HIP(hipSetDevice(ctx->device));
  const uint64_t n_rows = res->rows[hops], n_words = (n_rows + 63) / 64;
  ResultOwner o;
  if (materialise) o = make_result(ctx, ResultKind::TABLES, hops, hops);
  uint64_t counts_host[2] = {0, 0}, total = 0;  // rows with a value, rows that pass
  if (n_rows) {
    uint64_t *mask = nullptr;
    int64_t *xs = nullptr;
    unsigned long long *counts = nullptr;
    GG_TRY(value_probe(ctx, res, hops, value_col, const_cast<gg_csr *>(value_csr), values, valid, lo, hi, mode, false, &mask,
                       &xs, &counts));
    if (!materialise) {
      GG_TRY(read_back(ctx, {{counts, sizeof(counts_host), counts_host}}));
      total = counts_host[1];
    } else {
      uint64_t *group = nullptr;
      GG_TRY(mask_prefix(ctx, mask, n_rows, {{counts, sizeof(counts_host), counts_host}}, &group, &total));
      if (total >= (1ull << 32)) {
        set_error("gg_result_filter_value: %llu rows to materialise (2^32 or more); count them, or filter a smaller table",
                  (unsigned long long)total);
        return GG_ERR_TOO_LARGE;
      }
      if (total) {
        ValIn in{};
        ValOut out{};
        const int ncols = value_columns(res, hops, edges, &in);
        GG_TRY(value_alloc_out(ctx, o.get(), hops, edges, total, &out));
        GG_TRY(value_write_launch(ctx, in, ncols, n_rows, mask, n_words, group, total, out));
        GG_TRY(sync_checked(ctx));
      }
    }
  }
  if (stats) stats->rows_in = n_rows, stats->rows_valued = counts_host[0], stats->rows_out = total;
  if (materialise) {
    o->rows[hops] = total;
    *out_result = o.release();
  }
  return GG_OK;
}

extern "C" int gg_result_top_rows(gg_ctx *ctx, const gg_result *res, int hops, int value_col, const gg_csr *value_csr,
                                  const int64_t *values, const uint64_t *valid, int64_t lo, int64_t hi, int mode,
                                  int descending, int tie_col, uint64_t n, gg_value_top_stats *stats,
                                  gg_result **out_result) {
  if (out_result) *out_result = nullptr;
  if (stats) memset(stats, 0, sizeof(*stats));
  bool edges = false;
  GG_TRY(value_check("gg_result_top_rows", ctx, res, hops, value_col, value_csr, values, mode, &edges));
  if (!out_result) {
    set_error("gg_result_top_rows: NULL out_result");
    return GG_ERR_INVALID_ARG;
  }
  if (tie_col < -1 || tie_col > hops) {
    set_error("gg_result_top_rows: tie column %d outside -1..%d", tie_col, hops);
    return GG_ERR_INVALID_ARG;
  }
  ApiScope scope(ctx);
  GG_HIP(hipSetDevice(ctx->device));
  const uint64_t N = res->rows[hops], bound = n < N ? n : N;  // (min(n, candidates) <= bound)
  if (N >= (1ull << 32)) {
    set_error("gg_result_top_rows: a table of %llu rows (2^32 or more); filter it first (gg_result_filter_value)",
              (unsigned long long)N);
    return GG_ERR_TOO_LARGE;
  }
  ResultOwner o = make_result(ctx, ResultKind::TABLES, hops, hops);
  uint64_t counts_host[2] = {0, 0}, hw[3] = {0, 0, 0};  // valued, candidates; passes run, (unused), survivors
  int route = 0;
  if (N) {
    hipStream_t st = ctx->stream;
    uint64_t *mask = nullptr;
    int64_t *xs = nullptr;
    unsigned long long *counts = nullptr;
    GG_TRY(value_probe(ctx, res, hops, value_col, const_cast<gg_csr *>(value_csr), values, valid, lo, hi, mode, bound != 0,
                       &mask, &xs, &counts));
    if (bound == 0) {
      GG_TRY(read_back(ctx, {{counts, sizeof(counts_host), counts_host}}));
    } else {
      uint64_t *w = nullptr;
      GG_TRY(ctx->dev_alloc((void **)&w, TW_WORDS * sizeof(uint64_t)));
      GG_HIP(hipMemsetAsync(w, 0, TW_WORDS * sizeof(uint64_t), st));
      unsigned long long *listed = nullptr;
      GG_TRY(ctx->dev_alloc((void **)&listed, sizeof(unsigned long long)));
      GG_HIP(hipMemsetAsync(listed, 0, sizeof(unsigned long long), st));
      ValueKeys c{xs, tie_col >= 0 ? res->cols[hops][tie_col] : nullptr, mask, descending != 0};
      TopPlan plan;
      for (int b = 23; b >= 16; b--) plan.bytes[plan.n_bytes++] = b;
      if (c.tie)
        for (int b = 15; b >= 8; b--) plan.bytes[plan.n_bytes++] = b;
      for (int b = (bits_for(N) + 7) / 8 - 1; b >= 0; b--) plan.bytes[plan.n_bytes++] = b;
      // pieces 0..1 are row-number bits, which the stable passes never need; piece 2 holds the tie word's low byte and
      // piece 5 its top byte next to the value's low two
      for (int ch = c.tie ? 2 : 5; ch < 8; ch++) plan.chunks[plan.n_chunks++] = ch;
      const uint32_t *ordered = nullptr;
      GG_TRY(top_select_order(ctx, c, N, bound, (const uint64_t *)(counts + 1), plan, ctx->val_top_route, ctx->val_top_floor, w,
                              listed, &ordered, &route));
      ValIn in{};
      ValOut out{};
      const int ncols = value_columns(res, hops, edges, &in);
      GG_TRY(value_alloc_out(ctx, o.get(), hops, edges, bound, &out));
      dim3 ggrid = stride_grid(ctx, bound);
      ggrid.y = (unsigned)ncols;
      GG_LAUNCH(ctx, "k_value_gather", k_value_gather, ggrid, dim3(256), 0, in, ordered, bound,
                (const uint64_t *)(w + TW_NSURV), out);
      GG_TRY(read_back(ctx, {{w + TW_PASSES, sizeof(hw), hw}, {counts, sizeof(counts_host), counts_host}}));
      const uint64_t m = n < counts_host[1] ? n : counts_host[1];
      if (hw[2] != m) {
        set_error("internal: gg_result_top_rows selected %llu rows, not %llu", (unsigned long long)hw[2],
                  (unsigned long long)m);
        return GG_ERR_STATE;
      }
      if (m < 2) route = 0;
    }
  }
  const uint64_t m = n < counts_host[1] ? n : counts_host[1];
  if (stats) {
    stats->rows_in = N, stats->rows_valued = counts_host[0], stats->candidates = counts_host[1], stats->rows_out = m;
    stats->select_passes = (uint32_t)hw[0], stats->sort_route = (uint32_t)route;
  }
  o->rows[hops] = m;
  *out_result = o.release();
  return GG_OK;
}

extern "C" int gg_debug_value_top(gg_ctx *ctx, int sort_route, uint32_t candidate_floor) {
  if (!ctx || sort_route < 0 || sort_route > 2) return GG_ERR_INVALID_ARG;
  ctx->val_top_route = sort_route;
  ctx->val_top_floor = candidate_floor;
  return GG_OK;
}
