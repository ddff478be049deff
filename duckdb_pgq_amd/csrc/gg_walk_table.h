// gg_walk_table.h — what the operators over the rows of a materialised walk table share around their kernels: the argument
// checks, the id dictionary and the value column as kernel arguments, the result's kept columns, the split of a launch, and
// the wavefront pieces of the two GROUP BY kernels.  Inline host functions and __device__
// __forceinline__ functions only: no kernel lives here, so a translation unit grows by nothing it does not call.
//
// The checks are small on purpose.  When a call has two faults it is answered with the code of the check that comes first,
// so the ORDER of an entry point's checks is behaviour (tests/test_gpu_walk_row_refusals.py), and every entry point calls
// the pieces in the order it always had; nothing here fixes one order for all of them.  Each takes the caller's name.
#pragma once
#include "gg_internal.h"

namespace gg {

// ---- checks ----------------------------------------------------------------------------------------------------------
// a NULL context or result, a result of another context
inline int result_arg(const char *fn, const gg_ctx *ctx, const gg_result *res) {
  if (ctx && res && res->ctx == ctx) return GG_OK;
  set_error("%s: bad context / result argument", fn);
  return GG_ERR_INVALID_ARG;
}

// What a result that holds no walk tables is answered with.  Every entry point keeps the rule it was born with
// (tests/test_gpu_result_kinds.py pins them): EXPECT is expect_kind's, which tells older kinds from younger ones.
enum class KindRule { STATE, INVALID_ARG, EXPECT };
inline int walk_kind_arg(const char *fn, const gg_result *res, KindRule rule) {
  if (rule == KindRule::EXPECT) return expect_kind(res, ResultKind::TABLES, fn);
  if (res->kind == ResultKind::TABLES) return GG_OK;
  set_error("%s: the result has no fixed-length table: it holds %s", fn, KIND_NAMES[(int)res->kind].holds);
  return rule == KindRule::STATE ? GG_ERR_STATE : GG_ERR_INVALID_ARG;
}

// `hops` is a level of the result and at most max_hops
inline int hops_arg(const char *fn, const gg_result *res, int hops, int max_hops = GG_MAX_HOPS) {
  if (hops >= res->k_min && hops <= res->k_max && hops >= 0 && hops <= max_hops) return GG_OK;
  set_error("%s: hops %d outside the result's range [%d, %d] or above %d", fn, hops, res->k_min, res->k_max, max_hops);
  return GG_ERR_INVALID_ARG;
}

// the three above, for an entry point that has nothing in between
inline int walk_table_arg(const char *fn, const gg_ctx *ctx, const gg_result *res, int hops, KindRule rule,
                          int max_hops = GG_MAX_HOPS) {
  GG_TRY(result_arg(fn, ctx, res));
  GG_TRY(walk_kind_arg(fn, res, rule));
  return hops_arg(fn, res, hops, max_hops);
}

// a NULL CSR, a CSR of another context
inline int csr_arg(const char *fn, const gg_ctx *ctx, const gg_csr *csr) {
  if (csr && csr->ctx == ctx) return GG_OK;
  set_error("%s: bad csr argument", fn);
  return GG_ERR_INVALID_ARG;
}
// a shard; `role` says what the CSR was to be: "the condition graph", "the joined table", ...
inline int whole_csr(const char *fn, const gg_csr *csr, const char *role) {
  if (csr->n_parts <= 1) return GG_OK;
  set_error("%s: a CSR shard (gg_csr_build_shard) cannot be %s", fn, role);
  return GG_ERR_STATE;
}
inline int whole_csr_arg(const char *fn, const gg_ctx *ctx, const gg_csr *csr, const char *role) {
  GG_TRY(csr_arg(fn, ctx, csr));
  return whole_csr(fn, csr, role);
}

// a column index outside lo..hops (lo is 0, or -1 where "none" is allowed)
inline int column_arg(const char *fn, const char *what, int col, int lo, int hops) {
  if (col >= lo && col <= hops) return GG_OK;
  set_error("%s: %s column %d outside %d..%d", fn, what, col, lo, hops);
  return GG_ERR_INVALID_ARG;
}

// table `hops` has rows but not the id columns cols[0..n) (cols NULL: the columns 0..n-1); negative entries are "none"
inline int id_columns_present(const char *fn, const gg_result *res, int hops, const int *cols, int n) {
  if (!res->rows[hops]) return GG_OK;
  for (int j = 0; j < n; j++) {
    const int c = cols ? cols[j] : j;
    if (c >= 0 && !res->cols[hops][c]) {
      set_error("%s: table %d of the result has rows but no id columns", fn, hops);
      return GG_ERR_STATE;
    }
  }
  return GG_OK;
}

// table `hops` carries the edge columns e1..e_hops of its walks
inline bool walk_edge_columns(const gg_result *res, int hops) {
  bool e = hops > 0;
  for (int c = 0; c < hops; c++) e = e && res->ecols[hops][c];
  return e;
}

// ---- the id dictionary of a CSR as a kernel argument -------------------------------------------------------------------
struct DictView {
  const HtSlot *ht;  // null: the CSR has no vertex (or the caller found nothing to look up): no cell is a vertex
  uint64_t cap;
  int64_t min_idx;
  // dense index of `key`, INVALID_U32 if it is no vertex; ht must not be null
  __device__ __forceinline__ uint32_t lookup(int64_t key) const { return ht_lookup(ht, cap, min_idx, key); }
};

// fills the dictionary on first use (ensure_ht); a CSR without a vertex leaves ht null and launches nothing
inline int dict_view(gg_ctx *ctx, const gg_csr *csr, DictView *d) {
  *d = DictView{nullptr, 0, -1};
  if (!csr->V) return GG_OK;
  GG_TRY(ensure_ht(ctx, const_cast<gg_csr *>(csr)));
  *d = DictView{csr->ht, csr->ht_cap, csr->ht_min_idx};
  return GG_OK;
}

// ---- the value of a row ------------------------------------------------------------------------------------------------
// The cell of the value column looked up in the value table's dictionary; the row has the value values[d] iff the cell is
// a vertex d and d's valid bit is set.
struct ValueColumn {
  const int64_t *cells;   // the value column's cells
  DictView dict;          // ht null: no row has a value
  const int64_t *values;  // device, V entries
  const uint64_t *valid;  // device, ceil(V / 64) words; null: every vertex has a value
};

__device__ __forceinline__ bool row_value(const ValueColumn &v, uint64_t r, int64_t &x) {
  if (!v.dict.ht) return false;
  const uint32_t d = v.dict.lookup(v.cells[r]);
  // (d < V: values has V entries and valid ceil(V / 64) words)
  if (d == INVALID_U32 || (v.valid && !((v.valid[d >> 6] >> (d & 63)) & 1ull))) return false;
  x = v.values[d];
  return true;
}

// The view over `cells` and csr's dictionary, with `values` and `valid` (nullable) copied into pool blocks.  Both are
// caller memory and the copies are only enqueued: every entry point that calls this reaches a read_back / sync_checked
// before it returns, so they have been read by then.
inline int value_column(gg_ctx *ctx, const gg_csr *csr, const int64_t *cells, const int64_t *values, const uint64_t *valid,
                        ValueColumn *v) {
  *v = ValueColumn{cells, {}, nullptr, nullptr};
  GG_TRY(dict_view(ctx, csr, &v->dict));
  const uint64_t V = csr->V;
  if (!V) return GG_OK;
  int64_t *v_dev = nullptr;
  GG_TRY(ctx->dev_alloc((void **)&v_dev, V * sizeof(int64_t)));
  GG_HIP(hipMemcpyAsync(v_dev, values, V * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
  v->values = v_dev;
  if (valid) {
    uint64_t *b_dev = nullptr;
    const size_t bytes = ((V + 63) / 64) * sizeof(uint64_t);
    GG_TRY(ctx->dev_alloc((void **)&b_dev, bytes));
    GG_HIP(hipMemcpyAsync(b_dev, valid, bytes, hipMemcpyHostToDevice, ctx->stream));
    v->valid = b_dev;
  }
  return GG_OK;
}

// ---- result columns and launches -----------------------------------------------------------------------------------------
// cols[0..n): pool blocks of `rows` int64 cells each that outlive the call (they belong to the result under construction)
inline int alloc_kept_columns(gg_ctx *ctx, int64_t **cols, int n, uint64_t rows) {
  for (int c = 0; c < n; c++) {
    GG_TRY(ctx->dev_alloc((void **)&cols[c], rows * sizeof(int64_t)));
    ctx->keep(cols[c]);
  }
  return GG_OK;
}

constexpr uint64_t MAX_LAUNCH_GROUPS = 0xFFFFFFFFull / 256;  // workgroups of 256 per launch: GG_LAUNCH refuses 2^32 threads

// f(g0, ng) for consecutive pieces [g0, g0 + ng) of n_groups workgroups, each at most gg_debug_max_grid_tiles and
// MAX_LAUNCH_GROUPS long, like the expansion and triangle kernels; stops at the first piece that does not return GG_OK
template <typename F>
int split_groups(const gg_ctx *ctx, uint64_t n_groups, F f) {
  const uint64_t per = ctx->max_grid_tiles && ctx->max_grid_tiles < MAX_LAUNCH_GROUPS ? ctx->max_grid_tiles : MAX_LAUNCH_GROUPS;
  for (uint64_t g0 = 0; g0 < n_groups; g0 += per) GG_TRY(f(g0, n_groups - g0 < per ? n_groups - g0 : per));
  return GG_OK;
}

// ---- wavefront pieces of the GROUP BY kernels (gg_group.hip argues why the carries are order-free) ----------------------
// (lo, hi) += (blo, bhi) mod 2^128
__device__ __forceinline__ void add128(uint64_t &lo, uint64_t &hi, uint64_t blo, uint64_t bhi) {
  lo += blo;
  hi += bhi + (uint64_t)(lo < blo);
}

// heads: the ballot of the lanes that head a run of adjacent equal lanes; one past the last lane of `lane`'s run
__device__ __forceinline__ int run_end(uint64_t heads, int lane) {
  const uint64_t after = lane == 63 ? 0 : heads >> (lane + 1);
  return after ? lane + 1 + __builtin_ctzll(after) : 64;
}

// the cell pair (*lo_cell, *hi_cell) += (lo, hi) mod 2^128: the low word by a returning atomic, its carry with the high
// word.  The cells are LDS words or global cells: inlined, each call compiles to the atomics of its own address space.
__device__ __forceinline__ void atomic_add128(unsigned long long *lo_cell, unsigned long long *hi_cell,
                                              unsigned long long lo, unsigned long long hi) {
  const unsigned long long old = atomicAdd(lo_cell, lo);
  atomicAdd(hi_cell, hi + (unsigned long long)(old + lo < lo));
}

}  // namespace gg
