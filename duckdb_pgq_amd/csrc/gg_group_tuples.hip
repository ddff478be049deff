// gg_group_tuples.hip — GROUP BY several columns of a materialised walk table: count(*), count(x), sum(x), min(x), max(x)
// per tuple of raw int64 cells, as a result of its own kind.
//
// The reference's LDBC statements group joined rows by more than one column, by cells that are vertices of no CSR, and
// under min and max: `GROUP BY m.friendid, t.t_name` under count(*) (benchmark/ldbc/queries/bi-10-shortestpath.sql:74),
// `min(hopCount) ... GROUP BY startPerson, friend` (bi-10-shortestpath.sql:28-30), `GROUP BY person1id, person2id` with a
// summed score (bi-14.sql:111), `max(l_creationdate) ... GROUP BY l_personid` (interactive-complex-7.sql:7-12).  There that
// is PhysicalHashAggregate (src/execution/operator/aggregate/physical_hash_aggregate.cpp:152-266).  gg_result_group_by
// (gg_group.hip) groups by ONE column whose cells are vertices of a CSR and forms count and sum only.
//
// The passes:
//   tuple table      gg_tuples.h's k_distinct_insert and k_distinct_flag, unchanged: every tuple owns one
//                    slot, the slot holds the tuple's first row q, and the mask flags the first rows.  gg_rows.h's
//                    k_value_groups and the scan give every 256-row group its exclusive prefix; after the scan the host
//                    knows `groups`, and a first row q has the RANK prefix[q / 256] + popcount of the mask bits below q in
//                    its group — its place in gg_result_distinct's output.
//   k_tuple_valued   only when no rows are asked for: counts the rows that have a value (stats->rows_valued).
//   k_tuple_init     the cells: min starts at INT64_MAX and max at INT64_MIN.
//   k_tuple_accum    one thread per input row, workgroups striding over groups of 256 rows exactly as the insert pass, so a
//                    row sits in the lane it sat in there.  Runs of equal tuples in adjacent lanes are found by the insert
//                    pass's comparison of the cells (NOT by a marker in slot_of: with combining on a non-head lane stored
//                    slot 0, which is a slot like any other); with combining off every row is its own run.  A run's count
//                    is its length; its valued count, its 128-bit sum, its min and its max are segmented suffix
//                    reductions by shuffles (gg_group.hip's add128 scheme).  The head lane alone reads its slot, the
//                    slot's row q and q's rank and adds to cell `rank`
//                      LDS     of the workgroup's private cells (LDS atomics); after its last tile the workgroup flushes
//                              every touched cell with one set of global atomics
//                      GLOBAL  of the global cells
//   k_tuple_write    the cells become six columns (rows, valued, sum low, sum high, min, max; min = max = 0 where valued
//                    == 0); the key columns are the first rows' cells at their rank: gg_rows.h's k_value_write.
// State is sized by the number of GROUPS, not of slots: a cell per slot would be 48 cap >= 96 bytes per input row to
// initialise and to scan for occupied slots.  That is why accumulation is not fused into the insert pass (a slot's rank
// is unknown until every row is in), and why the accumulate pass comes after a host synchronisation.
// The 128-bit sum from 64-bit atomics is gg_group.hip's: low word by a returning add, its carry added
// with the high word; order-free, and the same one level up at the flush.  min and max are signed 64-bit atomics, which
// are order-free as well.  Everything is integer addition mod 2^64 / 2^128 and integer min / max: both routes, every grid,
// every slot count and every arrival order give the same bits.
// Staleness: gg_tuples.h's insert pass reads slots that other workgroups write meanwhile, and gg_distinct.hip argues why
// a stale value is harmless there.  Here the plain loads of `tab`, `slot_of`, the mask and the prefixes come after a
// kernel boundary (and a host synchronisation) behind their last writer, so staleness does not arise.
// No unbounded loop but ht_lookup's (the id dictionary always has an empty slot); every cell index is checked against
// `groups` before it is used.
// Bytes per row (model), c key columns: 8 c B cells; valued form + 8 B value cell (unless it is a key column) + one
// 16-byte dictionary slot + 8 B value + 1/8 B valid; per run head 4 B slot number + one slot word + 8 B prefix + up to
// four mask words, and the atomics: 1 (count form) or up to 6 per run.  Per group: 8 / 48 B initialised, read once by
// the write pass, 8 c + 48 B (count form 8 c + 8 B) written; on the LDS route 8 / 48 B of global atomics per touched
// cell and workgroup.
#include "gg_internal.h"
#include "gg_rows.h"
#include "gg_tuples.h"

using namespace gg;

namespace gg {
namespace {

constexpr uint32_t TG_LDS_BYTES = 48 * 1024;  // gg_group.hip's budget: three workgroups share a CU's LDS
constexpr uint32_t TG_WG_PER_CU_LDS = 3, TG_WG_PER_CU_GLOBAL = 8;
constexpr int TG_KEYS_TABLE = 0, TG_AGG_TABLE = 1;  // where a TUPLE_GROUPS result keeps its columns (gg_internal.h)
constexpr int TG_AGG_COLS = 6;

struct TupleCell {  // the global state of a group in the valued form: 48 bytes
  unsigned long long rows, valued, lo, hi;
  long long mn, mx;
};

struct TupleArgs {
  DistinctArgs d;         // the key columns, the tuple table, slot_of, the mask and the combine flag of the insert pass
  const uint64_t *group;  // the exclusive prefix of the first rows per 256-row group
  uint64_t groups;
  ValueColumn v;          // the value of a row (gg_walk_table.h), as gg_value.hip's k_value_probe forms it
  unsigned long long *cnt;  // count form: groups u64
  TupleCell *cell;          // valued form: groups cells
};

// rows that have a value -> *valued
__global__ __launch_bounds__(256) void k_tuple_valued(ValueColumn v, uint64_t n_rows, unsigned long long *valued) {
  const uint64_t tiles = (n_rows + 255) / 256;
  uint64_t n = 0;  // (uniform over the wavefront)
  for (uint64_t g = blockIdx.x; g < tiles; g += gridDim.x) {
    const uint64_t r = g * 256 + threadIdx.x;
    int64_t x = 0;
    const bool has = r < n_rows && row_value(v, r, x);
    n += (uint64_t)__popcll(__ballot(has));
  }
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(valued, (unsigned long long)n);
}

__global__ __launch_bounds__(256) void k_tuple_init(TupleCell *cell, uint64_t groups) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < groups; i += (uint64_t)gridDim.x * blockDim.x)
    cell[i] = TupleCell{0, 0, 0, 0, INT64_MAX, INT64_MIN};
}

// LDS layout, indexed by rank: rows[G], then valued[G], lo[G], hi[G], min[G], max[G] in the valued form.
template <bool LDS, bool VALUED>
__global__ __launch_bounds__(256) void k_tuple_accum(TupleArgs A) {
  extern __shared__ __align__(16) unsigned long long s_cell[];
  const int lane = threadIdx.x & 63;
  const uint32_t G = (uint32_t)A.groups;  // (LDS route: groups <= 6144)
  if (LDS) {
    for (uint32_t i = threadIdx.x; i < G; i += 256) {
      s_cell[i] = 0;
      if (VALUED) {
        s_cell[G + i] = 0, s_cell[2 * G + i] = 0, s_cell[3 * G + i] = 0;
        s_cell[4 * G + i] = (unsigned long long)INT64_MAX, s_cell[5 * G + i] = (unsigned long long)INT64_MIN;
      }
    }
    __syncthreads();
  }
  const DistinctArgs &a = A.d;
  const uint64_t tiles = (a.n_rows + 255) / 256, n_words = (a.n_rows + 63) / 64;
  for (uint64_t g = blockIdx.x; g < tiles; g += gridDim.x) {
    const uint64_t r = g * 256 + threadIdx.x;
    const bool live = r < a.n_rows;
    bool same = true;  // as the row of the lane below: the insert pass's comparison
#pragma unroll
    for (int c = 0; c < DST_MAX_COLS; c++) {
      if (c < a.ncols) {  // (uniform: every lane shuffles)
        const int64_t mine = live ? a.c[c][r] : 0;
        const int64_t below = (int64_t)__shfl_up((unsigned long long)mine, 1, 64);
        same = same && below == mine;
      }
    }
    // lane l heads a run iff the insert pass made it probe; a lane past the table ends the run before it
    const uint64_t heads = __ballot(!live || !(a.combine && lane != 0 && same));
    const int end = run_end(heads, lane);  // one past the last lane of this lane's run
    uint64_t lo = 0, hi = 0;
    uint32_t nv = 0;
    int64_t mn = INT64_MAX, mx = INT64_MIN;
    if (VALUED) {
      int64_t x = 0;
      if (live && row_value(A.v, r, x)) lo = (uint64_t)x, hi = (uint64_t)(x >> 63), nv = 1, mn = x, mx = x;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {  // segmented suffix reductions: lane l ends with those of [l, end)
        const uint64_t blo = __shfl_down((unsigned long long)lo, d, 64), bhi = __shfl_down((unsigned long long)hi, d, 64);
        const uint32_t bnv = (uint32_t)__shfl_down((int)nv, d, 64);
        const int64_t bmn = (int64_t)__shfl_down((unsigned long long)mn, d, 64);
        const int64_t bmx = (int64_t)__shfl_down((unsigned long long)mx, d, 64);
        if (lane + d < end) {
          add128(lo, hi, blo, bhi);
          nv += bnv;
          mn = bmn < mn ? bmn : mn;
          mx = bmx > mx ? bmx : mx;
        }
      }
    }
    if (live && ((heads >> lane) & 1)) {
      const uint32_t s = a.slot_of[r];  // (< cap: the slot this lane's probe ended in)
      const uint32_t q = a.tab[s];      // the tuple's first row
      uint64_t rank = A.groups;
      if (q < a.n_rows) {  // (always: the slot holds a row of this tuple)
        const uint64_t qg = q >> 8;
        rank = A.group[qg];
        for (uint32_t k = 0; k < ((q >> 6) & 3u); k++) rank += (uint64_t)__popcll(mask_word(a.mask, n_words, 4 * qg + k));
        rank += (uint64_t)__popcll(mask_word(a.mask, n_words, q >> 6) & ((1ull << (q & 63)) - 1));
      }
      if (rank < A.groups) {  // (always: q is a first row, and the prefixes count the first rows)
        const unsigned long long cnt = (unsigned long long)(end - lane);
        if (LDS) {
          atomicAdd(&s_cell[rank], cnt);
          if (VALUED && nv) {
            atomicAdd(&s_cell[G + rank], (unsigned long long)nv);
            atomic_add128(&s_cell[2 * G + rank], &s_cell[3 * G + rank], lo, hi);
            atomicMin((long long *)&s_cell[4 * G + rank], (long long)mn);
            atomicMax((long long *)&s_cell[5 * G + rank], (long long)mx);
          }
        } else if (VALUED) {
          TupleCell *cell = &A.cell[rank];
          atomicAdd(&cell->rows, cnt);
          if (nv) {
            atomicAdd(&cell->valued, (unsigned long long)nv);
            atomic_add128(&cell->lo, &cell->hi, lo, hi);
            atomicMin(&cell->mn, (long long)mn);
            atomicMax(&cell->mx, (long long)mx);
          }
        } else {
          atomicAdd(&A.cnt[rank], cnt);
        }
      }
    }
  }
  if (LDS) {
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < G; k += 256) {
      const unsigned long long cnt = s_cell[k];
      if (!cnt) continue;  // (no row of this workgroup is in the group)
      if (VALUED) {
        TupleCell *cell = &A.cell[k];
        atomicAdd(&cell->rows, cnt);
        const unsigned long long nv = s_cell[G + k];
        if (nv) {
          atomicAdd(&cell->valued, nv);
          atomic_add128(&cell->lo, &cell->hi, s_cell[2 * G + k], s_cell[3 * G + k]);
          atomicMin(&cell->mn, (long long)s_cell[4 * G + k]);
          atomicMax(&cell->mx, (long long)s_cell[5 * G + k]);
        }
      } else {
        atomicAdd(&A.cnt[k], cnt);
      }
    }
  }
}

struct TupleOut {
  int64_t *c[TG_AGG_COLS];  // rows, valued, sum low, sum high, min, max (count form: c[0] alone)
};

// the cells as columns; sums[0] += the groups' valued rows, sums[1] += the groups' rows
__global__ __launch_bounds__(256) void k_tuple_write(const unsigned long long *__restrict__ cnt,
                                                     const TupleCell *__restrict__ cell, uint64_t groups, TupleOut out,
                                                     unsigned long long *__restrict__ sums) {
  uint64_t rows = 0, valued = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < groups; i += (uint64_t)gridDim.x * blockDim.x) {
    if (cell) {
      const TupleCell c = cell[i];
      out.c[0][i] = (int64_t)c.rows, out.c[1][i] = (int64_t)c.valued;
      out.c[2][i] = (int64_t)c.lo, out.c[3][i] = (int64_t)c.hi;
      out.c[4][i] = c.valued ? c.mn : 0, out.c[5][i] = c.valued ? c.mx : 0;
      rows += c.rows, valued += c.valued;
    } else {
      const unsigned long long c = cnt[i];
      out.c[0][i] = (int64_t)c;
      rows += c;
    }
  }
  rows = wave_reduce_add_u64(rows), valued = wave_reduce_add_u64(valued);
  if ((threadIdx.x & 63) == 0) {
    if (valued) atomicAdd(&sums[0], (unsigned long long)valued);
    if (rows) atomicAdd(&sums[1], (unsigned long long)rows);
  }
}

}  // namespace
}  // namespace gg

extern "C" int gg_result_group_tuples(gg_ctx *ctx, const gg_result *res, int hops, const int *cols, int n_cols,
                                      int value_col, const gg_csr *value_csr, const int64_t *values, const uint64_t *valid,
                                      gg_group_tuples_stats *stats, gg_result **out_result) {
  const char *fn = "gg_result_group_tuples";
  if (out_result) *out_result = nullptr;
  if (stats) memset(stats, 0, sizeof(*stats));
  GG_TRY(result_arg(fn, ctx, res));
  if (!cols) {
    set_error("%s: NULL cols", fn);
    return GG_ERR_INVALID_ARG;
  }
  GG_TRY(walk_kind_arg(fn, res, KindRule::EXPECT));
  if (!stats && !out_result) {
    set_error("%s: neither stats nor out_result is asked for", fn);
    return GG_ERR_INVALID_ARG;
  }
  GG_TRY(tuple_columns_check(fn, res, hops, cols, n_cols));
  const bool valued = value_col != -1;
  if (!valued && (value_csr || values || valid)) {
    set_error("%s: a value table, values or valid bits without a value column", fn);
    return GG_ERR_INVALID_ARG;
  }
  if (valued) {
    GG_TRY(column_arg(fn, "value", value_col, -1, hops));
    if (!values) {
      set_error("%s: NULL values", fn);
      return GG_ERR_INVALID_ARG;
    }
    GG_TRY(whole_csr_arg(fn, ctx, value_csr, "the values' table"));
    GG_TRY(id_columns_present(fn, res, hops, &value_col, 1));
  }
  const uint64_t n_rows = res->rows[hops], n_words = (n_rows + 63) / 64;
  ApiScope scope(ctx);
  GG_HIP(hipSetDevice(ctx->device));
  ResultOwner o;
  if (out_result) o = make_result(ctx, ResultKind::TUPLE_GROUPS, n_cols - 1, n_cols - 1);
  // probe steps, error, first rows; rows with a value (stats only); the groups' valued rows, the groups' rows (write pass)
  uint64_t words_host[6] = {0, 0, 0, 0, 0, 0}, groups = 0, cap = 0;
  uint32_t route = 0;
  if (n_rows) {
    hipStream_t st = ctx->stream;
    cap = tuple_slots(ctx, n_rows);
    TupleArgs A{};
    DistinctArgs &a = A.d;
    for (int j = 0; j < n_cols; j++) a.c[j] = res->cols[hops][cols[j]];
    a.ncols = n_cols;
    a.n_rows = n_rows;
    a.cap = cap;
    a.combine = ctx->distinct_combine != 1;
    GG_TRY(ctx->dev_alloc((void **)&a.tab, cap * sizeof(uint32_t)));
    GG_HIP(hipMemsetAsync(a.tab, 0xFF, cap * sizeof(uint32_t), st));
    GG_TRY(ctx->dev_alloc((void **)&a.slot_of, n_rows * sizeof(uint32_t)));
    GG_TRY(ctx->dev_alloc((void **)&a.mask, n_words * sizeof(uint64_t)));
    GG_TRY(ctx->dev_alloc((void **)&a.words, sizeof(words_host)));
    GG_HIP(hipMemsetAsync(a.words, 0, sizeof(words_host), st));
    if (valued) GG_TRY(value_column(ctx, value_csr, res->cols[hops][value_col], values, valid, &A.v));
    dim3 grid = stride_grid(ctx, n_rows);
    if (ctx->max_grid_tiles && ctx->max_grid_tiles < grid.x) grid.x = (unsigned)ctx->max_grid_tiles;
    GG_LAUNCH(ctx, "k_distinct_insert", k_distinct_insert, grid, dim3(256), 0, a);
    GG_LAUNCH(ctx, "k_distinct_flag", k_distinct_flag, grid, dim3(256), 0, a);
    if (valued && !o)
      GG_LAUNCH(ctx, "k_tuple_valued", k_tuple_valued, grid, dim3(256), 0, A.v, n_rows, a.words + 3);
    const uint64_t tiles = (n_rows + 255) / 256;
    uint64_t *group = nullptr;
    GG_TRY(mask_prefix(ctx, a.mask, n_rows, {{a.words, 4 * sizeof(uint64_t), words_host}}, &group, &groups));
    if (words_host[1]) {
      set_error("internal: %s found no slot for a row in a table of %llu slots for %llu rows", fn, (unsigned long long)cap,
                (unsigned long long)n_rows);
      return GG_ERR_STATE;
    }
    if (groups != words_host[2] || !groups) {
      set_error("internal: %s counted %llu first rows and flagged %llu", fn, (unsigned long long)groups,
                (unsigned long long)words_host[2]);
      return GG_ERR_STATE;
    }
    // the route: the workgroup-private cells wherever the groups fit them, unless the global cells are forced
    const size_t cell_bytes = valued ? sizeof(TupleCell) : sizeof(unsigned long long);
    uint64_t lds_groups = TG_LDS_BYTES / cell_bytes;
    if (ctx->tuple_lds_groups && ctx->tuple_lds_groups < lds_groups) lds_groups = ctx->tuple_lds_groups;
    route = ctx->tuple_route != 2 && groups <= lds_groups ? 1 : 2;
    if (o) {
      A.group = group;
      A.groups = groups;
      void *state = nullptr;
      GG_TRY(ctx->dev_alloc(&state, groups * cell_bytes));
      if (valued) {
        A.cell = (TupleCell *)state;
        GG_LAUNCH(ctx, "k_tuple_init", k_tuple_init, stride_grid(ctx, groups), dim3(256), 0, A.cell, groups);
      } else {
        A.cnt = (unsigned long long *)state;
        GG_HIP(hipMemsetAsync(state, 0, groups * cell_bytes, st));
      }
      uint64_t agrid = (uint64_t)ctx->num_cus * (route == 1 ? TG_WG_PER_CU_LDS : TG_WG_PER_CU_GLOBAL);
      if (ctx->max_grid_tiles && ctx->max_grid_tiles < agrid) agrid = ctx->max_grid_tiles;
      if (tiles < agrid) agrid = tiles;
      const size_t lds = route == 1 ? groups * cell_bytes : 0;  // (<= TG_LDS_BYTES)
      if (route == 1 && valued)
        GG_LAUNCH(ctx, "k_tuple_accum_lds_valued", (k_tuple_accum<true, true>), dim3((unsigned)agrid), dim3(256), lds, A);
      else if (route == 1)
        GG_LAUNCH(ctx, "k_tuple_accum_lds", (k_tuple_accum<true, false>), dim3((unsigned)agrid), dim3(256), lds, A);
      else if (valued)
        GG_LAUNCH(ctx, "k_tuple_accum_valued", (k_tuple_accum<false, true>), dim3((unsigned)agrid), dim3(256), 0, A);
      else
        GG_LAUNCH(ctx, "k_tuple_accum", (k_tuple_accum<false, false>), dim3((unsigned)agrid), dim3(256), 0, A);
      ValIn in{};
      ValOut keys{};
      GG_TRY(alloc_kept_columns(ctx, o->cols[TG_KEYS_TABLE], n_cols, groups));
      for (int j = 0; j < n_cols; j++) in.c[j] = a.c[j], keys.c[j] = o->cols[TG_KEYS_TABLE][j];
      GG_TRY(value_write_launch(ctx, in, n_cols, n_rows, a.mask, n_words, group, groups, keys));
      TupleOut out{};
      const int agg_cols = valued ? TG_AGG_COLS : 1;
      GG_TRY(alloc_kept_columns(ctx, o->cols[TG_AGG_TABLE], agg_cols, groups));
      for (int c = 0; c < agg_cols; c++) out.c[c] = o->cols[TG_AGG_TABLE][c];
      GG_LAUNCH(ctx, "k_tuple_write", k_tuple_write, stride_grid(ctx, groups), dim3(256), 0,
                (const unsigned long long *)A.cnt, (const TupleCell *)A.cell, groups, out, a.words + 4);
      GG_TRY(read_back(ctx, {{a.words + 4, 2 * sizeof(uint64_t), words_host + 4}}));
      if (words_host[5] != n_rows) {
        set_error("internal: %s put %llu of %llu rows into groups", fn, (unsigned long long)words_host[5],
                  (unsigned long long)n_rows);
        return GG_ERR_STATE;
      }
      words_host[3] = words_host[4];
    }
  }
  if (stats) {
    stats->rows_in = n_rows, stats->rows_valued = words_host[3], stats->groups = groups, stats->slots = cap;
    stats->probe_steps = words_host[0], stats->route = route;
  }
  if (o) {
    o->rows[0] = groups;
    *out_result = o.release();
  }
  return GG_OK;
}

extern "C" int gg_tuple_groups_rows(const gg_result *res, uint64_t *n_rows, int *n_key_cols) {
  GG_TRY(expect_kind(res, ResultKind::TUPLE_GROUPS, "gg_tuple_groups_rows"));
  if (!n_rows && !n_key_cols) return GG_ERR_INVALID_ARG;
  if (n_rows) *n_rows = res->rows[0];
  if (n_key_cols) *n_key_cols = res->k_max + 1;
  return GG_OK;
}

extern "C" int gg_tuple_groups_fetch(const gg_result *res, uint64_t offset, uint32_t max_rows, int64_t *const *keys,
                                     uint64_t *rows, uint64_t *valued, int64_t *sum_lo, int64_t *sum_hi, int64_t *min,
                                     int64_t *max, uint32_t *n_out) {
  GG_TRY(expect_kind(res, ResultKind::TUPLE_GROUPS, "gg_tuple_groups_fetch"));
  if (!n_out) return GG_ERR_INVALID_ARG;
  const int n_keys = res->k_max + 1;
  void *const agg[TG_AGG_COLS] = {rows, valued, sum_lo, sum_hi, min, max};
  // two slices: fetch_slice takes a table's GG_MAX_HOPS + 1 columns at most
  SliceCol want[DST_MAX_COLS];
  for (int j = 0; j < n_keys; j++) want[j] = {keys ? (void *)keys[j] : nullptr, res->cols[TG_KEYS_TABLE][j]};
  GG_TRY(fetch_slice(res->ctx, res->rows[0], offset, max_rows, want, n_keys, n_out));
  for (int c = 0; c < TG_AGG_COLS; c++) want[c] = {agg[c], res->cols[TG_AGG_TABLE][c]};
  GG_TRY(fetch_slice(res->ctx, res->rows[0], offset, max_rows, want, TG_AGG_COLS, n_out));
  // the count form forms no value state: those columns read as 0
  for (int c = 1; c < TG_AGG_COLS; c++)
    if (agg[c] && !res->cols[TG_AGG_TABLE][c]) memset(agg[c], 0, (size_t)*n_out * sizeof(int64_t));
  return GG_OK;
}

extern "C" int gg_debug_group_tuples(gg_ctx *ctx, int route, uint32_t lds_groups) {
  if (!ctx || route < 0 || route > 2) return GG_ERR_INVALID_ARG;
  ctx->tuple_route = route;
  ctx->tuple_lds_groups = lds_groups;
  return GG_OK;
}
