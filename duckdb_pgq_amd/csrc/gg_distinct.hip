// gg_distinct.hip — SELECT DISTINCT over chosen columns of a walk table: the first row of every tuple, in input order.
//
// The reference's LDBC statements form "friends and friends of friends" as a set before they join it with anything: a
// UNION (benchmark/ldbc/queries/interactive-complex-6.sql:3-12, -3, -5, -9, -11) or `SELECT DISTINCT k2.k_person2id`
// (interactive-complex-10.sql:19-24); bi-14.sql:30-102 takes `SELECT DISTINCT p1.personid, p2.personid` above chains that
// leave `knows`, and interactive-complex-10.sql:2-9 counts distinct messages per person.  There that is a
// PhysicalHashAggregate without aggregates (src/execution/operator/aggregate/physical_hash_aggregate.cpp:152-266).  Here the
// rows are columns in HBM and a walk table holds a friend of a friend once per middle vertex, so without this every later
// join and count sees that person once per walk.
//
// The table: `cap` slots of 32-bit ROW NUMBERS, not of keys — 4 bytes per slot whatever the number of chosen columns, no
// sentinel among the ids (every int64 value is an ordinary cell), one code path for 1 to 9 columns.  A slot holds the
// smallest row number seen so far among the rows of ONE tuple; the tuple is read from the input columns through it.
// The two kernels live in gg_tuples.h, which gg_group_tuples.hip includes as well.
//   k_distinct_insert  one thread per row, striding by workgroups of 256 rows: the chosen cells, their hash (fmix64 folded
//                      over the columns in their chosen order, so (a, b) and (b, a) differ), linear probing from the home
//                      slot.  An empty slot (0xFFFFFFFF) is claimed by a 32-bit atomicCAS of the own row number; on an
//                      occupied slot the occupant's tuple is compared in every chosen column: equal and the occupant is the
//                      smaller row — done, no atomic; equal and the own row is smaller — atomicMin; different — next slot.
//                      The slot the row ended in goes to a 4 B/row array.
//                      Lanes of a wavefront that hold the same tuple in adjacent rows are combined first (__shfl_up of the
//                      cells, as gg_group.hip's runs): only a run's first lane probes, the others are no first occurrences
//                      by construction.  Without it a table of 29 M rows over 64 distinct v0 sends every row to 64 slots.
//   k_distinct_flag    a kernel of its own — the kernel boundary orders it after every insert.  Row r survives iff the slot
//                      it ended in holds r.  The pass bit goes into a ballot word per wavefront, exactly as k_value_probe's.
//   count, scan, write gg_rows.h's k_value_groups / k_value_write over that mask, the chosen columns as the column list.
// All rows that ever share a slot hold one tuple (a row moves on from a slot whose tuple differs), so a slot's tuple never
// changes after its claim, and a tuple never owns two slots: a row can only pass a slot after it has seen a different tuple
// in it.
// A STALE plain read of a slot is harmless.  Slots are written by device-scope atomics only, which act in the memory-side
// cache; a plain load may be served by this CU's L1 or by this XCD's L2 and show an OLDER value of the slot.  The older
// values of a slot are: empty, or a larger row number of the same tuple.  Stale-empty is caught by the CAS, which returns
// the true occupant (then treated like any occupant).  A stale occupant q of the same tuple with q < r ends the row's work
// rightly — the true value is <= q < r; with q > r the atomicMin(r) is right whatever the true value is.  A stale occupant
// never has a different tuple than the true one.  Agent-scope (sc1) loads instead would pass the L1 on every probe for no
// change in the result; they were not measured.
// Kept slot or second probe in the flag pass (byte model): the kept slot costs 4 B/row written and 4 B/row read; a second
// probe reads the 8 c B/row of the c chosen cells again, hashes, and at every probed slot gathers the occupant's c cells from
// c random lines.  The slot is kept.
// No unbounded loop: cap is a power of two strictly greater than the number of rows (the next power of two >= 2 rows by
// default, at most 2^32), so an empty slot always exists, and the probe loop is bounded by cap all the same: a row that
// exhausts it sets the call's error word and the call returns GG_ERR_STATE.
// Bytes per row (model), c chosen columns: insert 8 c B cells + 4 B slot written + per probed slot one 4 B slot word (a
// 32 B sector) and, where occupied, c gathered cells (c sectors); flag 4 B slot number + one slot word + 1/8 B mask; write
// as gg_rows.h.  The table itself: 4 cap B set to 0xFF.
#include "gg_internal.h"
#include "gg_rows.h"
#include "gg_tuples.h"

using namespace gg;

extern "C" int gg_result_distinct(gg_ctx *ctx, const gg_result *res, int hops, const int *cols, int n_cols,
                                  int materialise, gg_distinct_stats *stats, gg_result **out_result) {
  if (out_result) *out_result = nullptr;
  if (stats) memset(stats, 0, sizeof(*stats));
  const char *fn = "gg_result_distinct";
  GG_TRY(result_arg(fn, ctx, res));
  if (!cols) {
    set_error("%s: NULL cols", fn);
    return GG_ERR_INVALID_ARG;
  }
  GG_TRY(walk_kind_arg(fn, res, KindRule::EXPECT));
  if (materialise && !out_result) {
    set_error("%s: materialise without out_result", fn);
    return GG_ERR_INVALID_ARG;
  }
  if (!stats && !out_result) {
    set_error("%s: neither stats nor out_result is asked for", fn);
    return GG_ERR_INVALID_ARG;
  }
  GG_TRY(tuple_columns_check(fn, res, hops, cols, n_cols));
  const uint64_t n_rows = res->rows[hops], n_words = (n_rows + 63) / 64;
  ApiScope scope(ctx);
  GG_HIP(hipSetDevice(ctx->device));
  const int out_hops = n_cols - 1;
  ResultOwner o;
  if (materialise) o = make_result(ctx, ResultKind::TABLES, out_hops, out_hops);
  uint64_t words_host[3] = {0, 0, 0}, total = 0, cap = 0;  // probe steps, error, rows that pass
  if (n_rows) {
    hipStream_t st = ctx->stream;
    cap = tuple_slots(ctx, n_rows);
    DistinctArgs a{};
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
    dim3 grid = stride_grid(ctx, n_rows);
    if (ctx->max_grid_tiles && ctx->max_grid_tiles < grid.x) grid.x = (unsigned)ctx->max_grid_tiles;
    GG_LAUNCH(ctx, "k_distinct_insert", k_distinct_insert, grid, dim3(256), 0, a);
    GG_LAUNCH(ctx, "k_distinct_flag", k_distinct_flag, grid, dim3(256), 0, a);
    uint64_t *group = nullptr;
    if (!materialise) {
      GG_TRY(read_back(ctx, {{a.words, sizeof(words_host), words_host}}));
      total = words_host[2];
    } else {
      GG_TRY(mask_prefix(ctx, a.mask, n_rows, {{a.words, sizeof(words_host), words_host}}, &group, &total));
    }
    if (words_host[1]) {
      set_error("internal: gg_result_distinct found no slot for a row in a table of %llu slots for %llu rows",
                (unsigned long long)cap, (unsigned long long)n_rows);
      return GG_ERR_STATE;
    }
    if (total != words_host[2]) {
      set_error("internal: gg_result_distinct counted %llu rows and flagged %llu", (unsigned long long)total,
                (unsigned long long)words_host[2]);
      return GG_ERR_STATE;
    }
    if (materialise && total) {
      ValIn in{};
      ValOut out{};
      GG_TRY(alloc_kept_columns(ctx, o->cols[out_hops], n_cols, total));
      for (int j = 0; j < n_cols; j++) in.c[j] = a.c[j], out.c[j] = o->cols[out_hops][j];
      GG_TRY(value_write_launch(ctx, in, n_cols, n_rows, a.mask, n_words, group, total, out));
      GG_TRY(sync_checked(ctx));
    }
  }
  if (stats) {
    stats->rows_in = n_rows, stats->rows_out = total, stats->slots = cap, stats->probe_steps = words_host[0];
  }
  if (materialise) {
    o->rows[out_hops] = total;
    *out_result = o.release();
  }
  return GG_OK;
}

extern "C" int gg_debug_distinct(gg_ctx *ctx, uint64_t slots, int combine) {
  if (!ctx || combine < 0 || combine > 1) return GG_ERR_INVALID_ARG;
  ctx->distinct_slots = slots;
  ctx->distinct_combine = combine;
  return GG_OK;
}
