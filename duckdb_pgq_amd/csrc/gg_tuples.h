// gg_tuples.h — the table of 32-bit row numbers that turns "tuple of 1 to 9 raw int64 cells" into "one stable slot": the
// insert and flag passes shared by gg_distinct.hip (first occurrences of a tuple) and gg_group_tuples.hip (aggregates per
// tuple).  What the table is, why a stale plain read of a slot is harmless and why no loop is unbounded is argued in
// gg_distinct.hip's file comment; the kernels are the ones that file held, moved here unchanged.
#pragma once
#include "gg_internal.h"
#include "gg_walk_table.h"

namespace gg {
namespace {

constexpr int DST_MAX_COLS = GG_MAX_HOPS + 1;
constexpr uint32_t DST_EMPTY = 0xFFFFFFFFu;  // no row: row numbers are below 2^32 - 1 (n_rows < 2^32)
constexpr uint64_t DST_MAX_SLOTS = 1ull << 32;

struct DistinctArgs {
  const int64_t *c[DST_MAX_COLS];  // the chosen columns, in their chosen order
  int ncols;
  uint64_t n_rows;
  uint32_t *tab;      // cap slots
  uint64_t cap;       // a power of two > n_rows
  uint32_t *slot_of;  // n_rows: the slot the row ended in (0 for a row that did not probe: no slot ever holds such a row)
  int combine;        // adjacent equal lanes of a wavefront are combined
  uint64_t *mask;     // ceil(n_rows / 64) words (k_distinct_flag)
  unsigned long long *words;  // [0] probe steps, [1] error (a row exhausted the probe bound), [2] rows that pass
};

// Workgroup g owns rows [256 g, 256 g + 256); the grid strides over the groups.
__global__ __launch_bounds__(256) void k_distinct_insert(DistinctArgs a) {
  const int lane = threadIdx.x & 63;
  const uint64_t groups = (a.n_rows + 255) / 256, smask = a.cap - 1;
  uint64_t steps = 0;
  bool failed = false;
  for (uint64_t g = blockIdx.x; g < groups; g += gridDim.x) {
    const uint64_t r = g * 256 + threadIdx.x;
    const bool live = r < a.n_rows;
    int64_t mine[DST_MAX_COLS];
    uint64_t h = 0;
    bool same = true;  // as the row of the lane below
#pragma unroll
    for (int c = 0; c < DST_MAX_COLS; c++) {
      if (c < a.ncols) {  // (uniform: every lane shuffles)
        mine[c] = live ? a.c[c][r] : 0;
        h = fmix64((h ^ (uint64_t)mine[c]) + DIG_GOLD);
        const int64_t below = (int64_t)__shfl_up((unsigned long long)mine[c], 1, 64);
        same = same && below == mine[c];
      }
    }
    // (lane l - 1 holds row r - 1 < n_rows whenever lane l is live)
    const bool probes = live && !(a.combine && lane != 0 && same);
    uint32_t my_slot = 0;
    if (probes) {
      const uint32_t me = (uint32_t)r;
      uint64_t s = h & smask;
      bool done = false;
      for (uint64_t t = 0; t < a.cap && !done; t++, s = (s + 1) & smask) {  // (s < cap: the table's bound)
        steps++;
        uint32_t occ = __atomic_load_n(&a.tab[s], __ATOMIC_RELAXED);  // (may be stale: see the file comment)
        if (occ == DST_EMPTY) {
          occ = atomicCAS(&a.tab[s], DST_EMPTY, me);
          if (occ == DST_EMPTY) {
            my_slot = (uint32_t)s, done = true;
            break;
          }
        }
        if (occ >= a.n_rows) break;  // (cannot happen: a slot holds empty or a row number; never gather out of bounds)
        bool eq = true;
#pragma unroll
        for (int c = 0; c < DST_MAX_COLS; c++)
          if (c < a.ncols) eq = eq && a.c[c][occ] == mine[c];
        if (eq) {
          if (me < occ) atomicMin(&a.tab[s], me);
          my_slot = (uint32_t)s, done = true;
        }
      }
      if (!done) failed = true, my_slot = 0;
    }
    if (live) a.slot_of[r] = my_slot;
  }
  steps = wave_reduce_add_u64(steps);
  if (lane == 0 && steps) atomicAdd(&a.words[0], (unsigned long long)steps);
  if (failed) atomicMax(&a.words[1], 1ull);
}

// row r passes iff its slot holds r; mask word r / 64 is the wavefront's ballot, as k_value_probe writes it
__global__ __launch_bounds__(256) void k_distinct_flag(DistinctArgs a) {
  const int lane = threadIdx.x & 63;
  const uint64_t groups = (a.n_rows + 255) / 256;
  uint64_t passed = 0;  // (uniform over the wavefront)
  for (uint64_t g = blockIdx.x; g < groups; g += gridDim.x) {
    const uint64_t r = g * 256 + threadIdx.x;
    bool pass = false;
    if (r < a.n_rows) {
      const uint32_t s = a.slot_of[r];  // (< cap)
      pass = a.tab[s] == (uint32_t)r;
    }
    const uint64_t pm = __ballot(pass);
    passed += (uint64_t)__popcll(pm);
    if (lane == 0 && (r & ~63ull) < a.n_rows) a.mask[r >> 6] = pm;  // (r >> 6 < ceil(n_rows / 64))
  }
  if (lane == 0 && passed) atomicAdd(&a.words[2], (unsigned long long)passed);
}

uint64_t pow2_at_least(uint64_t n) {
  uint64_t p = 1;
  while (p < n) p <<= 1;
  return p;
}

// the slot count of a call over n_rows > 0 rows: the next power of two >= 2 n_rows, or gg_debug_distinct's, raised to the
// smallest power of two above n_rows (so an empty slot always exists; n_rows < 2^32, so 2^32 slots always do)
uint64_t tuple_slots(const gg_ctx *ctx, uint64_t n_rows) {
  const uint64_t want = ctx->distinct_slots ? ctx->distinct_slots : 2 * n_rows;
  uint64_t cap = pow2_at_least(want < DST_MAX_SLOTS ? want : DST_MAX_SLOTS);
  const uint64_t least = pow2_at_least(n_rows + 1);  // (<= 2^32)
  return cap < least ? least : cap;
}

// gg_result_distinct's argument checks on (hops, cols, n_cols) and the table's size, under the caller's name
int tuple_columns_check(const char *fn, const gg_result *res, int hops, const int *cols, int n_cols) {
  GG_TRY(hops_arg(fn, res, hops));
  if (n_cols < 1 || n_cols > hops + 1) {
    set_error("%s: %d columns chosen, outside 1..%d", fn, n_cols, hops + 1);
    return GG_ERR_INVALID_ARG;
  }
  uint32_t seen = 0;
  for (int j = 0; j < n_cols; j++) {
    if (cols[j] < 0 || cols[j] > hops || ((seen >> cols[j]) & 1u)) {
      set_error("%s: column %d (place %d) outside 0..%d or chosen twice", fn, cols[j], j, hops);
      return GG_ERR_INVALID_ARG;
    }
    seen |= 1u << cols[j];
  }
  const uint64_t n_rows = res->rows[hops];
  if (n_rows >= (1ull << 32)) {
    set_error("%s: a table of %llu rows (2^32 or more); filter it first", fn, (unsigned long long)n_rows);
    return GG_ERR_TOO_LARGE;
  }
  return id_columns_present(fn, res, hops, cols, n_cols);
}

}  // namespace
}  // namespace gg
