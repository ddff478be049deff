// gg_rows.h — keep the rows of a walk table whose bit is set in a pass mask: count, scan, write.  Shared by the operators
// that decide per row and then compact (gg_value.hip: a value predicate; gg_distinct.hip: first occurrences of a tuple).
//
// The mask holds one bit per input row, word i the rows [64 i, 64 i + 64) — a wavefront's __ballot, stored by its lane 0.
//   k_value_groups  one thread per group of 256 rows: the popcount of its four mask words
//   scan            exclusive prefix of the groups' rows (mask_prefix runs both; the caller's read-back items ride on it)
//   k_value_write   a row's place is the group's prefix + the popcounts of the group's mask words below its wavefront +
//                   the popcount of its own word below its lane: no LDS, no barrier.  It copies the cells of the columns
//                   it is given; the kept lanes of a wavefront write consecutive cells of every column, in input order,
//                   at the same places on every run.
// Bytes per row (model): 1/8 B mask + 8 (columns) B read per kept row + 8 (columns) B written.
#pragma once
#include "gg_internal.h"
#include "gg_walk_table.h"

namespace gg {
namespace {

constexpr int VAL_MAX_COLS = 2 * GG_MAX_HOPS + 1;  // hops + 1 id columns and hops edge columns

struct ValIn {
  const int64_t *c[VAL_MAX_COLS];
};
struct ValOut {
  int64_t *c[VAL_MAX_COLS];
};

__device__ __forceinline__ uint64_t mask_word(const uint64_t *__restrict__ mask, uint64_t n_words, uint64_t i) {
  return i < n_words ? mask[i] : 0;
}

// group[g] = rows of group g that pass
__global__ __launch_bounds__(256) void k_value_groups(const uint64_t *__restrict__ mask, uint64_t n_words, uint64_t groups,
                                                      uint64_t *__restrict__ group) {
  for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t n = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) n += (uint32_t)__popcll(mask_word(mask, n_words, 4 * g + k));
    group[g] = n;
  }
}

// Workgroup g0 + blockIdx.x owns rows [256 g, 256 g + 256); group[g] is its first output row.
__global__ __launch_bounds__(256) void k_value_write(ValIn in, int ncols, uint64_t g0, uint64_t n_rows,
                                                     const uint64_t *__restrict__ mask, uint64_t n_words,
                                                     const uint64_t *__restrict__ group, uint64_t total, ValOut out) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint64_t g = g0 + blockIdx.x, r = g * 256 + threadIdx.x;
  uint64_t pos = group[g];
  for (int k = 0; k < wave; k++) pos += (uint64_t)__popcll(mask_word(mask, n_words, 4 * g + k));
  const uint64_t mine = mask_word(mask, n_words, 4 * g + wave);
  pos += (uint64_t)__popcll(mine & ((1ull << lane) - 1));
  // (a set bit is a row < n_rows, and pos < total: the groups' counts are the popcounts of the same words)
  if (((mine >> lane) & 1ull) && r < n_rows && pos < total) {
#pragma unroll
    for (int c = 0; c < VAL_MAX_COLS; c++)
      if (c < ncols) out.c[c][pos] = in.c[c][r];
  }
}

// The mask's prefix: *group (from the pool) gets the exclusive prefix of the passing rows per group of 256 rows, *total
// their number.  One host synchronisation, the scan's read-back, on which the caller's `extra` items ride.
int mask_prefix(gg_ctx *ctx, const uint64_t *mask, uint64_t n_rows, std::initializer_list<ReadBack> extra, uint64_t **group,
                uint64_t *total) {
  const uint64_t groups = (n_rows + 255) / 256, n_words = (n_rows + 63) / 64;
  GG_TRY(ctx->dev_alloc((void **)group, groups * sizeof(uint64_t)));
  GG_LAUNCH(ctx, "k_value_groups", k_value_groups, stride_grid(ctx, groups), dim3(256), 0, mask, n_words, groups, *group);
  return scan_total_u64(ctx, *group, *group, groups, total, false, extra);
}

int value_write_launch(gg_ctx *ctx, const ValIn &in, int ncols, uint64_t n_rows, const uint64_t *mask, uint64_t n_words,
                       const uint64_t *group, uint64_t total, const ValOut &out) {
  return split_groups(ctx, (n_rows + 255) / 256, [&](uint64_t g0, uint64_t ng) -> int {
    GG_LAUNCH(ctx, "k_value_write", k_value_write, dim3((unsigned)ng), dim3(256), 0, in, ncols, g0, n_rows, mask, n_words,
              group, total, out);
    return GG_OK;
  });
}

}  // namespace
}  // namespace gg
