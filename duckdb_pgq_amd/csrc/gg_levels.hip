// gg_levels.hip — level sets: for every level L >= 1 the set of (class, vertex) that L edges lead to from the seeds.
//
// Replaces the reference's PhysicalRecursiveCTE over a UNION arm that joins the CTE with one table on one column and
// carries a depth counter `counter + constant` (src/execution/operator/set/physical_recursive_cte.cpp:47-139; the
// friends(startPerson, hopCount, friend) CTE of benchmark/ldbc/queries/bi-10-shortestpath.sql:8-25).  A row of level L
// carries start + step * L, so it never equals a row of another level: UNION only deduplicates inside a level, and
// level L is the set image of level L - 1 under the CSR's edges key -> next, per class of carried columns.  No visited
// set survives a level (gg_reach.hip's is cumulative), and the recursion ends by its bound or on an empty level.
//   level 0   the frontier is every seed (class, dense id); duplicates are harmless (level 1 is a set)
//   level L   frontier_offsets     degrees of the frontier's vertices, their exclusive scan, the child count M
//             (the set is emptied, see below)
//             one of two order routes gives the level's rows ascending by (class, vertex index):
//     sort      expand_claim_sorted, gg_reach.hip's step: one thread per child reads, then claims (class, child); a
//               wave's winners append through one returning add; the rows are radix-sorted by vertex, then class
//     compact   (bitmap only) k_levels_mark   one thread per child: read the word, and only if the bit is clear a
//                                             non-returning atomicOr — no ballot, no counter, no returned value
//                             k_levels_count  popcount per 16-byte group of words -> scan_exclusive_u32
//                             k_levels_rows   every set bit b of a group at its scanned position: class b / V, vertex
//                                             b % V (a word may straddle two classes); ascending b is ascending
//                                             (class, vertex), so nothing is sorted
//   The rows are level L's output and level L + 1's frontier.
// The per-level set, two forms (same rows, same order):
//   bitmap    bit class * V + vertex, under gg_reach.hip's budget (2^33 bits, a quarter of the free memory).  Between
//             levels exactly the previous level's rows are set.  Emptying it, by bytes moved (W words of 4 bytes,
//             n rows of the previous level, sorted, so the words they touch lie in runs):
//               whole map       4 W                        written
//               touched words   8 n  +  64 min(n, W / 16)  the rows read, every touched 64-byte line written
//             the cheaper one is taken.
//   hash set  64-bit keys class << 32 | vertex in at least 2 M slots: M is known from the scan before the expand
//             launches, so the set never grows or rebuilds inside a level.  The allocation is kept across levels and
//             enlarged only when a level needs more; the slots a level uses are reset to empty before it.
// Order route, chosen per level over a bitmap from bytes moved (n <= min(M, bits) rows expected, p radix passes of 8
// bits over vertex and class indices):
//     compact   4 W (count reads) + 4 W (rows reads) + 3 W (group counts written, scanned, read) + 8 n (rows written)
//     sort      8 n (append) + 24 p n (per pass: the pairs read for the histogram, read again, written)
//               + one returning add on one word per winning wave + LEVELS_SORT_FIXED_BYTES
//   Emptying costs both the same.  Compact is taken when 11 W <= 24 p n + LEVELS_SORT_FIXED_BYTES.  The fixed term is
//   what the sort route costs before it moves a byte — two launches per radix pass, the count word's reset and read —
//   expressed as the bytes the chip streams in that time: measured 0.03-0.06 ms per level on levels too small to load
//   it, 128 MiB at the ~4 TB/s such passes reach.  So sort is only taken over a map of more than
//   ~49 MB whose level is sparse; on the dense levels of a mirrored graph and on every small map compact wins.
#include <algorithm>

#include "gg_internal.h"

using namespace gg;

namespace {

constexpr uint64_t LEVELS_BITMAP_MAX_BITS = 1ull << 33;  // REACH_BITMAP_MAX_BITS of gg_reach.hip
constexpr uint64_t LEVELS_MIN_SLOTS = 1024;
constexpr uint64_t LEVELS_SORT_FIXED_BYTES = 128ull << 20;

// one thread per child: the bit of (class, child) set, without asking who set it
__global__ __launch_bounds__(XT) void k_levels_mark(const uint32_t *__restrict__ off, const uint32_t *__restrict__ nbr,
                                                    const uint32_t *__restrict__ fcls, const uint32_t *__restrict__ fvtx,
                                                    const uint64_t *__restrict__ foff, uint64_t n_entries, uint64_t M,
                                                    const uint32_t *__restrict__ tile_entry, uint32_t *__restrict__ bits,
                                                    uint64_t V) {
  __shared__ uint64_t s_foff[XT + 1];
  const uint64_t p = (uint64_t)blockIdx.x * XT + threadIdx.x;  // foff[0] == 0: an exclusive scan
  const uint64_t i0 = tile_entry[blockIdx.x];
  load_window(s_foff, foff, n_entries, i0);
  __syncthreads();
  if (p >= M) return;
  uint64_t k;
  const uint64_t i = locate_entry(s_foff, foff, n_entries, i0, p, &k);
  const uint64_t b = (uint64_t)fcls[i] * V + nbr[off[fvtx[i]] + (uint32_t)k];
  const uint32_t mask = 1u << (b & 31);
  if (!(__atomic_load_n(&bits[b >> 5], __ATOMIC_RELAXED) & mask)) atomicOr(&bits[b >> 5], mask);  // (result unused)
}

// set bits per group of four words
__global__ __launch_bounds__(256) void k_levels_count(const uint4 *__restrict__ groups, uint64_t n_groups,
                                                      uint32_t *__restrict__ count) {
  for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n_groups; g += (uint64_t)gridDim.x * blockDim.x) {
    const uint4 w = groups[g];
    count[g] = __popc(w.x) + __popc(w.y) + __popc(w.z) + __popc(w.w);
  }
}

// (class, vertex) of every set bit of group g at at[g] and after, in ascending bit order
__global__ __launch_bounds__(256) void k_levels_rows(const uint4 *__restrict__ groups, uint64_t n_groups,
                                                     const uint32_t *__restrict__ at, uint64_t V,
                                                     uint32_t *__restrict__ out_cls, uint32_t *__restrict__ out_vtx) {
  for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n_groups; g += (uint64_t)gridDim.x * blockDim.x) {
    const uint4 w4 = groups[g];
    if (!(w4.x | w4.y | w4.z | w4.w)) continue;
    const uint32_t word[4] = {w4.x, w4.y, w4.z, w4.w};
    uint32_t r = at[g];
    uint64_t c = g * 128 / V, c_first = c * V;  // the class of the group's first bit, and that class's first bit
#pragma unroll
    for (int j = 0; j < 4; j++) {
      for (uint32_t w = word[j]; w; w &= w - 1) {
        const uint64_t b = g * 128 + j * 32 + (__ffs(w) - 1);
        while (b - c_first >= V) {  // (V need not be a multiple of 32: a word may hold the end of one class and the
          c_first += V;             // start of the next, or several whole classes of a tiny V)
          c++;
        }
        out_cls[r] = (uint32_t)c;
        out_vtx[r] = (uint32_t)(b - c_first);
        r++;
      }
    }
  }
}

// the words of the previous level's rows back to zero
__global__ __launch_bounds__(256) void k_levels_clear(const uint32_t *__restrict__ cls, const uint32_t *__restrict__ vtx,
                                                      uint64_t n, uint64_t V, uint32_t *__restrict__ bits) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    bits[((uint64_t)cls[i] * V + vtx[i]) >> 5] = 0;
}

int radix_passes(uint64_t n) { return (bits_for(n) + 7) / 8; }

}  // namespace

extern "C" int gg_debug_level_sets(gg_ctx *ctx, int set_mode, int order_mode) {
  if (!ctx || set_mode < 0 || set_mode > 2 || order_mode < 0 || order_mode > 2) return GG_ERR_INVALID_ARG;
  if (set_mode == 2 && order_mode == 2) {
    set_error("gg_debug_level_sets: the compact order route reads a bitmap, not the hash set");
    return GG_ERR_INVALID_ARG;
  }
  ctx->levels_set_mode = set_mode;
  ctx->levels_order_mode = order_mode;
  return GG_OK;
}

extern "C" int gg_level_sets(gg_ctx *ctx, const gg_csr *csr, const int64_t *seed_ids, const uint32_t *seed_class,
                             uint64_t n_seeds, uint32_t n_classes, int max_levels, gg_result **out) {
  ApiScope scope(ctx);
  if (!out || (n_seeds && (!seed_ids || !seed_class))) return GG_ERR_INVALID_ARG;
  *out = nullptr;
  GG_TRY(check_whole_csr(ctx, csr));
  if (n_seeds >= (1ull << 32)) {
    set_error("gg_level_sets: %llu seeds do not fit a 32-bit seed index", (unsigned long long)n_seeds);
    return GG_ERR_TOO_LARGE;
  }
  for (uint64_t i = 0; i < n_seeds; i++) {
    if (seed_class[i] >= n_classes) {
      set_error("gg_level_sets: seed %llu has class %u of %u", (unsigned long long)i, seed_class[i], n_classes);
      return GG_ERR_INVALID_ARG;
    }
  }
  GG_HIP(hipSetDevice(ctx->device));
  ResultOwner res = make_result(ctx, ResultKind::LEVEL_SETS);
  uint32_t *seed_dense = nullptr, *seed_cls = nullptr;
  GG_TRY(upload_ids(ctx, csr, seed_ids, n_seeds, &seed_dense));
  GG_TRY(ctx->dev_alloc((void **)&seed_cls, (n_seeds ? n_seeds : 1) * sizeof(uint32_t)));
  if (n_seeds) GG_HIP(hipMemcpyAsync(seed_cls, seed_class, n_seeds * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));

  // ---- the set's form
  Visited vs;
  vs.V = csr->V;
  const uint64_t bits = (uint64_t)n_classes * csr->V;
  bool bitmap = ctx->levels_set_mode == 1;
  if (ctx->levels_set_mode == 0) {
    size_t free_bytes = 0, total_bytes = 0;
    GG_HIP(hipMemGetInfo(&free_bytes, &total_bytes));
    bitmap = bits <= LEVELS_BITMAP_MAX_BITS && bits / 8 <= free_bytes / 4;
  }
  if (!bitmap && ctx->levels_order_mode == 2) {  // (auto chose the hash set under a forced compact route)
    set_error("gg_level_sets: the compact order route reads a bitmap, and %llu bits are over the bitmap's budget",
              (unsigned long long)bits);
    return GG_ERR_INVALID_ARG;
  }
  // whole groups of four words, the padding never set, so that k_levels_count / k_levels_rows read 16 bytes at a time
  const uint64_t n_groups = std::max<uint64_t>((bits + 127) / 128, 1), words = 4 * n_groups;
  uint64_t slots_allocated = 0;

  std::vector<PairLevel> levels;
  uint32_t *count = nullptr;
  GG_TRY(ctx->dev_alloc((void **)&count, sizeof(uint32_t)));
  const uint32_t *fcls = seed_cls, *fvtx = seed_dense;
  uint64_t n_parent = n_seeds;
  for (int level = 1; n_parent > 0 && (max_levels < 0 || level <= max_levels); level++) {
    uint64_t *foff = nullptr, M = 0;
    GG_TRY(frontier_offsets(ctx, csr, fvtx, n_parent, &foff, &M));
    if (M == 0) break;
    if (M >= (1ull << 32)) {
      set_error("gg_level_sets: level %d has %llu children (2^32 or more)", level, (unsigned long long)M);
      return GG_ERR_TOO_LARGE;
    }
    if (max_levels < 0 && (uint64_t)level > csr->V) {
      // a walk of V + 1 edges visits some vertex twice: the recursion would never reach an empty level
      set_error("gg_level_sets: level %d is not empty, so a walk repeats a vertex (a cycle is reachable from a seed); "
                "an unbounded recursion over it never ends — bound the levels", level);
      return GG_ERR_STATE;
    }
    // ---- the set, empty
    if (bitmap) {
      if (!vs.bits) {
        GG_TRY(ctx->dev_alloc((void **)&vs.bits, words * sizeof(uint32_t)));
        GG_HIP(hipMemsetAsync(vs.bits, 0, words * sizeof(uint32_t), ctx->stream));
      } else {  // the set bits are exactly the previous level's rows: the frontier
        const uint64_t whole = 4 * words, touched = 8 * n_parent + 64 * std::min<uint64_t>(n_parent, words / 16);
        if (touched < whole)
          GG_LAUNCH(ctx, "levels_clear", k_levels_clear, stride_grid(ctx, n_parent), dim3(256), 0, fcls, fvtx, n_parent,
                    vs.V, vs.bits);
        else
          GG_HIP(hipMemsetAsync(vs.bits, 0, words * sizeof(uint32_t), ctx->stream));
      }
    } else {
      vs.cap = std::max<uint64_t>(2 * M, LEVELS_MIN_SLOTS);
      if (vs.cap > slots_allocated) {
        if (vs.slots) ctx->dev_free(vs.slots);
        vs.slots = nullptr;
        GG_TRY(ctx->dev_alloc((void **)&vs.slots, vs.cap * sizeof(unsigned long long)));
        slots_allocated = vs.cap;
      }
      GG_HIP(hipMemsetAsync(vs.slots, 0xFF, vs.cap * sizeof(unsigned long long), ctx->stream));
    }
    // ---- the order route
    bool compact = bitmap && ctx->levels_order_mode == 2;
    if (bitmap && ctx->levels_order_mode == 0) {
      const uint64_t n_est = std::min<uint64_t>(M, bits);
      const uint64_t passes = radix_passes(csr->V) + (n_classes > 1 ? radix_passes(n_classes) : 0);
      compact = 11 * words <= 24 * passes * n_est + LEVELS_SORT_FIXED_BYTES;
    }
    PairLevel l{nullptr, nullptr, 0};
    if (!compact) {
      GG_TRY(expand_claim_sorted(ctx, csr, fcls, fvtx, foff, n_parent, M, vs, n_classes, count, &l));
      ctx->dev_free(foff);
    } else {
      uint32_t *tile_entry = nullptr, *group_at = nullptr;
      uint64_t n_tiles = 0;
      GG_TRY(make_tiles_u64(ctx, foff, n_parent, M, &tile_entry, &n_tiles));
      GG_LAUNCH(ctx, "levels_mark", k_levels_mark, dim3((unsigned)n_tiles), dim3(XT), 0, csr->off, csr->nbr, fcls, fvtx,
                foff, n_parent, M, tile_entry, vs.bits, vs.V);
      GG_TRY(ctx->dev_alloc((void **)&group_at, n_groups * sizeof(uint32_t)));
      GG_LAUNCH(ctx, "levels_count", k_levels_count, stride_grid(ctx, n_groups), dim3(256), 0, (const uint4 *)vs.bits,
                n_groups, group_at);
      GG_TRY(scan_total_u32(ctx, group_at, group_at, n_groups, &l.n));  // (>= 1: M > 0 children were marked)
      ctx->dev_free(tile_entry);
      ctx->dev_free(foff);
      GG_TRY(ctx->dev_alloc((void **)&l.cls, l.n * sizeof(uint32_t)));
      GG_TRY(ctx->dev_alloc((void **)&l.vtx, l.n * sizeof(uint32_t)));
      GG_LAUNCH(ctx, "levels_rows", k_levels_rows, stride_grid(ctx, n_groups), dim3(256), 0, (const uint4 *)vs.bits,
                n_groups, (const uint32_t *)group_at, vs.V, l.cls, l.vtx);
      ctx->dev_free(group_at);
    }
    if (l.n == 0) break;  // (not reached with M > 0; kept so that an empty level never becomes a frontier)
    levels.push_back(l);
    res->level_rows.push_back(l.n);
    fcls = l.cls;
    fvtx = l.vtx;
    n_parent = l.n;
  }

  GG_TRY(emit_pair_levels(ctx, csr, levels, res.get()));
  *out = res.release();
  return GG_OK;
}

extern "C" int gg_level_sets_levels(const gg_result *res, uint64_t *rows_per_level, int capacity, int *n_levels) {
  GG_TRY(expect_kind(res, ResultKind::LEVEL_SETS, "gg_level_sets_levels"));
  return level_rows_levels(res, rows_per_level, capacity, n_levels);
}

extern "C" int gg_level_sets_fetch(const gg_result *res, uint64_t offset, uint32_t max_rows, int64_t *seed_class,
                                   int64_t *vertex_id, int32_t *level, uint32_t *n_out) {
  GG_TRY(expect_kind(res, ResultKind::LEVEL_SETS, "gg_level_sets_fetch"));
  return level_rows_fetch(res, offset, max_rows, seed_class, vertex_id, level, n_out);
}
