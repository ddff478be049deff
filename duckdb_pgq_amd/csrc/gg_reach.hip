// gg_reach.hip — reachability closure: every (class, vertex) reachable from a list of seeds, each pair once.
//
// Replaces the reference's PhysicalRecursiveCTE over a UNION (not UNION ALL) arm that joins the CTE with one table on
// one column (src/execution/operator/set/physical_recursive_cte.cpp:47-70 ProbeHT / Sink: every produced row is probed
// against a GroupedAggregateHashTable of every row emitted so far and only new groups are kept; :75-139 the loop, the
// arm's hash join rebuilt per level).  The table's rows are the CSR's edges key -> next; a CTE row is (class, vertex):
// the class stands for the columns the arm carries unchanged, the vertex for the link.  A multi-source BFS whose
// visited set is keyed by (class, vertex):
//   level 0   the frontier is every seed (class, dense id); the visited set holds the seeds marked seen (their anchor
//             row equals an arm row: gg_reach_closure's seed_seen)
//   level L   k_reach_deg       degree of every frontier entry's vertex (a gather of off[v], off[v+1])
//             scan              exclusive prefix of the degrees (scan_exclusive_u64; one 8-byte read of the total)
//             tile_partition    the entry each tile of XT children starts in (make_tiles_u64)
//             k_reach_expand    one thread per child: test-and-set (class, nbr) in the visited set; the winners of a
//                               wave append with ONE returning atomic add (ballot + popcount), not one per lane
//             (one 4-byte read of the number of new rows)
//             sort              the new rows by (class, vertex index): a stable radix sort by vertex, then by class
//                               (sort_pairs_by_key; the second pass is skipped for one class) — so a level's rows do
//                               not depend on the order the atomics arrived in
//   The sorted new rows are level L's rows and level L + 1's frontier; the first empty level ends the recursion (each
//   (class, vertex) enters the visited set once, so it always ends, cycles included).
// Visited set, two forms (same rows, same order):
//   bitmap    n_classes x V bits, claimed with a returning atomicOr; taken while that is at most REACH_BITMAP_MAX_BITS
//             bits and a quarter of the device's free memory (single-source reachability, a tag-class hierarchy)
//   hash set  open addressing over 64-bit keys class << 32 | vertex, claimed with a 64-bit atomicCAS.  Before a level
//             expands M children the table holds at least 2 x (visited + M) slots, so an insert always finds an empty
//             slot; it grows by a rebuild from the seen seeds plus every level's rows, which are exactly the visited set.
// k_reach_emit finally writes the int64 (class, vertex id) columns a fetch reads.
#include <algorithm>

#include "gg_internal.h"

using namespace gg;

namespace {

// the bitmap form's budget: 2^33 bits = 1 GiB (and never more than a quarter of the free device memory); above it —
// e.g. 10 M classes over 100 M vertices — the hash set, whose size follows the rows actually reached
constexpr uint64_t REACH_BITMAP_MAX_BITS = 1ull << 33;
constexpr uint64_t REACH_MIN_SLOTS = 1024;

__global__ __launch_bounds__(256) void k_reach_deg(const uint32_t *__restrict__ off, const uint32_t *__restrict__ vtx,
                                                   uint64_t n, uint64_t *__restrict__ deg) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t v = vtx[i];
    deg[i] = v == INVALID_U32 ? 0 : (uint64_t)(off[v + 1] - off[v]);
  }
}

// (cls[i], vtx[i]) into the set, i < n (seen: only where seen[i] != 0; vertex INVALID_U32: skipped) — the seen seeds at
// the start, and every visited entry again when the hash set is rebuilt larger
__global__ __launch_bounds__(256) void k_reach_insert(const uint32_t *__restrict__ cls, const uint32_t *__restrict__ vtx,
                                                      const uint8_t *__restrict__ seen, uint64_t n, Visited vs) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    if ((!seen || seen[i]) && vtx[i] != INVALID_U32) claim(vs, cls[i], vtx[i]);
  }
}

__global__ __launch_bounds__(XT) void k_reach_expand(const uint32_t *__restrict__ off, const uint32_t *__restrict__ nbr,
                                                     const uint32_t *__restrict__ fcls, const uint32_t *__restrict__ fvtx,
                                                     const uint64_t *__restrict__ foff, uint64_t n_entries, uint64_t M,
                                                     const uint32_t *__restrict__ tile_entry, Visited vs,
                                                     uint32_t *__restrict__ count, uint32_t *__restrict__ out_cls,
                                                     uint32_t *__restrict__ out_vtx) {
  __shared__ uint64_t s_foff[XT + 1];
  const uint64_t p = (uint64_t)blockIdx.x * XT + threadIdx.x;  // foff[0] == 0: an exclusive scan
  const uint64_t i0 = tile_entry[blockIdx.x];
  load_window(s_foff, foff, n_entries, i0);
  __syncthreads();
  bool won = false;
  uint32_t c = 0, w = 0;
  if (p < M) {  // (no early return: the whole wave takes part in the ballot below)
    uint64_t k;
    const uint64_t i = locate_entry(s_foff, foff, n_entries, i0, p, &k);
    c = fcls[i];
    w = nbr[off[fvtx[i]] + (uint32_t)k];
    won = claim(vs, c, w);
  }
  const uint64_t winners = __ballot(won);
  if (!winners) return;
  const int lane = threadIdx.x & 63, leader = __ffsll((unsigned long long)winners) - 1;
  uint32_t base = 0;
  if (lane == leader) base = atomicAdd(count, (uint32_t)__popcll(winners));
  base = __shfl(base, leader, 64);
  if (won) {
    const uint32_t at = base + (uint32_t)__popcll(winners & ((1ull << lane) - 1));
    out_cls[at] = c;
    out_vtx[at] = w;
  }
}

// the high piece of every class index, as a sort key of its own (expand_claim_sorted, more than 2^31 classes)
constexpr int REACH_CLASS_PIECE_BITS = 16;
__global__ __launch_bounds__(256) void k_reach_class_high(const uint32_t *__restrict__ cls, uint64_t n,
                                                          uint32_t *__restrict__ high) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    high[i] = cls[i] >> REACH_CLASS_PIECE_BITS;
}

// rows of one level -> the result's int64 columns at their offset
__global__ __launch_bounds__(256) void k_reach_emit(const uint32_t *__restrict__ cls, const uint32_t *__restrict__ vtx,
                                                    uint64_t n, const int64_t *__restrict__ vid,
                                                    int64_t *__restrict__ cls_out, int64_t *__restrict__ vid_out,
                                                    const unsigned long long *__restrict__ err) {
  if (*err) return;  // the rows of a level are not all written after a scan error (see k_radix_scatter)
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (uint64_t)gridDim.x * blockDim.x) {
    cls_out[r] = (int64_t)cls[r];
    vid_out[r] = vid[vtx[r]];
  }
}

using Level = PairLevel;

// a hash set of `cap` slots holding the seen seeds and every level's rows so far
int hash_build(gg_ctx *ctx, uint64_t cap, const uint32_t *seed_cls, const uint32_t *seed_dense, const uint8_t *seen,
               uint64_t n_seeds, const std::vector<Level> &levels, Visited *vs) {
  if (vs->slots) ctx->dev_free(vs->slots);
  vs->slots = nullptr;
  GG_TRY(ctx->dev_alloc((void **)&vs->slots, cap * sizeof(unsigned long long)));
  vs->cap = cap;
  GG_HIP(hipMemsetAsync(vs->slots, 0xFF, cap * sizeof(unsigned long long), ctx->stream));
  if (seen && n_seeds)
    GG_LAUNCH(ctx, "reach_insert", k_reach_insert, stride_grid(ctx, n_seeds), dim3(256), 0, seed_cls, seed_dense, seen,
              n_seeds, *vs);
  for (const Level &l : levels)
    GG_LAUNCH(ctx, "reach_insert", k_reach_insert, stride_grid(ctx, l.n), dim3(256), 0, l.cls, l.vtx,
              (const uint8_t *)nullptr, l.n, *vs);
  return GG_OK;
}

}  // namespace

namespace gg {

int frontier_offsets(gg_ctx *ctx, const gg_csr *csr, const uint32_t *fvtx, uint64_t n_parent, uint64_t **foff_out,
                     uint64_t *M) {
  uint64_t *foff = nullptr;
  GG_TRY(ctx->dev_alloc((void **)&foff, (n_parent + 1) * sizeof(uint64_t)));
  GG_LAUNCH(ctx, "reach_deg", k_reach_deg, stride_grid(ctx, n_parent), dim3(256), 0, csr->off, fvtx, n_parent, foff);
  GG_TRY(offsets_from_deg(ctx, foff, n_parent, M));
  *foff_out = foff;
  return GG_OK;
}

int expand_claim_sorted(gg_ctx *ctx, const gg_csr *csr, const uint32_t *fcls, const uint32_t *fvtx, const uint64_t *foff,
                        uint64_t n_parent, uint64_t M, const Visited &vs, uint32_t n_classes, uint32_t *count,
                        PairLevel *out) {
  *out = PairLevel{nullptr, nullptr, 0};
  uint32_t *tile_entry = nullptr;
  uint64_t n_tiles = 0;
  GG_TRY(make_tiles_u64(ctx, foff, n_parent, M, &tile_entry, &n_tiles));
  uint32_t *new_cls = nullptr, *new_vtx = nullptr;
  GG_TRY(ctx->dev_alloc((void **)&new_cls, M * sizeof(uint32_t)));
  GG_TRY(ctx->dev_alloc((void **)&new_vtx, M * sizeof(uint32_t)));
  GG_HIP(hipMemsetAsync(count, 0, sizeof(uint32_t), ctx->stream));
  GG_LAUNCH(ctx, "reach_expand", k_reach_expand, dim3((unsigned)n_tiles), dim3(XT), 0, csr->off, csr->nbr, fcls, fvtx,
            foff, n_parent, M, tile_entry, vs, count, new_cls, new_vtx);
  uint32_t n_new = 0;
  GG_TRY(read_back(ctx, {{count, sizeof(uint32_t), &n_new}}));
  ctx->dev_free(tile_entry);
  if (n_new == 0) {
    ctx->dev_free(new_vtx);
    ctx->dev_free(new_cls);
    return GG_OK;
  }
  // (class, vertex index) ascending: by vertex, then stably by class
  PairLevel l{nullptr, nullptr, n_new};
  GG_TRY(ctx->dev_alloc((void **)&l.cls, n_new * sizeof(uint32_t)));
  GG_TRY(ctx->dev_alloc((void **)&l.vtx, n_new * sizeof(uint32_t)));
  GG_TRY(sort_pairs_by_key(ctx, new_vtx, new_cls, n_new, bits_for(csr->V), l.vtx, l.cls));
  if (n_classes > 1 && bits_for(n_classes) < 32) {
    GG_TRY(sort_pairs_by_key(ctx, l.cls, l.vtx, n_new, bits_for(n_classes), new_cls, new_vtx));
    std::swap(l.cls, new_cls);
    std::swap(l.vtx, new_vtx);
  } else if (n_classes > 1) {
    // more than 2^31 classes: a class index may fill 32 bits, which the radix sort does not take as one key (its
    // 0xFFFFFFFF is "no element"; a class is at most 2^32 - 2, so no class is that key).  Two stable sorts by 16-bit
    // pieces, the low one first: the sort ignores the class's high half, then the high half is a key of its own
    GG_TRY(sort_pairs_by_key(ctx, l.cls, l.vtx, n_new, REACH_CLASS_PIECE_BITS, new_cls, new_vtx));
    uint32_t *high = nullptr, *high_sorted = nullptr;
    GG_TRY(ctx->dev_alloc((void **)&high, n_new * sizeof(uint32_t)));
    GG_TRY(ctx->dev_alloc((void **)&high_sorted, n_new * sizeof(uint32_t)));
    GG_LAUNCH(ctx, "reach_class_high", k_reach_class_high, stride_grid(ctx, n_new), dim3(256), 0,
              (const uint32_t *)new_cls, (uint64_t)n_new, high);
    GG_TRY(sort_triples_by_key(ctx, high, new_cls, new_vtx, n_new, 32 - REACH_CLASS_PIECE_BITS, high_sorted, l.cls, l.vtx));
    ctx->dev_free(high_sorted);
    ctx->dev_free(high);
  }
  ctx->dev_free(new_vtx);
  ctx->dev_free(new_cls);
  *out = l;
  return GG_OK;
}

int alloc_level_columns(gg_ctx *ctx, gg_result *res) {
  for (uint64_t m : res->level_rows) res->rows[0] += m;
  for (int c = 0; c < 2; c++) {
    GG_TRY(ctx->dev_alloc((void **)&res->cols[0][c], (res->rows[0] ? res->rows[0] : 1) * sizeof(int64_t)));
    ctx->keep(res->cols[0][c]);
  }
  return GG_OK;
}

int emit_pair_levels(gg_ctx *ctx, const gg_csr *csr, const std::vector<PairLevel> &levels, gg_result *res) {
  GG_TRY(alloc_level_columns(ctx, res));
  uint64_t at = 0;
  for (const PairLevel &l : levels) {
    GG_LAUNCH(ctx, "reach_emit", k_reach_emit, stride_grid(ctx, l.n), dim3(256), 0, l.cls, l.vtx, l.n, csr->vid,
              res->cols[0][0] + at, res->cols[0][1] + at, (const unsigned long long *)ctx->dev_err);
    at += l.n;
  }
  return sync_checked(ctx);
}

int level_rows_levels(const gg_result *res, uint64_t *rows_per_level, int capacity, int *n_levels) {
  if (!n_levels || (capacity > 0 && !rows_per_level)) return GG_ERR_INVALID_ARG;
  *n_levels = (int)res->level_rows.size();
  for (int l = 0; l < capacity && l < *n_levels; l++) rows_per_level[l] = res->level_rows[l];
  return GG_OK;
}

int level_rows_fetch(const gg_result *res, uint64_t offset, uint32_t max_rows, int64_t *col0, int64_t *col1, int32_t *level,
                     uint32_t *n_out) {
  if (!n_out || !col0 || !col1) return GG_ERR_INVALID_ARG;
  GG_TRY(fetch_slice(res->ctx, res->rows[0], offset, max_rows, {{col0, res->cols[0][0]}, {col1, res->cols[0][1]}}, n_out));
  if (level) {  // the level of a row follows from the per-level row counts
    uint64_t start = 0;
    for (size_t l = 0; l < res->level_rows.size(); l++) {
      const uint64_t end = start + res->level_rows[l];
      for (uint64_t r = offset > start ? offset : start; r < end && r < offset + *n_out; r++)
        level[r - offset] = (int32_t)(l + 1);
      start = end;
    }
  }
  return GG_OK;
}

}  // namespace gg

extern "C" int gg_debug_reach_visited(gg_ctx *ctx, int mode, uint64_t hash_initial_slots) {
  if (!ctx || mode < 0 || mode > 2) return GG_ERR_INVALID_ARG;
  ctx->reach_visited_mode = mode;
  ctx->reach_hash_slots = hash_initial_slots;
  return GG_OK;
}

extern "C" int gg_reach_closure(gg_ctx *ctx, const gg_csr *csr, const int64_t *seed_ids, const uint32_t *seed_class,
                                const uint8_t *seed_seen, uint64_t n_seeds, uint32_t n_classes, gg_result **out) {
  ApiScope scope(ctx);
  if (!out || (n_seeds && (!seed_ids || !seed_class))) return GG_ERR_INVALID_ARG;
  *out = nullptr;
  GG_TRY(check_whole_csr(ctx, csr));
  if (n_seeds >= (1ull << 32)) {  // (classes: n_classes is a uint32_t, so every class index fits a key's high half)
    set_error("gg_reach_closure: %llu seeds do not fit a 32-bit seed index", (unsigned long long)n_seeds);
    return GG_ERR_TOO_LARGE;
  }
  uint64_t n_seen = 0;
  for (uint64_t i = 0; i < n_seeds; i++) {
    if (seed_class[i] >= n_classes) {
      set_error("gg_reach_closure: seed %llu has class %u of %u", (unsigned long long)i, seed_class[i], n_classes);
      return GG_ERR_INVALID_ARG;
    }
    n_seen += seed_seen && seed_seen[i];
  }
  GG_HIP(hipSetDevice(ctx->device));
  ResultOwner res = make_result(ctx, ResultKind::REACH);
  uint32_t *seed_dense = nullptr, *seed_cls = nullptr;
  uint8_t *seen = nullptr;
  GG_TRY(upload_ids(ctx, csr, seed_ids, n_seeds, &seed_dense));
  GG_TRY(ctx->dev_alloc((void **)&seed_cls, (n_seeds ? n_seeds : 1) * sizeof(uint32_t)));
  if (n_seeds) GG_HIP(hipMemcpyAsync(seed_cls, seed_class, n_seeds * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
  if (n_seen) {
    GG_TRY(ctx->dev_alloc((void **)&seen, n_seeds));
    GG_HIP(hipMemcpyAsync(seen, seed_seen, n_seeds, hipMemcpyHostToDevice, ctx->stream));
  }

  // ---- the visited set's form
  Visited vs;
  vs.V = csr->V;
  const uint64_t bits = (uint64_t)n_classes * csr->V;
  bool bitmap = ctx->reach_visited_mode == 1;
  if (ctx->reach_visited_mode == 0) {
    size_t free_bytes = 0, total_bytes = 0;
    GG_HIP(hipMemGetInfo(&free_bytes, &total_bytes));
    bitmap = bits <= REACH_BITMAP_MAX_BITS && bits / 8 <= free_bytes / 4;
  }
  std::vector<Level> levels;
  if (bitmap) {
    const uint64_t words = (bits + 31) / 32;
    GG_TRY(ctx->dev_alloc((void **)&vs.bits, (words ? words : 1) * sizeof(uint32_t)));
    GG_HIP(hipMemsetAsync(vs.bits, 0, (words ? words : 1) * sizeof(uint32_t), ctx->stream));
    if (n_seen)
      GG_LAUNCH(ctx, "reach_insert", k_reach_insert, stride_grid(ctx, n_seeds), dim3(256), 0, seed_cls, seed_dense,
                (const uint8_t *)seen, n_seeds, vs);
  } else {
    uint64_t cap = ctx->reach_hash_slots ? ctx->reach_hash_slots : std::max<uint64_t>(2 * n_seeds, REACH_MIN_SLOTS);
    cap = std::max<uint64_t>(cap, 2 * n_seen + 1);
    GG_TRY(hash_build(ctx, cap, seed_cls, seed_dense, seen, n_seeds, levels, &vs));
  }
  uint64_t visited = n_seen;  // an upper bound of the set's entries (a seen seed may repeat or be no vertex)

  uint32_t *count = nullptr;
  GG_TRY(ctx->dev_alloc((void **)&count, sizeof(uint32_t)));
  const uint32_t *fcls = seed_cls, *fvtx = seed_dense;
  uint64_t n_parent = n_seeds;
  for (int level = 1; n_parent > 0; level++) {
    uint64_t *foff = nullptr, M = 0;
    GG_TRY(frontier_offsets(ctx, csr, fvtx, n_parent, &foff, &M));
    if (M == 0) break;
    if (M >= (1ull << 32)) {
      set_error("gg_reach_closure: level %d has %llu children (2^32 or more)", level, (unsigned long long)M);
      return GG_ERR_TOO_LARGE;
    }
    // an insert must always find an empty slot; a rebuild sizes the table at twice the bound, so a closure that keeps
    // growing rebuilds every other level at most (each rebuild re-inserts every visited entry — on the 10^8-message
    // forest the rebuilds took 6.0 ms of 48 when the table grew only to the bound, 3.4 of 41 at twice it)
    if (!bitmap && vs.cap < 2 * (visited + M))
      GG_TRY(hash_build(ctx, std::max(4 * (visited + M), 2 * vs.cap), seed_cls, seed_dense, seen, n_seeds, levels, &vs));
    Level l;
    GG_TRY(expand_claim_sorted(ctx, csr, fcls, fvtx, foff, n_parent, M, vs, n_classes, count, &l));
    ctx->dev_free(foff);
    if (l.n == 0) break;
    const uint64_t n_new = l.n;
    levels.push_back(l);
    res->level_rows.push_back(n_new);
    visited += n_new;
    fcls = l.cls;
    fvtx = l.vtx;
    n_parent = n_new;
  }

  GG_TRY(emit_pair_levels(ctx, csr, levels, res.get()));
  *out = res.release();
  return GG_OK;
}

extern "C" int gg_reach_closure_levels(const gg_result *res, uint64_t *rows_per_level, int capacity, int *n_levels) {
  GG_TRY(expect_kind(res, ResultKind::REACH, "gg_reach_closure_levels"));
  return level_rows_levels(res, rows_per_level, capacity, n_levels);
}

extern "C" int gg_reach_closure_fetch(const gg_result *res, uint64_t offset, uint32_t max_rows, int64_t *seed_class,
                                      int64_t *vertex_id, int32_t *level, uint32_t *n_out) {
  GG_TRY(expect_kind(res, ResultKind::REACH, "gg_reach_closure_fetch"));
  return level_rows_fetch(res, offset, max_rows, seed_class, vertex_id, level, n_out);
}
