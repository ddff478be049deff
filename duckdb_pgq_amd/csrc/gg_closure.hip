// gg_closure.hip — walk closure: every walk from a list of seeds, level by level, to no fixed depth.
//
// Replaces the reference's PhysicalRecursiveCTE over a UNION ALL arm that joins the CTE with one table on one column
// (src/execution/operator/set/physical_recursive_cte.cpp:60-139: the recursive pipeline — a hash join whose build
// side is re-made — runs once per level until a level is empty).  The table's rows are the CSR's edges key -> next;
// a CTE row of level L is a walk of L edges from a seed; UNION ALL keeps one row per walk.
//
// Row layout: a level-L row is (seed index u32, CSR slot u32) — the slot of the walk's last edge, whose destination
// nbr[slot] is the vertex its children hang off.  So one level's rows are the next level's frontier; level 0 is the
// seeds' dense ids.  Per level:
//   k_closure_deg     degree of every row's end vertex (a gather of off[v], off[v+1])
//   scan              exclusive prefix of the degrees (scan_exclusive_u64; the total is the one 8-byte read per level)
//   tile_partition    the entry each tile of XT children starts in (make_tiles_u64)
//   k_closure_expand  one thread per child: locate its parent in the tile's window of offsets, write (seed, slot)
// The expansion balances on children, so a hub row of 10^5 children spreads over 400 workgroups instead of one wave.
// Order: by level; inside a level by parent row, then by CSR order inside the parent's vertex row.
// k_closure_emit finally writes the int64 (seed index, edge rowid) columns a fetch reads.
#include "gg_internal.h"

using namespace gg;

namespace {

// parent i of the current level: the end vertex of its walk (INVALID_U32: a seed that is not a vertex)
__device__ __forceinline__ uint32_t parent_vertex(const uint32_t *__restrict__ seed_dense, const uint2 *__restrict__ prow,
                                                  const uint32_t *__restrict__ nbr, uint64_t i) {
  return seed_dense ? seed_dense[i] : nbr[prow[i].y];
}

__global__ __launch_bounds__(256) void k_closure_deg(const uint32_t *__restrict__ off, const uint32_t *__restrict__ nbr,
                                                     const uint32_t *__restrict__ seed_dense,
                                                     const uint2 *__restrict__ prow, uint64_t n,
                                                     uint64_t *__restrict__ deg) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t v = parent_vertex(seed_dense, prow, nbr, i);
    deg[i] = v == INVALID_U32 ? 0 : (uint64_t)(off[v + 1] - off[v]);
  }
}

__global__ __launch_bounds__(XT) void k_closure_expand(const uint32_t *__restrict__ off, const uint32_t *__restrict__ nbr,
                                                       const uint32_t *__restrict__ seed_dense,
                                                       const uint2 *__restrict__ prow, const uint64_t *__restrict__ foff,
                                                       uint64_t n_entries, uint64_t M,
                                                       const uint32_t *__restrict__ tile_entry, uint2 *__restrict__ out) {
  __shared__ uint64_t s_foff[XT + 1];
  const uint64_t p = (uint64_t)blockIdx.x * XT + threadIdx.x;  // foff[0] == 0: an exclusive scan
  const uint64_t i0 = tile_entry[blockIdx.x];
  load_window(s_foff, foff, n_entries, i0);
  __syncthreads();
  if (p >= M) return;
  uint64_t k;
  const uint64_t i = locate_entry(s_foff, foff, n_entries, i0, p, &k);
  const uint32_t v = parent_vertex(seed_dense, prow, nbr, i);
  const uint32_t seed = seed_dense ? (uint32_t)i : prow[i].x;
  out[p] = make_uint2(seed, off[v] + (uint32_t)k);
}

// rows of one level -> the result's int64 columns at their offset
__global__ __launch_bounds__(256) void k_closure_emit(const uint2 *__restrict__ rows, uint64_t n,
                                                      const int64_t *__restrict__ eid, const uint32_t *__restrict__ epos,
                                                      int64_t *__restrict__ seed_out, int64_t *__restrict__ rowid_out,
                                                      const unsigned long long *__restrict__ err) {
  if (*err) return;  // a level's rows were placed by the offsets of a chained scan: not valid once one gave up
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (uint64_t)gridDim.x * blockDim.x) {
    const uint2 row = rows[r];
    seed_out[r] = (int64_t)row.x;
    rowid_out[r] = eid ? eid[row.y] : (int64_t)epos[row.y];
  }
}

}  // namespace

extern "C" int gg_walk_closure(gg_ctx *ctx, const gg_csr *csr, const int64_t *seed_ids, uint64_t n_seeds,
                               int max_levels, gg_result **out) {
  ApiScope scope(ctx);
  if (!out || (!seed_ids && n_seeds)) return GG_ERR_INVALID_ARG;
  *out = nullptr;
  GG_TRY(check_whole_csr(ctx, csr));
  if (!csr->has_rowid) {
    set_error("gg_walk_closure: the CSR was built without edge rowids (gg_ctx_set_edge_rowid(ctx, 1))");
    return GG_ERR_STATE;
  }
  if (n_seeds >= INVALID_U32) {
    set_error("gg_walk_closure: %llu seeds do not fit a 32-bit seed index", (unsigned long long)n_seeds);
    return GG_ERR_TOO_LARGE;
  }
  GG_HIP(hipSetDevice(ctx->device));
  ResultOwner res = make_result(ctx, ResultKind::WALK_CLOSURE);
  uint32_t *seed_dense = nullptr;
  GG_TRY(upload_ids(ctx, csr, seed_ids, n_seeds, &seed_dense));

  std::vector<uint2 *> levels;  // levels[L - 1]: the rows of level L
  const uint2 *prow = nullptr;
  uint64_t n_parent = n_seeds;
  for (int level = 1; n_parent > 0 && (max_levels < 0 || level <= max_levels); level++) {
    uint64_t *foff = nullptr, M = 0;
    GG_TRY(ctx->dev_alloc((void **)&foff, (n_parent + 1) * sizeof(uint64_t)));
    const uint32_t *dense = level == 1 ? seed_dense : nullptr;
    GG_LAUNCH(ctx, "closure_deg", k_closure_deg, stride_grid(ctx, n_parent), dim3(256), 0, csr->off, csr->nbr, dense,
              prow, n_parent, foff);
    GG_TRY(offsets_from_deg(ctx, foff, n_parent, &M));
    if (M == 0) break;
    if (M >= (1ull << 32)) {
      set_error("gg_walk_closure: level %d holds %llu walks (2^32 or more)", level, (unsigned long long)M);
      return GG_ERR_TOO_LARGE;
    }
    if (max_levels < 0 && (uint64_t)level > csr->V) {
      // a walk of V + 1 edges visits some vertex twice: the recursion would never reach an empty level
      set_error("gg_walk_closure: level %d is not empty, so a walk repeats a vertex (a cycle is reachable from a seed); "
                "an unbounded recursion over it never ends — bound the levels", level);
      return GG_ERR_STATE;
    }
    uint32_t *tile_entry = nullptr;
    uint64_t n_tiles = 0;
    GG_TRY(make_tiles_u64(ctx, foff, n_parent, M, &tile_entry, &n_tiles));
    uint2 *rows = nullptr;
    GG_TRY(ctx->dev_alloc((void **)&rows, M * sizeof(uint2)));
    GG_LAUNCH(ctx, "closure_expand", k_closure_expand, dim3((unsigned)n_tiles), dim3(XT), 0, csr->off, csr->nbr, dense,
              prow, foff, n_parent, M, tile_entry, rows);
    ctx->dev_free(tile_entry);
    ctx->dev_free(foff);
    levels.push_back(rows);
    res->level_rows.push_back(M);
    prow = rows;
    n_parent = M;
  }

  GG_TRY(alloc_level_columns(ctx, res.get()));
  uint64_t at = 0;
  for (size_t l = 0; l < levels.size(); l++) {
    const uint64_t m = res->level_rows[l];
    GG_LAUNCH(ctx, "closure_emit", k_closure_emit, stride_grid(ctx, m), dim3(256), 0, levels[l], m, csr->eid, csr->epos,
              res->cols[0][0] + at, res->cols[0][1] + at, (const unsigned long long *)ctx->dev_err);
    at += m;
  }
  GG_TRY(sync_checked(ctx));
  *out = res.release();
  return GG_OK;
}

extern "C" int gg_walk_closure_levels(const gg_result *res, uint64_t *rows_per_level, int capacity, int *n_levels) {
  GG_TRY(expect_kind(res, ResultKind::WALK_CLOSURE, "gg_walk_closure_levels"));
  return level_rows_levels(res, rows_per_level, capacity, n_levels);
}

extern "C" int gg_walk_closure_fetch(const gg_result *res, uint64_t offset, uint32_t max_rows, int64_t *seed_index,
                                     int64_t *edge_rowid, int32_t *level, uint32_t *n_out) {
  GG_TRY(expect_kind(res, ResultKind::WALK_CLOSURE, "gg_walk_closure_fetch"));
  return level_rows_fetch(res, offset, max_rows, seed_index, edge_rowid, level, n_out);
}
