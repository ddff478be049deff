// gg_group.hip — GROUP BY one column of a materialised walk table: count(*) and sum(weight) per key, as an aggregate result.
//
// The reference's LDBC statements end their join chains in a grouped aggregate over a column of the joined rows
// (benchmark/ldbc/queries/interactive-complex-4.sql:1-22 and interactive-complex-6.sql:1-22: knows [-> knows] -> message ->
// message_tag under count(*) GROUP BY tag; interactive-complex-5.sql: by forum; bi-8.sql:41-53: a score summed per person).
// There that is PhysicalHashAggregate (src/execution/operator/aggregate/physical_hash_aggregate.cpp:152-266,
// GroupedAggregateHashTable::FindOrCreateGroups, src/execution/aggregate_hashtable.cpp:367-504) fed by the last hash join's
// ScanStructure::NextInnerJoin (src/execution/join_hashtable.cpp:442-476).  Here the rows are in HBM already
// (gg_expand_khop_result, gg_result_filter_edge, gg_result_extend_edge) and the key's table is a CSR of the same context:
// the group of a row is the dense index of its key cell, so the "hash table" is an array of V cells and needs no insert.
//   k_group_accum   one thread per input row and tile pass: the key cell, one dictionary probe; with weights a second cell,
//                   a second probe and one 8-byte gather.  Lanes of a wavefront that hold the same key in adjacent rows
//                   are combined first: one ballot finds the run heads, the run's count is its length, its 128-bit sum a
//                   segmented suffix sum by shuffles; the head lane alone adds
//                     LDS     to the workgroup's private table in LDS (LDS atomics); after its last tile the workgroup adds
//                             every non-zero cell to the global cells, one global atomic per cell and workgroup
//                     GLOBAL  to the global cells
//                   A workgroup takes tiles of GRP_TILE_ROWS consecutive rows by a grid stride.
//   k_group_flag    per key: has it a group (count != 0)?  + the groups' rows
//   scan            exclusive prefix of the flags: the groups' places, their number
//   k_group_write   (vertex id, walks, lo, hi) of every group at its place: ascending dense index
// The 128-bit sum from 64-bit atomics: a row's weight w is the pair (lo = w, hi = w >> 63).  lo is added to the low cell
// with a RETURNING atomic; the add carried iff (old + lo) mod 2^64 < lo, and hi + that carry is added to the high cell
// (atomic_add128, gg_walk_table.h).
// The atomics on one cell are applied in some serial order, and along it the low cell runs through the partial sums of
// the low words mod 2^64: it wraps once each time the exact partial sum passes a multiple of 2^64, so the carries counted
// are floor(exact sum of the low words / 2^64) whatever the order, and the high cell ends as the sum of the high words
// plus that — the sum mod 2^128.  The same holds one level up: a workgroup's LDS cell pair is a 128-bit partial sum, and
// its flush adds that pair to the global pair by the same two steps.  Integer addition mod 2^64 and mod 2^128 is
// commutative and associative: both routes, every grid and every arrival order give the same bits.  No floating point.
// Bytes (model): per input row 8 B of key cell + one 16-byte dictionary slot, with weights 8 B + 16 B + 8 B more (one cell
// and slot fewer if key and weight are the same column of the same CSR); atomics: one per run and wavefront (count form),
// two with weights.  Per key: 8 B (24 B with weights) zeroed, read twice (flag, write), 4 B of flag written, scanned and
// read, and 32 B written per group; on the LDS route 8 / 24 B of global atomics per non-zero cell and workgroup.
#include "gg_internal.h"
#include "gg_walk_table.h"

using namespace gg;

namespace gg {
namespace {

constexpr uint32_t GRP_TILE_ROWS = 1024;  // input rows a workgroup takes per pass: 4 per lane
// The workgroup-private table: 48 KiB of the CU's 160 KiB of LDS, so three workgroups (12 wavefronts, 3 per SIMD) share
// a CU — the probe and the gather are dependent loads and want the other waves to hide behind.
constexpr uint32_t GRP_LDS_BYTES = 48 * 1024;
constexpr uint32_t GRP_WG_PER_CU_LDS = 3, GRP_WG_PER_CU_GLOBAL = 8;

struct GroupCell {  // the global state of a key with weights: 24 bytes
  unsigned long long cnt, lo, hi;
};

struct GroupArgs {
  const int64_t *key_cells;  // the key column
  uint64_t n_rows;
  DictView key;             // the key table's dictionary
  ValueColumn w;            // the weight column (cells null: the count form), its table's dictionary and the weights;
                            // dict.ht null: no vertex at all, or unused because of same_cell
  int same_cell;            // the weight cell is the key cell and its CSR the key's: the key's dense index serves
  uint32_t V;               // keys
  unsigned long long *cnt;  // count form: V u64
  GroupCell *cell;          // weighted form: V cells
};

// Both tables are indexed by dense key.  LDS layout: cnt[V], then lo[V], hi[V] with weights.
template <bool LDS, bool WEIGHTED>
__global__ __launch_bounds__(256) void k_group_accum(GroupArgs A) {
  extern __shared__ __align__(16) unsigned long long s_tab[];
  const int lane = threadIdx.x & 63;
  if (LDS) {
    const uint32_t words = A.V * (WEIGHTED ? 3u : 1u);
    for (uint32_t i = threadIdx.x; i < words; i += 256) s_tab[i] = 0;
    __syncthreads();
  }
  const uint64_t n_tiles = (A.n_rows + GRP_TILE_ROWS - 1) / GRP_TILE_ROWS;
  for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
#pragma unroll
    for (uint32_t j = 0; j < GRP_TILE_ROWS / 256; j++) {
      const uint64_t r = t * GRP_TILE_ROWS + j * 256u + threadIdx.x;
      uint32_t u = INVALID_U32;
      uint64_t lo = 0, hi = 0;
      if (r < A.n_rows) {
        const int64_t cell = A.key_cells[r];
        u = A.key.lookup(cell);
        if (WEIGHTED && u != INVALID_U32) {  // (a row without a group needs no weight)
          uint32_t wv = INVALID_U32;
          if (A.same_cell)
            wv = u;
          else if (A.w.dict.ht)
            wv = A.w.dict.lookup(A.w.cells[r]);
          if (wv != INVALID_U32) {  // (wv < V(weight_csr): the weights have that many entries)
            const int64_t w = A.w.values[wv];
            lo = (uint64_t)w, hi = (uint64_t)(w >> 63);
          }
        }
      }
      // runs of equal keys in adjacent lanes: lane l heads one iff its key differs from lane l - 1's
      const uint32_t prev = (uint32_t)__shfl_up((int)u, 1, 64);
      const uint64_t heads = __ballot(lane == 0 || prev != u);
      const int end = run_end(heads, lane);  // one past the last lane of this lane's run
      if (WEIGHTED) {  // segmented suffix sums: lane l ends with the sum over [l, end)
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const uint64_t blo = __shfl_down((unsigned long long)lo, d, 64), bhi = __shfl_down((unsigned long long)hi, d, 64);
          if (lane + d < end) add128(lo, hi, blo, bhi);
        }
      }
      if (((heads >> lane) & 1) && u != INVALID_U32) {  // (u < V: a dense index of key_csr)
        const unsigned long long cnt = (unsigned long long)(end - lane);
        if (LDS) {
          atomicAdd(&s_tab[u], cnt);
          if (WEIGHTED) atomic_add128(&s_tab[A.V + u], &s_tab[2u * A.V + u], lo, hi);
        } else if (WEIGHTED) {
          atomicAdd(&A.cell[u].cnt, cnt);
          atomic_add128(&A.cell[u].lo, &A.cell[u].hi, lo, hi);
        } else {
          atomicAdd(&A.cnt[u], cnt);
        }
      }
    }
  }
  if (LDS) {
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < A.V; k += 256) {
      const unsigned long long cnt = s_tab[k];
      if (!cnt) continue;  // (no row of this workgroup had the key: its sums are 0 too)
      if (WEIGHTED) {
        atomicAdd(&A.cell[k].cnt, cnt);
        atomic_add128(&A.cell[k].lo, &A.cell[k].hi, s_tab[A.V + k], s_tab[2u * A.V + k]);
      } else {
        atomicAdd(&A.cnt[k], cnt);
      }
    }
  }
}

__device__ __forceinline__ uint64_t group_count(const unsigned long long *__restrict__ cnt,
                                                const GroupCell *__restrict__ cell, uint64_t v) {
  return cell ? cell[v].cnt : cnt[v];
}

// flag[v] = key v has a group; *grouped += the groups' rows
__global__ __launch_bounds__(256) void k_group_flag(const unsigned long long *__restrict__ cnt,
                                                    const GroupCell *__restrict__ cell, uint64_t V,
                                                    uint32_t *__restrict__ flag, unsigned long long *__restrict__ grouped) {
  __shared__ uint64_t s_red[4];
  uint64_t acc = 0;
  for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t c = group_count(cnt, cell, v);
    flag[v] = c != 0 ? 1u : 0u;
    acc += c;
  }
  acc = wave_reduce_add_u64(acc);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint64_t all = s_red[0] + s_red[1] + s_red[2] + s_red[3];
    if (all) atomicAdd(grouped, (unsigned long long)all);
  }
}

// pos: the exclusive prefix of the flags; the columns have `slots` entries (>= the number of groups)
__global__ __launch_bounds__(256) void k_group_write(const unsigned long long *__restrict__ cnt,
                                                     const GroupCell *__restrict__ cell, uint64_t V,
                                                     const uint32_t *__restrict__ pos, uint64_t slots,
                                                     const int64_t *__restrict__ vid, int64_t *__restrict__ out_id,
                                                     int64_t *__restrict__ out_walks, int64_t *__restrict__ out_lo,
                                                     int64_t *__restrict__ out_hi) {
  for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t c = group_count(cnt, cell, v);
    if (!c) continue;
    const uint32_t p = pos[v];
    if (p >= slots) continue;  // (cannot happen: groups <= min(V, rows) = slots)
    out_id[p] = vid[v];
    out_walks[p] = (int64_t)c;
    out_lo[p] = (int64_t)(cell ? cell[v].lo : c);
    out_hi[p] = cell ? (int64_t)cell[v].hi : 0;
  }
}

}  // namespace
}  // namespace gg

extern "C" int gg_result_group_by(gg_ctx *ctx, const gg_result *res, int hops, int key_col, const gg_csr *key_csr_c,
                                  int weight_col, const gg_csr *weight_csr_c, const int64_t *weights,
                                  gg_group_stats *stats, gg_result **out_result) {
  if (out_result) *out_result = nullptr;
  if (stats) memset(stats, 0, sizeof(*stats));
  const char *fn = "gg_result_group_by";
  GG_TRY(result_arg(fn, ctx, res));
  GG_TRY(csr_arg(fn, ctx, key_csr_c));
  if (!weight_csr_c) weight_csr_c = key_csr_c;
  GG_TRY(csr_arg(fn, ctx, weight_csr_c));
  if (!stats && !out_result) {
    set_error("%s: neither stats nor out_result is asked for", fn);
    return GG_ERR_INVALID_ARG;
  }
  GG_TRY(whole_csr(fn, key_csr_c, "the key's table"));
  GG_TRY(whole_csr(fn, weight_csr_c, "the weight's table"));
  GG_TRY(walk_kind_arg(fn, res, KindRule::STATE));
  GG_TRY(hops_arg(fn, res, hops));
  GG_TRY(column_arg(fn, "key", key_col, 0, hops));
  GG_TRY(column_arg(fn, "weight", weight_col, -1, hops));
  if ((weight_col >= 0) != (weights != nullptr)) {
    set_error("%s: weights go with a weight column, and only with one", fn);
    return GG_ERR_INVALID_ARG;
  }
  ApiScope scope(ctx);
  GG_HIP(hipSetDevice(ctx->device));
  gg_csr *kcsr = const_cast<gg_csr *>(key_csr_c), *wcsr = const_cast<gg_csr *>(weight_csr_c);
  const bool weighted = weight_col >= 0;
  const uint64_t n_rows = res->rows[hops], V = kcsr->V;
  ResultOwner o;
  if (out_result) o = make_result(ctx, ResultKind::AGGREGATE, hops, hops);
  uint64_t words_host[2] = {0, 0};  // groups, rows grouped
  uint32_t route = 0;
  const int id_cols[2] = {key_col, weight_col};  // (weight_col -1: none)
  GG_TRY(id_columns_present(fn, res, hops, id_cols, 2));
  if (n_rows && V) {
    hipStream_t st = ctx->stream;
    GroupArgs A{};
    A.key_cells = res->cols[hops][key_col];
    A.n_rows = n_rows;
    GG_TRY(dict_view(ctx, kcsr, &A.key));
    A.V = (uint32_t)V;  // (a CSR has fewer than 2^32 vertices)
    if (weighted) {
      A.same_cell = wcsr == kcsr && weight_col == key_col;  // (then the weight table's dictionary is never asked)
      GG_TRY(value_column(ctx, wcsr, res->cols[hops][weight_col], weights, nullptr, &A.w));
    }
    const size_t key_bytes = weighted ? sizeof(GroupCell) : sizeof(unsigned long long);
    void *state = nullptr;
    GG_TRY(ctx->dev_alloc(&state, V * key_bytes));
    GG_HIP(hipMemsetAsync(state, 0, V * key_bytes, st));
    if (weighted) A.cell = (GroupCell *)state; else A.cnt = (unsigned long long *)state;
    uint64_t *words = nullptr;
    GG_TRY(ctx->dev_alloc((void **)&words, sizeof(words_host)));
    GG_HIP(hipMemsetAsync(words, 0, sizeof(words_host), st));

    // the route: the LDS table wherever the keys fit it, unless the global cells are forced
    uint64_t lds_keys = GRP_LDS_BYTES / key_bytes;
    if (ctx->group_lds_keys && ctx->group_lds_keys < lds_keys) lds_keys = ctx->group_lds_keys;
    route = ctx->group_route != 2 && V <= lds_keys ? 1 : 2;
    const uint64_t n_tiles = (n_rows + GRP_TILE_ROWS - 1) / GRP_TILE_ROWS;
    uint64_t grid = (uint64_t)ctx->num_cus * (route == 1 ? GRP_WG_PER_CU_LDS : GRP_WG_PER_CU_GLOBAL);
    if (ctx->max_grid_tiles && ctx->max_grid_tiles < grid) grid = ctx->max_grid_tiles;
    if (n_tiles < grid) grid = n_tiles;
    const size_t lds = route == 1 ? V * key_bytes : 0;
    if (route == 1 && weighted)
      GG_LAUNCH(ctx, "k_group_accum_lds_sum", (k_group_accum<true, true>), dim3((unsigned)grid), dim3(256), lds, A);
    else if (route == 1)
      GG_LAUNCH(ctx, "k_group_accum_lds", (k_group_accum<true, false>), dim3((unsigned)grid), dim3(256), lds, A);
    else if (weighted)
      GG_LAUNCH(ctx, "k_group_accum_sum", (k_group_accum<false, true>), dim3((unsigned)grid), dim3(256), 0, A);
    else
      GG_LAUNCH(ctx, "k_group_accum", (k_group_accum<false, false>), dim3((unsigned)grid), dim3(256), 0, A);

    uint32_t *flag = nullptr;
    GG_TRY(ctx->dev_alloc((void **)&flag, V * sizeof(uint32_t)));
    const dim3 vgrid = stride_grid(ctx, V);
    GG_LAUNCH(ctx, "k_group_flag", k_group_flag, vgrid, dim3(256), 0, (const unsigned long long *)A.cnt,
              (const GroupCell *)A.cell, V, flag, (unsigned long long *)(words + 1));
    GG_TRY(scan_exclusive_u32(ctx, flag, flag, V, words));
    if (o) {
      // a level has at most min(V, rows) groups; their number stays on the device until the call's one read-back
      const uint64_t slots = V < n_rows ? V : n_rows;
      GG_TRY(alloc_kept_columns(ctx, o->cols[hops], 4, slots));
      GG_LAUNCH(ctx, "k_group_write", k_group_write, vgrid, dim3(256), 0, (const unsigned long long *)A.cnt,
                (const GroupCell *)A.cell, V, (const uint32_t *)flag, slots, (const int64_t *)kcsr->vid, o->cols[hops][0],
                o->cols[hops][1], o->cols[hops][2], o->cols[hops][3]);
    }
    GG_TRY(read_back(ctx, {{words, sizeof(words_host), words_host}}));
  }
  if (stats) {
    stats->rows_in = n_rows, stats->rows_grouped = words_host[1], stats->groups = words_host[0];
    stats->route = route;
  }
  if (o) {
    o->rows[hops] = words_host[0];
    *out_result = o.release();
  }
  return GG_OK;
}

extern "C" int gg_debug_group(gg_ctx *ctx, int route, uint32_t lds_keys) {
  if (!ctx || route < 0 || route > 2) return GG_ERR_INVALID_ARG;
  ctx->group_route = route;
  ctx->group_lds_keys = lds_keys;
  return GG_OK;
}
