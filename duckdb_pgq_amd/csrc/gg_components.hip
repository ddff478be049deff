// gg_components.hip — weakly connected components: a label and a size per vertex, a row per component.
//
// The reference answers "which vertices hang together" with a UNION recursive CTE under an aggregate,
//     WITH RECURSIVE cc(v, root) AS (SELECT id, id FROM person UNION SELECT u.b, cc.root FROM cc, und u WHERE cc.v = u.a)
//     SELECT v, min(root), count(*) FROM cc GROUP BY v
// PhysicalRecursiveCTE (src/execution/operator/set/physical_recursive_cte.cpp:47-139) re-runs the arm's hash join once per
// level and probes sum |component|^2 rows against one GroupedAggregateHashTable (src/execution/aggregate_hashtable.cpp:367-504)
// before PhysicalHashAggregate (src/execution/operator/aggregate/physical_hash_aggregate.cpp:152-266) folds them: quadratic
// in the giant component.  Here it is one pass over the edge entries with a lock-free union-find:
//   parent[v]      V x u32, the forest; a root is a cell that holds its own index
//   k_cc_init      parent[v] = v.  (Starting a vertex under its first out-neighbour of smaller index instead was built and
//                  measured: slower on knows at SF10 and SF100 and 9x slower on a forest with a hub, whose row one thread
//                  walks — DESIGN.md 4.16 — so init_mode 0 and 1 are the same start now)
//   k_cc_hook      one thread per edge entry (u, v), whichever COO pair the build left — direction does not matter, so the
//                  reverse pair serves as well as the forward one: find both roots with path halving, link the larger root
//                  under the smaller with one CAS, continue from the CAS's answer on failure.  One launch, no host round trip
//   k_cc_jump      next[v] = cur[cur[v]] between two arrays, one launch per doubling, until a launch changes nothing
//   k_cc_size      size[root[v]] += 1, a wave whose lanes all hold one root adds its popcount once
//   k_cc_flag      flag[v] = (root[v] == v), with the largest size and the number of sizes of 1 reduced per wave
//   k_cc_rows      table 0, a gather: id(v), id(root[v]), size[root[v]]
//   scan, k_cc_reps   table 1, placed by count, scan, write: one row (id(r), size[r]) per root r in dense-index order
// Bytes (model): 8 E for the entries + 12 V per jump launch (4 B read, 4 B gathered, 4 B written) + 28 V for sizes and
// table 0 (4 B root, 8 B id, 2 x 8 B written ...; DESIGN.md 4.16 has the terms).  The random traffic is on parent: 4 V bytes.
#include "gg_internal.h"

using namespace gg;

namespace gg {
namespace {

constexpr uint32_t CC_JUMPS_PER_CHECK = 4;  // default: pointer-doubling launches per look at the changed word

// device words of one call
enum { CC_HOOKS = 0, CC_CHANGED, CC_COMPONENTS, CC_LARGEST, CC_SINGLETONS, CC_WORDS = 8 };

__device__ __forceinline__ uint32_t cc_load(const uint32_t *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void cc_store(uint32_t *p, uint32_t x) {
  __hip_atomic_store(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void k_cc_init(uint64_t V, uint32_t *__restrict__ parent) {
  for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (uint64_t)gridDim.x * blockDim.x)
    parent[v] = (uint32_t)v;
}

// The root of x as far as this thread can see it, halving the path on the way: every cell left behind is pointed at its
// grandparent.  The value returned is an ancestor of x that held its own index when it was read.
__device__ __forceinline__ uint32_t cc_find(uint32_t *parent, uint32_t x) {
  uint32_t p = cc_load(&parent[x]);
  while (p != x) {
    const uint32_t gp = cc_load(&parent[p]);  // (p <= x < V)
    if (gp == p) return p;
    cc_store(&parent[x], gp);  // x is no root (p != x) and never becomes one again, so this never races with a CAS on x
    x = gp;
    p = cc_load(&parent[x]);
  }
  return x;
}

// Lock-free union-find over the edge entries.  Three things hold, and the kernel is correct because of them:
// 1. Every value ever stored into parent[x] is <= x and lies in x's tree (it was, when read, an ancestor of x, and trees only
//    ever merge): the CAS stores lo < hi, halving stores a grandparent, the initial value is x.
//    Indices strictly decrease along every walk, so a walk from x ends after at most x steps whatever the other threads do,
//    and a tree's root is its smallest member: once every entry has been through here the root of a component is its
//    smallest dense index under every interleaving.  No thread waits for another — no spin on another workgroup's
//    progress, no flag, no ticket; an entry is tried again only after somebody else's CAS has succeeded on its root, and
//    each cell loses its root status at most once.
// 2. While this kernel runs, parent cells are read with relaxed agent-scope atomic loads only and written only by
//    agent-scope atomics (the CAS; a relaxed atomic store for halving).  A plain load may be served from a stale L1 line
//    or be kept in a register across the loop; a stale value is still an ancestor, so the answer does not hinge on it, but
//    the end of a walk that keeps re-reading a stale self-pointer does.  What settles "hi is a root" is the CAS on the
//    cell itself, never a load.
// 3. hooks is counted per wave: one ballot of the lanes whose CAS succeeded, one add per wave at the end — never an atomic
//    per lane.
// erow / enbr: either COO pair of the CSR; erow == nullptr: the entry's row is searched in off (V + 1 offsets).
__global__ __launch_bounds__(256) void k_cc_hook(const uint32_t *__restrict__ erow, const uint32_t *__restrict__ enbr,
                                                 const uint32_t *__restrict__ off, uint64_t V, uint64_t E,
                                                 uint32_t *parent, unsigned long long *__restrict__ hooks) {
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  uint32_t wave_hooks = 0;  // wave-uniform
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < E; base += nthreads) {
    const uint64_t i = base + (threadIdx.x & 63);
    bool hooked = false;
    if (i < E) {
      uint32_t u;
      if (erow) {
        u = erow[i];
      } else {  // the last row whose offset is <= i
        uint64_t lo = 0, hi = V;
        while (hi - lo > 1) {
          const uint64_t mid = (lo + hi) >> 1;
          if (off[mid] <= i) lo = mid; else hi = mid;
        }
        u = (uint32_t)lo;
      }
      uint32_t v = enbr[i];  // (u, v < V: dense indices of a built CSR)
      while (u != v) {
        u = cc_find(parent, u);
        v = cc_find(parent, v);
        if (u == v) break;
        const uint32_t hi = u > v ? u : v, lo = u > v ? v : u;
        const uint32_t old = atomicCAS(&parent[hi], hi, lo);  // device scope
        if (old == hi) {
          hooked = true;
          break;
        }
        u = old, v = lo;  // hi was hooked by somebody else in the meantime: go on from where it points (old < hi)
      }
    }
    wave_hooks += (uint32_t)__popcll(__ballot(hooked));
  }
  if ((threadIdx.x & 63) == 0 && wave_hooks) atomicAdd(hooks, (unsigned long long)wave_hooks);
}

// one doubling: next[v] = cur[cur[v]]; cur is only read and next only written, so a launch is deterministic.  changed
// (nullable) += the cells whose value moved.
__global__ __launch_bounds__(256) void k_cc_jump(const uint32_t *__restrict__ cur, uint64_t V, uint32_t *__restrict__ next,
                                                 unsigned long long *__restrict__ changed) {
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  uint32_t wave_changed = 0;
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < V; base += nthreads) {
    const uint64_t v = base + (threadIdx.x & 63);
    bool moved = false;
    if (v < V) {
      const uint32_t p = cur[v], gp = cur[p];  // (p <= v < V)
      next[v] = gp;
      moved = gp != p;
    }
    wave_changed += (uint32_t)__popcll(__ballot(moved));
  }
  if (changed && (threadIdx.x & 63) == 0 && wave_changed) atomicAdd(changed, (unsigned long long)wave_changed);
}

// size[root[v]] += 1.  fold: a wave whose active lanes all hold the same root issues one add of their number (on a graph
// with a giant component almost every wave is such a wave); a mixed wave adds per lane.  Integer sums: any order.
__global__ __launch_bounds__(256) void k_cc_size(const uint32_t *__restrict__ root, uint64_t V, int fold,
                                                 uint32_t *__restrict__ size) {
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < V; base += nthreads) {
    const uint64_t v = base + (threadIdx.x & 63);
    const bool in = v < V;
    const uint32_t r = in ? root[v] : 0;  // (r <= v < V)
    const uint64_t live = __ballot(in);   // (lane 0 of the wave is in: base < V)
    const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)r);
    if (fold && __ballot(in && r == first) == live) {
      if ((threadIdx.x & 63) == 0) atomicAdd(&size[first], (uint32_t)__popcll(live));
    } else if (in) {
      atomicAdd(&size[r], 1u);
    }
  }
}

// flag[v] = 1 for a root; the largest size and the number of roots of size 1, reduced per wave
__global__ __launch_bounds__(256) void k_cc_flag(const uint32_t *__restrict__ root, const uint32_t *__restrict__ size,
                                                 uint64_t V, uint32_t *__restrict__ flag,
                                                 unsigned long long *__restrict__ largest,
                                                 unsigned long long *__restrict__ singletons) {
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  uint32_t big = 0, ones = 0;
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < V; base += nthreads) {
    const uint64_t v = base + (threadIdx.x & 63);
    uint32_t s = 0;
    if (v < V) {
      const bool is_root = root[v] == v;
      flag[v] = is_root ? 1u : 0u;
      if (is_root) s = size[v];
    }
    big = s > big ? s : big;
    ones += (uint32_t)__popcll(__ballot(s == 1));  // wave-uniform
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t other = (uint32_t)__shfl_xor((int)big, o, 64);
    big = other > big ? other : big;
  }
  if ((threadIdx.x & 63) == 0) {
    if (big) atomicMax(largest, (unsigned long long)big);
    if (ones) atomicAdd(singletons, (unsigned long long)ones);
  }
}

__global__ __launch_bounds__(256) void k_cc_rows(const uint32_t *__restrict__ root, const uint32_t *__restrict__ size,
                                                 const int64_t *__restrict__ vid, uint64_t V, int64_t *__restrict__ out_id,
                                                 int64_t *__restrict__ out_comp, int64_t *__restrict__ out_size) {
  for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t r = root[v];  // (r < V)
    out_id[v] = vid[v];
    out_comp[v] = vid[r];
    out_size[v] = (int64_t)size[r];
  }
}

// pos: the exclusive prefix of the root flags (pos[r] < number of components = the columns' length)
__global__ __launch_bounds__(256) void k_cc_reps(const uint32_t *__restrict__ root, const uint32_t *__restrict__ size,
                                                 const uint32_t *__restrict__ pos, const int64_t *__restrict__ vid,
                                                 uint64_t V, int64_t *__restrict__ out_comp, int64_t *__restrict__ out_size) {
  for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (uint64_t)gridDim.x * blockDim.x)
    if (root[v] == v) {
      out_comp[pos[v]] = vid[v];
      out_size[pos[v]] = (int64_t)size[v];
    }
}

}  // namespace
}  // namespace gg

extern "C" int gg_components(gg_ctx *ctx, const gg_csr *csr, gg_cc_stats *stats, gg_result **out_result) {
  if (out_result) *out_result = nullptr;
  if (stats) memset(stats, 0, sizeof(*stats));
  if (!stats && !out_result) {
    set_error("gg_components: neither stats nor out_result is asked for");
    return GG_ERR_INVALID_ARG;
  }
  GG_TRY(check_whole_csr(ctx, csr));
  ApiScope scope(ctx);
  GG_HIP(hipSetDevice(ctx->device));
  const uint64_t V = csr->V, E = csr->E;
  ResultOwner res;
  if (out_result) res = make_result(ctx, ResultKind::COMPONENTS);
  if (V) {
    hipStream_t st = ctx->stream;
    unsigned long long *words = nullptr;
    GG_TRY(ctx->dev_alloc((void **)&words, CC_WORDS * sizeof(uint64_t)));
    GG_HIP(hipMemsetAsync(words, 0, CC_WORDS * sizeof(uint64_t), st));
    uint32_t *buf[2] = {nullptr, nullptr}, *size = nullptr;
    for (int b = 0; b < 2; b++) GG_TRY(ctx->dev_alloc((void **)&buf[b], V * sizeof(uint32_t)));
    GG_TRY(ctx->dev_alloc((void **)&size, V * sizeof(uint32_t)));
    GG_HIP(hipMemsetAsync(size, 0, V * sizeof(uint32_t), st));
    const dim3 vgrid = stride_grid(ctx, V);

    GG_LAUNCH(ctx, "cc_init", k_cc_init, vgrid, dim3(256), 0, V, buf[0]);
    if (E) {
      // whichever COO pair the build left: (row, nbr) of the multi-pass build, (rrow, rnbr) of the bucketed one
      const uint32_t *erow = csr->row, *enbr = csr->nbr;
      // (a derived build: roff == off, so the row index is the row of every FORWARD entry as well, and no reverse rows are
      // needed; it is expanded from the offsets here if nobody asked for it before)
      if (!erow && csr->rev_derived) {
        GG_TRY(ensure_reverse_index(ctx, const_cast<gg_csr *>(csr)));
        erow = csr->rrow_index;
      } else if (!erow && csr->rrow_index && csr->rnbr_rows) {
        erow = csr->rrow_index, enbr = csr->rnbr_rows;
      }
      GG_LAUNCH(ctx, "cc_hook", k_cc_hook, stride_grid(ctx, E), dim3(256), 0, erow, enbr, (const uint32_t *)csr->off, V, E,
                buf[0], words + CC_HOOKS);
    }

    // flatten: only the last launch between two looks counts what it moved — if it moved nothing the forest is flat
    const uint32_t per_check = ctx->cc_jumps_per_check ? ctx->cc_jumps_per_check : CC_JUMPS_PER_CHECK;
    uint32_t launches = 0;
    int cur = 0;
    while (true) {
      for (uint32_t j = 0; j < per_check; j++, launches++, cur ^= 1) {
        const bool last = j + 1 == per_check;
        if (last) GG_HIP(hipMemsetAsync(words + CC_CHANGED, 0, sizeof(uint64_t), st));
        GG_LAUNCH(ctx, "cc_jump", k_cc_jump, vgrid, dim3(256), 0, (const uint32_t *)buf[cur], V, buf[cur ^ 1],
                  last ? words + CC_CHANGED : (unsigned long long *)nullptr);
      }
      uint64_t changed = 0;
      GG_TRY(read_back(ctx, {{words + CC_CHANGED, sizeof(uint64_t), &changed}}));
      if (!changed) break;
    }
    const uint32_t *root = buf[cur];
    uint32_t *flag = buf[cur ^ 1];  // (the other array is free again)

    GG_LAUNCH(ctx, "cc_size", k_cc_size, vgrid, dim3(256), 0, root, V, ctx->cc_size_fold ? 1 : 0, size);
    GG_LAUNCH(ctx, "cc_flag", k_cc_flag, vgrid, dim3(256), 0, root, (const uint32_t *)size, V, flag, words + CC_LARGEST,
              words + CC_SINGLETONS);
    GG_TRY(scan_exclusive_u32(ctx, flag, flag, V, (uint64_t *)(words + CC_COMPONENTS)));
    if (res) {
      for (int c = 0; c < 3; c++) {
        GG_TRY(ctx->dev_alloc((void **)&res->cols[0][c], V * sizeof(int64_t)));
        ctx->keep(res->cols[0][c]);
      }
      GG_LAUNCH(ctx, "cc_rows", k_cc_rows, vgrid, dim3(256), 0, root, (const uint32_t *)size, (const int64_t *)csr->vid, V,
                res->cols[0][0], res->cols[0][1], res->cols[0][2]);
      res->rows[0] = V;
    }
    uint64_t hw[CC_WORDS];
    GG_TRY(read_back(ctx, {{words, sizeof(hw), hw}}));  // every counter in one look
    const uint64_t n_comp = hw[CC_COMPONENTS];
    if (res) {  // (1 <= n_comp <= V)
      for (int c = 0; c < 2; c++) {
        GG_TRY(ctx->dev_alloc((void **)&res->cols[1][c], n_comp * sizeof(int64_t)));
        ctx->keep(res->cols[1][c]);
      }
      GG_LAUNCH(ctx, "cc_reps", k_cc_reps, vgrid, dim3(256), 0, root, (const uint32_t *)size, (const uint32_t *)flag,
                (const int64_t *)csr->vid, V, res->cols[1][0], res->cols[1][1]);
      res->rows[1] = n_comp;  // (no further look: a fetch is ordered behind the stream, as is the pool blocks' next user)
    }
    if (stats) {
      stats->components = n_comp;
      stats->largest = hw[CC_LARGEST];
      stats->singletons = hw[CC_SINGLETONS];
      stats->hooks = hw[CC_HOOKS];
      stats->jump_launches = launches;
    }
  }
  if (stats) {
    stats->vertices = V;
    stats->entries_read = E;
  }
  if (out_result) *out_result = res.release();
  return GG_OK;
}

extern "C" int gg_components_rows(const gg_result *res, int table, uint64_t *n_rows) {
  if (!res || !n_rows) return GG_ERR_INVALID_ARG;
  GG_TRY(expect_kind(res, ResultKind::COMPONENTS, "gg_components_rows"));
  if (table < 0 || table > 1) return GG_ERR_INVALID_ARG;
  *n_rows = res->rows[table];
  return GG_OK;
}

extern "C" int gg_components_fetch(const gg_result *res, uint64_t offset, uint32_t max_rows, int64_t *vertex_id,
                                   int64_t *component_id, uint64_t *size, uint32_t *n_out) {
  if (!res || !n_out) return GG_ERR_INVALID_ARG;
  GG_TRY(expect_kind(res, ResultKind::COMPONENTS, "gg_components_fetch"));
  int64_t *const *col = res->cols[0];
  return fetch_slice(res->ctx, res->rows[0], offset, max_rows, {{vertex_id, col[0]}, {component_id, col[1]}, {size, col[2]}},
                     n_out);
}

extern "C" int gg_components_fetch_sizes(const gg_result *res, uint64_t offset, uint32_t max_rows, int64_t *component_id,
                                         uint64_t *size, uint32_t *n_out) {
  if (!res || !n_out) return GG_ERR_INVALID_ARG;
  GG_TRY(expect_kind(res, ResultKind::COMPONENTS, "gg_components_fetch_sizes"));
  return fetch_slice(res->ctx, res->rows[1], offset, max_rows, {{component_id, res->cols[1][0]}, {size, res->cols[1][1]}},
                     n_out);
}

extern "C" int gg_debug_components(gg_ctx *ctx, int init_mode, uint32_t jumps_per_check) {
  if (!ctx || init_mode < 0 || init_mode > 1) return GG_ERR_INVALID_ARG;
  ctx->cc_init_mode = init_mode;
  ctx->cc_jumps_per_check = jumps_per_check;
  return GG_OK;
}
