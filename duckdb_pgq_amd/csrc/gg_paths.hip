// gg_paths.hip — the shortest paths themselves, read backwards off a finished 64-lane BFS (gg_bfs.hip).
//
// The reference has no relation for this (its bi-10 query stops at min(hopCount),
// benchmark/ldbc/queries/bi-10-shortestpath.sql:26-31); what a host would do with its operators is one more self-join
// of friends_shortest with knows per step (PhysicalHashJoin::Execute -> JoinHashTable::Probe,
// src/execution/operator/join/physical_hash_join.cpp:217-254, src/execution/join_hashtable.cpp:304-476) under a
// min(rowid) aggregate (src/execution/operator/aggregate/physical_hash_aggregate.cpp:152-266).  Here everything a path
// needs is still on the device when the BFS batch ends: the distance cells dist[V][64], the reverse CSR and the forward
// CSR with its rowids.
//
// The relation (include/gg.h, gg_bfs64_paths): for lane s and vertex x at distance d >= 1,
//   pred(s, x) = the entry u of x's reverse row with dist[u][s] == d - 1 that has the smallest dense index
//   edge(s, x) = the first entry of pred's forward row whose destination is x      (the edge appended first)
// and the path of a pair (s, t) is t, pred(s, t), ... back to the source; one row per step.
//
//   k_path_len     per pair d + 1 (0: unreached or not a vertex); scan_exclusive_u32 turns them into row bases
//   k_path_trace   GG_PATH_LANES lanes per pair walk from t back to s; the groups of a wavefront advance in lockstep,
//                  one chunk of GG_PATH_LANES row entries per trip each, whatever phase each is in
// Bytes per step (model): the reverse row up to the predecessor (4 B an entry) + one 64/128-byte distance
// line per entry looked at (a gather: the cells of one lane lie 64 cells apart) + the predecessor's forward row up to
// the edge (4 B an entry) + 8 B rowid + 28 B of result row.  The serial depth of a pair is its distance.
#include "gg_internal.h"

#ifndef GG_PATH_LANES
#define GG_PATH_LANES 16  // lanes per pair in k_path_trace.  SF100 knows, 64 sources, k_path_trace per batch: every vertex as target
                          // (28.7 M pairs, 114 M rows) 64 lanes 227.7 ms, 16: 192.8, 8: 196.2; 10^4 sampled targets (640 000
                          // pairs) 64: 5.38 ms, 16: 5.02, 8: 5.36 (profiles/r09_paths_sf100_l{64,16,8}.json; batches spread ~3 %)
#endif

using namespace gg;

namespace gg {

template <typename DistT>
__global__ __launch_bounds__(256) void k_path_len(const DistT *__restrict__ dist, const uint32_t *__restrict__ pair_lane,
                                                  const uint32_t *__restrict__ dst_dense, uint64_t n_pairs,
                                                  uint32_t *__restrict__ len) {
  for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_pairs; p += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t t = dst_dense[p];
    uint32_t n = 0;
    if (t != INVALID_U32) {
      const DistT d = dist[(uint64_t)t * 64 + pair_lane[p]];
      if (d != (DistT)~(DistT)0) n = (uint32_t)d + 1u;
    }
    len[p] = n;
  }
}

// the source of every forward CSR entry (the COO view the bucketed build does not keep): a binary search in the offsets
__global__ __launch_bounds__(256) void k_entry_rows(const uint32_t *__restrict__ off, uint64_t V, uint64_t E,
                                                    uint32_t *__restrict__ row) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < E; i += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t lo = 0, hi = V;  // the last v with off[v] <= i
    while (hi - lo > 1) {
      const uint64_t mid = (lo + hi) >> 1;
      if (off[mid] <= i) lo = mid; else hi = mid;
    }
    row[i] = (uint32_t)lo;
  }
}

// csr->rnbr_by_src: the reverse rows with their entries ascending by (source, forward CSR position), under the same
// csr->roff.  The bucketed build leaves reverse rows in rowid order (gg_csr_fast.hip) and only the multi-pass build
// sorts them by source; a BFS pull does not care, the trace does: with the sources ascending, the FIRST entry one level
// closer is the predecessor with the smallest dense index and a step ends at the first hit.  One stable sort of the
// forward entries by destination, once per CSR (first gg_bfs64_paths call), 4 E bytes kept with it.
int ensure_reverse_by_source(gg_ctx *ctx, gg_csr *csr) {
  if (csr->rnbr_by_src) return GG_OK;
  // (a search of zero levels never built it; a derived build has the offsets and not yet the rows its callers pull along)
  if (!csr->roff || !csr->rnbr_rows) GG_TRY(ensure_reverse(ctx, csr));
  const uint64_t V = csr->V, E = csr->E;
  uint32_t *row = csr->row, *own_row = nullptr, *key_out = nullptr, *sorted = nullptr;
  GG_TRY(ctx->dev_alloc((void **)&sorted, (E ? E : 1) * sizeof(uint32_t)));
  if (E) {
    if (!row) {
      GG_TRY(ctx->dev_alloc((void **)&own_row, E * sizeof(uint32_t)));
      GG_LAUNCH(ctx, "path_entry_rows", k_entry_rows, stride_grid(ctx, E), dim3(256), 0, (const uint32_t *)csr->off, V, E,
                own_row);
      row = own_row;
    }
    GG_TRY(ctx->dev_alloc((void **)&key_out, E * sizeof(uint32_t)));
    GG_TRY(sort_pairs_by_key(ctx, csr->nbr, row, E, bits_for(V < 2 ? 2 : V), key_out, sorted));
    GG_TRY(sync_checked(ctx));
  }
  ctx->keep(sorted);
  csr->rnbr_by_src = sorted;
  return GG_OK;
}

__global__ __launch_bounds__(256) void k_entry_positions(uint64_t E, uint32_t *__restrict__ pos) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < E; i += (uint64_t)gridDim.x * blockDim.x)
    pos[i] = (uint32_t)i;
}

// csr->rpos_by_src: the forward CSR position of every entry of rnbr_by_src — the same stable sort of the forward
// entries by destination, carrying the position instead of the source.  Equal sources c of a's row therefore stand in
// ascending forward position, i.e. in append order (forward rows are in append order on every build), which is the
// order gg_triangles_edges lists parallel closing rows c -> a in.  Once per CSR, on the first gg_triangles_edges call;
// 4 E bytes kept with it.  gg_bfs64_paths and gg_triangles never build it.
int ensure_reverse_pos_by_source(gg_ctx *ctx, gg_csr *csr) {
  if (csr->rpos_by_src) return GG_OK;
  const uint64_t V = csr->V, E = csr->E;
  uint32_t *pos = nullptr, *key_out = nullptr, *sorted = nullptr;
  GG_TRY(ctx->dev_alloc((void **)&sorted, (E ? E : 1) * sizeof(uint32_t)));
  if (E) {
    GG_TRY(ctx->dev_alloc((void **)&pos, E * sizeof(uint32_t)));
    GG_TRY(ctx->dev_alloc((void **)&key_out, E * sizeof(uint32_t)));
    GG_LAUNCH(ctx, "tri_entry_positions", k_entry_positions, stride_grid(ctx, E), dim3(256), 0, E, pos);
    GG_TRY(sort_pairs_by_key(ctx, csr->nbr, pos, E, bits_for(V < 2 ? 2 : V), key_out, sorted));
    GG_TRY(sync_checked(ctx));
  }
  ctx->keep(sorted);
  csr->rpos_by_src = sorted;
  return GG_OK;
}

// One lane group per pair (grid-strided).  A group is in one of two phases: looking through the reverse row of x, its
// sources ascending (rnbr_by_src), for the first in-neighbour one level closer (phase 0), or through that neighbour's
// forward row for the first entry that leads to x (phase 1: forward rows are in append order on every build).  Each
// trip of the loop every group of the wavefront reads one chunk of L entries of its row, ballots and either moves its
// cursor or commits; all state is uniform inside a group and every cross-lane operation is executed by the whole
// wavefront.  (c += L cannot wrap: c < e <= E <= 2^32 - 2 and a trip past e ends the search.)
template <typename DistT, int L>
__global__ __launch_bounds__(256) void k_path_trace(const DistT *__restrict__ dist, const uint32_t *__restrict__ pair_lane,
                                                    const uint32_t *__restrict__ dst_dense, uint64_t n_pairs,
                                                    const uint32_t *__restrict__ base /* exclusive scan of len */,
                                                    const uint32_t *__restrict__ len, const uint32_t *__restrict__ off,
                                                    const uint32_t *__restrict__ nbr, const uint32_t *__restrict__ epos,
                                                    const int64_t *__restrict__ eid, const uint32_t *__restrict__ roff,
                                                    const uint32_t *__restrict__ rnbr, const int64_t *__restrict__ vid,
                                                    int64_t *__restrict__ out_pair, int32_t *__restrict__ out_step,
                                                    int64_t *__restrict__ out_vtx, int64_t *__restrict__ out_edge /* nullable */,
                                                    uint32_t *__restrict__ bad /* != 0: distances and CSR disagree */) {
  constexpr int GPW = 64 / L;  // groups per wavefront
  constexpr uint64_t GMASK = L == 64 ? ~0ULL : ((1ULL << (L % 64)) - 1ULL);
  const int lane = threadIdx.x & 63, gbase = (lane / L) * L, gl = lane % L;
  const uint64_t wave0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  const bool want_edges = out_edge != nullptr;
  for (uint64_t pbase = wave0 * GPW; pbase < n_pairs; pbase += nwaves * GPW) {
    const uint64_t p = pbase + (uint64_t)(lane / L);
    uint32_t n = p < n_pairs ? len[p] : 0u;
    const uint64_t row0 = n ? base[p] : 0;
    const uint32_t bl = n ? pair_lane[p] : 0u;
    uint32_t x = n ? dst_dense[p] : 0u;  // the vertex of step i
    uint32_t i = n ? n - 1 : 0u;         // steps still to take
    if (n && i == 0 && gl == 0) {        // s == t (or the walk arrived): the row of step 0
      out_pair[row0] = (int64_t)p;
      out_step[row0] = 0;
      out_vtx[row0] = vid[x];
      if (want_edges) out_edge[row0] = -1;
    }
    bool active = n && i >= 1;
    int phase = 0;
    uint32_t pu = 0;                // pred(s, x), valid in phase 1
    uint32_t c = 0, e = 0;          // cursor and end of the row being searched
    if (active) {
      c = roff[x];
      e = roff[x + 1];
    }
    while (__any(active)) {
      const uint32_t idx = c + (uint32_t)gl;
      const bool inb = active && idx < e;
      const uint32_t val = inb ? (phase ? nbr[idx] : rnbr[idx]) : INVALID_U32;
      bool hit = false;
      if (inb) hit = phase ? val == x : dist[(uint64_t)val * 64 + bl] == (DistT)(i - 1);
      const uint64_t g = (__ballot(hit) >> gbase) & GMASK;
      const int first = g ? __ffsll((long long)g) - 1 : 0;
      const uint32_t sel = (uint32_t)__shfl((int)val, gbase + first, 64);
      if (active) {
        bool commit = false, lost = false;
        int64_t rowid = -1;
        if (g) {
          if (phase == 0) {
            pu = sel;
            if (want_edges) {
              phase = 1;
              c = off[pu];
              e = off[pu + 1];
            } else {
              commit = true;
            }
          } else {
            const uint32_t at = c + (uint32_t)first;
            rowid = eid ? eid[at] : (int64_t)epos[at];
            commit = true;
          }
        } else {
          c += L;
          // no in-neighbour one level closer, or no edge pu -> x: never with a consistent BFS and CSR
          lost = c >= e;
        }
        if (lost) {
          if (gl == 0) atomicOr(bad, 1u);
          active = false;
        }
        if (commit) {
          if (gl == 0) {
            out_pair[row0 + i] = (int64_t)p;
            out_step[row0 + i] = (int32_t)i;
            out_vtx[row0 + i] = vid[x];
            if (want_edges) out_edge[row0 + i] = rowid;
          }
          x = pu;
          i -= 1;
          phase = 0;
          if (i >= 1) {
            c = roff[x];
            e = roff[x + 1];
          } else {
            if (gl == 0) {
              out_pair[row0] = (int64_t)p;
              out_step[row0] = 0;
              out_vtx[row0] = vid[x];
              if (want_edges) out_edge[row0] = -1;
            }
            active = false;
          }
        }
      }
    }
  }
}

template <typename DistT>
static int paths_emit_t(gg_ctx *ctx, const gg_csr *csr, const DistT *dist, const PathsRequest &rq) {
  gg_result *res = rq.res;
  const uint64_t n = rq.n_pairs;
  hipStream_t s = ctx->stream;
  uint32_t *lane_dev = nullptr, *dst_dense = nullptr, *len = nullptr, *base = nullptr, *bad = nullptr;
  uint64_t rows = 0;
  GG_TRY(ctx->dev_alloc((void **)&lane_dev, n * sizeof(uint32_t)));
  GG_TRY(ctx->dev_alloc((void **)&len, n * sizeof(uint32_t)));
  GG_TRY(ctx->dev_alloc((void **)&base, n * sizeof(uint32_t)));
  GG_TRY(ctx->dev_alloc((void **)&bad, sizeof(uint32_t)));
  GG_HIP(hipMemcpyAsync(lane_dev, rq.pair_lane, n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  GG_HIP(hipMemsetAsync(bad, 0, sizeof(uint32_t), s));
  GG_TRY(upload_ids(ctx, csr, rq.pair_dst_ids, n, &dst_dense));
  GG_LAUNCH(ctx, "path_len", (k_path_len<DistT>), stride_grid(ctx, n), dim3(256), 0, dist, (const uint32_t *)lane_dev,
            (const uint32_t *)dst_dense, n, len);
  GG_TRY(scan_total_u32(ctx, len, base, n, &rows));
  if (rows >= (1ull << 32)) {  // (the bases are 32-bit and have wrapped: nothing is traced)
    set_error("gg_bfs64_paths: %llu path rows in one batch (2^32 or more)", (unsigned long long)rows);
    return GG_ERR_TOO_LARGE;
  }
  if (rows == 0) return GG_OK;
  const int ncols = rq.want_edges ? 4 : 3;  // pair, vertex, step (int32), edge
  for (int c = 0; c < ncols; c++)
    GG_TRY(ctx->dev_alloc((void **)&res->cols[PATHS_TABLE][c], rows * (c == 2 ? sizeof(int32_t) : sizeof(int64_t))));
  constexpr int L = GG_PATH_LANES, GPW = 64 / L;
  static_assert(L == 64 || L == 32 || L == 16 || L == 8 || L == 4, "GG_PATH_LANES divides the wavefront");
  const uint64_t waves = (n + GPW - 1) / GPW, max_waves = (uint64_t)ctx->num_cus * 32;
  const unsigned grid = (unsigned)(((waves < max_waves ? waves : max_waves) * 64 + 255) / 256);
  GG_LAUNCH(ctx, "path_trace", (k_path_trace<DistT, L>), dim3(grid), dim3(256), 0, dist, (const uint32_t *)lane_dev,
            (const uint32_t *)dst_dense, n, (const uint32_t *)base, (const uint32_t *)len, (const uint32_t *)csr->off,
            (const uint32_t *)csr->nbr, (const uint32_t *)csr->epos, (const int64_t *)csr->eid,
            (const uint32_t *)csr->roff, (const uint32_t *)csr->rnbr_by_src, (const int64_t *)csr->vid,
            res->cols[PATHS_TABLE][0], reinterpret_cast<int32_t *>(res->cols[PATHS_TABLE][2]), res->cols[PATHS_TABLE][1],
            rq.want_edges ? res->cols[PATHS_TABLE][3] : (int64_t *)nullptr, bad);
  uint32_t n_bad = 0;
  GG_TRY(read_back(ctx, {{bad, sizeof(uint32_t), &n_bad}}));
  if (n_bad) {
    set_error("gg_bfs64_paths: a reached vertex has no in-neighbour one level closer (distances and CSR disagree)");
    for (int c = 0; c < ncols; c++) res->cols[PATHS_TABLE][c] = nullptr;  // (not kept: the caller's ApiScope frees them)
    return GG_ERR_STATE;
  }
  for (int c = 0; c < ncols; c++) ctx->keep(res->cols[PATHS_TABLE][c]);
  res->rows[PATHS_TABLE] = rows;
  return GG_OK;
}

int paths_emit(gg_ctx *ctx, gg_csr *csr, const void *dist, size_t cell_bytes, const PathsRequest &rq) {
  if (rq.n_pairs == 0) return GG_OK;
  GG_TRY(ensure_reverse_by_source(ctx, csr));
  return cell_bytes == 1 ? paths_emit_t<uint8_t>(ctx, csr, (const uint8_t *)dist, rq)
                         : paths_emit_t<uint16_t>(ctx, csr, (const uint16_t *)dist, rq);
}

}  // namespace gg

extern "C" int gg_bfs64_paths_rows(const gg_result *res, uint64_t *n_rows) {
  GG_TRY(expect_kind(res, ResultKind::PATHS, "gg_bfs64_paths_rows"));
  if (!n_rows) return GG_ERR_INVALID_ARG;
  *n_rows = res->rows[PATHS_TABLE];
  return GG_OK;
}

extern "C" int gg_bfs64_paths_fetch(const gg_result *res, uint64_t offset, uint32_t max_rows, int64_t *pair_index,
                                    int32_t *step, int64_t *vertex_id, int64_t *edge_rowid, uint32_t *n_out) {
  GG_TRY(expect_kind(res, ResultKind::PATHS, "gg_bfs64_paths_fetch"));
  if (!n_out || !pair_index || !step || !vertex_id) return GG_ERR_INVALID_ARG;
  int64_t *const *col = res->cols[PATHS_TABLE];
  GG_TRY(fetch_slice(res->ctx, res->rows[PATHS_TABLE], offset, max_rows,
                     {{pair_index, col[0]}, {vertex_id, col[1]}, {edge_rowid, col[3]}, {step, col[2], sizeof(int32_t)}},
                     n_out));
  if (!col[3] && edge_rowid)
    for (uint32_t r = 0; r < *n_out; r++) edge_rowid[r] = -1;  // searched without edges
  return GG_OK;
}
