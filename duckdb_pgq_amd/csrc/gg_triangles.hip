// gg_triangles.hip — triangle rows (closed 3-edge walks) counted and listed on the device.
//
// The reference evaluates `knows k1, knows k2, knows k3 WHERE k1.dst = k2.src AND k2.dst = k3.src AND k3.dst = k1.src`
// as a chain of three hash joins whose last join carries two conditions (PhysicalHashJoin::Execute ->
// JoinHashTable::Probe + ScanStructure::NextInnerJoin, src/execution/operator/join/physical_hash_join.cpp:217-254,
// src/execution/join_hashtable.cpp:304-476): every 2-hop walk is formed and probed.  "Friend triangles",
// benchmark/ldbc/queries/bi-11.sql:22-33, is that chain under count(*) with p1.id < p2.id < p3.id.
//
// Here a wedge a -> b -> c is closed by a search: its rows are the entries equal to c of a's reverse row, which
// csr->rnbr_by_src holds with its sources ascending (gg_paths.hip), so the multiplicity is a run length.
//
//   entries   the pairs (source s, b) with a = source s, b in out(a), out(b) not empty, in source order then CSR order
//             (k_tri_src_count, scan, k_tri_src_write); woff = exclusive prefix of |out(b)| over them
//   tiles     source s owns ceil(wedges(s) / TRI_TW) tiles of TRI_TW consecutive wedges (toff = prefix over sources): the
//             work is cut by WEDGE count, a hub's wedges spread over as many wavefronts as they need
//   k_tri_tiles   one wavefront per tile, four tiles per workgroup.  The wavefront finds its source (search in toff) and
//             its first entry (search in woff), stages the <= TRI_TW + 1 wedge offsets of its entries and, if it fits,
//             the sorted in-row of a in LDS; then 64 wedges per trip: entry by a search in the staged offsets, c by
//             one coalesced read of out(b), lower and upper bound of c in the in-row.  An in-row above the LDS budget
//             (gg_debug_triangle_tile lowers it) is searched where it lies, in global memory: every tile of that
//             hub reads the same row, which stays in L2.
//   order = 1   rank(v) = position of v's id among the ids ascending (two radix passes over the id halves, once per
//             call), then two filtered copies of the rows made by count, scan, write: F = forward entries x -> y with
//             rank(x) < rank(y), D = reverse entries (y <- x) with rank(x) > rank(y), sources still ascending.  A row
//             with id(a) < id(b) < id(c) is a wedge of F closed by an entry of D, so the same kernel runs on (F, D):
//             pruned on both sides, and no id or rank is read per wedge at all.
//   rows      count mode leaves each tile's row count; after a scan the same traversal writes the rows, a wedge's rows
//             at tile base + prefix inside the wavefront: no atomics-ordered append, the same rows at the same places
//             on every run.
//
//   edges     gg_triangles_edges also writes the rowids of e1: a -> b, e2: b -> c, e3: c -> a (k_tri_write_edges, the third
//             mode of k_tri_tiles).  All three are eid / epos of a forward CSR position: e1's is kept per entry (ent_pos),
//             e2's is foff[b] + k, e3's is csr->rpos_by_src (gg_paths.hip) at the run's index in a's in-row.  Under
//             order = 1 the filter passes carry the positions of F's and D's entries along (fmap, imap).  Positions are
//             read from global memory, and only for wedges that have rows.
//
// Bytes per wedge (model): 4 B of out(b), read coalesced, plus ~log2|in(a)| 4-byte probes in LDS; per tile 8 B x
// (entries + 1) of woff, 4 B x entries of ent_b and 4 B x |in(a)| of the in-row staged once per TRI_TW wedges; per
// row written 24 B (with edges 48 B, and per wedge with rows two 4-byte positions + two rowids, per row one position
// + one rowid).  Per call 12 B per entry written and read once, and for order = 1 the O(V + E) filter passes.
#include "gg_internal.h"

using namespace gg;

namespace {

constexpr int TRI_TW = 512;         // wedges per tile = per wavefront
constexpr int TRI_WAVES = 4;        // tiles per workgroup of 256 threads
constexpr int TRI_LDS_IN = 1535;    // in-row entries a wavefront may stage: (TRI_TW + 1) + 1535 words = 8 KB a wavefront,
                                    // 32 KB a workgroup, five workgroups (20 wavefronts) per CU of 160 KB
constexpr uint64_t TRI_MAX_GROUPS = 0xFFFFFFFFull / 256;

// ---- order = 1: rank of every vertex id, filtered rows ------------------------------------------------------------
// One LSD piece of the rank sort: TRI_RANK_PIECE_BITS bits at `shift` of the id with its sign bit flipped (so that the
// unsigned pieces order the ids signed), of the vertices in the order the earlier pieces left (perm; null: 0..V-1).
// (Pieces, not 32-bit halves: the shared radix sort keeps key 0xFFFFFFFF for "no element" — gg_internal.h — and a half
// of an id such as -1, 4294967295 or INT64_MAX is exactly that.)
constexpr int TRI_RANK_PIECE_BITS = 16;
__global__ __launch_bounds__(256) void k_tri_rank_key(const int64_t *__restrict__ vid, const uint32_t *__restrict__ perm,
                                                      uint64_t V, uint32_t shift, uint32_t *__restrict__ key,
                                                      uint32_t *__restrict__ val) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < V; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t v = perm ? perm[i] : (uint32_t)i;
    const uint64_t id = (uint64_t)vid[v] ^ (1ull << 63);
    key[i] = (uint32_t)(id >> shift) & ((1u << TRI_RANK_PIECE_BITS) - 1);
    val[i] = v;
  }
}

__global__ __launch_bounds__(256) void k_tri_rank_scatter(const uint32_t *__restrict__ perm, uint64_t V,
                                                          uint32_t *__restrict__ rank) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < V; i += (uint64_t)gridDim.x * blockDim.x)
    rank[perm[i]] = (uint32_t)i;
}

// cnt[v] = entries y of row v with rank(y) > rank(v); cnt[V] = 0 (the scan's last element)
__global__ __launch_bounds__(256) void k_tri_filter_count(const uint32_t *__restrict__ off, const uint32_t *__restrict__ nbr,
                                                          const uint32_t *__restrict__ rank, uint64_t V,
                                                          uint32_t *__restrict__ cnt) {
  for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v <= V; v += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t n = 0;
    if (v < V) {
      const uint32_t r = rank[v];
      for (uint32_t j = off[v], e = off[v + 1]; j < e; j++) n += rank[nbr[j]] > r;
    }
    cnt[v] = n;
  }
}

// POS: pos_out[o] = the forward CSR position of the entry kept at o — pos_in[j], or j itself where pos_in is null
template <bool POS>
__global__ __launch_bounds__(256) void k_tri_filter_write(const uint32_t *__restrict__ off, const uint32_t *__restrict__ nbr,
                                                          const uint32_t *__restrict__ rank, uint64_t V,
                                                          const uint32_t *__restrict__ off_out,
                                                          uint32_t *__restrict__ nbr_out,
                                                          const uint32_t *__restrict__ pos_in,
                                                          uint32_t *__restrict__ pos_out) {
  for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t r = rank[v];
    uint32_t o = off_out[v];
    for (uint32_t j = off[v], e = off[v + 1]; j < e; j++) {
      const uint32_t y = nbr[j];
      if (rank[y] > r) {  // (o < off_out[v + 1]: the count kernel counted the same entries)
        if (POS) pos_out[o] = pos_in ? pos_in[j] : j;
        nbr_out[o++] = y;
      }
    }
  }
}

// ---- entries and tiles of the sources -----------------------------------------------------------------------------
// per source: entries with wedges, and tiles; element n_src of both is 0 (the scans' last element)
__global__ __launch_bounds__(256) void k_tri_src_count(const uint32_t *__restrict__ sdense, uint64_t n_src, uint64_t V,
                                                       const uint32_t *__restrict__ foff, const uint32_t *__restrict__ fnbr,
                                                       uint64_t *__restrict__ ecnt, uint64_t *__restrict__ tcnt) {
  for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s <= n_src; s += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t n = 0, w = 0;
    const uint32_t a = s < n_src ? (sdense ? sdense[s] : (uint32_t)s) : INVALID_U32;
    if (a != INVALID_U32 && a < V) {
      for (uint32_t j = foff[a], e = foff[a + 1]; j < e; j++) {
        const uint32_t b = fnbr[j], d = foff[b + 1] - foff[b];
        n += d != 0;
        w += d;
      }
    }
    ecnt[s] = n;
    tcnt[s] = (w + TRI_TW - 1) / TRI_TW;
  }
}

// ent_b / ent_w of every source's entries at eoff[s]..; ent_w[n_ent] = 0.  POS: ent_pos = the entry's index in fnbr
template <bool POS>
__global__ __launch_bounds__(256) void k_tri_src_write(const uint32_t *__restrict__ sdense, uint64_t n_src, uint64_t V,
                                                       const uint32_t *__restrict__ foff, const uint32_t *__restrict__ fnbr,
                                                       const uint64_t *__restrict__ eoff, uint32_t *__restrict__ ent_b,
                                                       uint64_t *__restrict__ ent_w, uint32_t *__restrict__ ent_pos) {
  for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s <= n_src; s += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t o = eoff[s];
    if (s == n_src) {
      ent_w[o] = 0;
      continue;
    }
    const uint32_t a = sdense ? sdense[s] : (uint32_t)s;
    if (a == INVALID_U32 || a >= V) continue;
    for (uint32_t j = foff[a], e = foff[a + 1]; j < e; j++) {
      const uint32_t b = fnbr[j], d = foff[b + 1] - foff[b];
      if (d) {  // (o < eoff[s + 1]: k_tri_src_count counted the same entries)
        ent_b[o] = b;
        ent_w[o] = d;
        if (POS) ent_pos[o] = j;
        o++;
      }
    }
  }
}

// ---- the wedge kernel -----------------------------------------------------------------------------------------------
struct TriArgs {
  const uint32_t *sdense;  // nullable: source s is vertex s
  uint64_t n_src;
  const uint32_t *foff, *fnbr;  // the rows wedges are formed from
  const uint32_t *ioff, *inbr;  // the in-rows the closing edge is looked for in, entries ascending
  const uint64_t *eoff;         // n_src + 1: first entry of a source
  const uint64_t *woff;         // n_ent + 1: first wedge of an entry
  const uint64_t *toff;         // n_src + 1: first tile of a source
  const uint32_t *ent_b;
  uint32_t lds_cap;             // in-rows of more entries are searched in global memory
  unsigned long long *stats;    // count: [0] += rows, [1] += digest
  uint64_t *tile_rows;          // count: rows of a tile (nullable); write: first row of a tile
  const int64_t *vid;           // write
  int64_t *out_a, *out_b, *out_c;
};

// k_tri_write_edges only: every rowid is eid / epos of a forward CSR position.  (A parameter of its own behind t0 and nt,
// so that the kernel arguments of the count and write modes lie where they always did.)
struct TriEdges {
  const uint32_t *ent_pos;      // index in fnbr of an entry's edge a -> b
  const uint32_t *fmap;         // forward CSR position of an index in fnbr (nullable: fnbr is the forward CSR)
  const uint32_t *imap;         // forward CSR position of an index in inbr
  const uint32_t *epos;
  const int64_t *eid;           // nullable: the rowid is epos
  int64_t *out_e1, *out_e2, *out_e3;
};

enum TriMode { TRI_COUNT = 0, TRI_WRITE = 1, TRI_WRITE_EDGES = 2 };

// how often c occurs in the ascending row[0..n); first = the index of its first occurrence (if it occurs)
template <typename Row>
__device__ __forceinline__ uint32_t tri_run(Row row, uint32_t n, uint32_t c, uint32_t &first) {
  uint32_t lo = 0, hi = n;  // first idx with row[idx] >= c
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (row[mid] < c) lo = mid + 1; else hi = mid;
  }
  if (lo == n || row[lo] != c) return 0;
  first = lo;
  uint32_t l2 = lo + 1, h2 = n;  // first idx with row[idx] > c
  while (l2 < h2) {
    const uint32_t mid = (l2 + h2) >> 1;
    if (row[mid] <= c) l2 = mid + 1; else h2 = mid;
  }
  return l2 - lo;
}

template <int MODE>
__global__ __launch_bounds__(256) void k_tri_tiles(const TriArgs A, uint64_t t0, uint64_t nt, const TriEdges X) {
  constexpr bool WRITE = MODE != TRI_COUNT, EDGES = MODE == TRI_WRITE_EDGES;
  __shared__ uint32_t s_mem[TRI_WAVES][TRI_TW + 1 + TRI_LDS_IN];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint32_t *s_w = s_mem[wave], *s_in = s_mem[wave] + TRI_TW + 1;
  const uint64_t tl = (uint64_t)blockIdx.x * TRI_WAVES + wave;
  const bool live = tl < nt;  // (uniform in the wavefront)
  const uint64_t t = t0 + tl;
  uint32_t a = 0, n = 0, nwin = 2, in_n = 0;
  uint64_t e_first = 0, skip = 0;
  const uint32_t *in_row = A.inbr;
  bool staged = false;
  if (live) {
    uint64_t lo = 0, hi = A.n_src;  // first idx in [0, n_src] with toff[idx] > t (toff[n_src] = all tiles > t)
    while (lo < hi) {
      const uint64_t mid = (lo + hi) >> 1;
      if (A.toff[mid] <= t) lo = mid + 1; else hi = mid;
    }
    const uint64_t s = lo - 1;  // (toff[0] = 0 <= t)
    a = A.sdense ? A.sdense[s] : (uint32_t)s;  // a vertex: only sources with wedges have tiles
    const uint64_t e_lo = A.eoff[s], e_hi = A.eoff[s + 1], w_hi = A.woff[e_hi];
    const uint64_t g0 = A.woff[e_lo] + (t - A.toff[s]) * TRI_TW;  // < w_hi: the source has ceil(wedges / TRI_TW) tiles
    n = (uint32_t)(w_hi - g0 < TRI_TW ? w_hi - g0 : TRI_TW);
    lo = e_lo, hi = e_hi;  // first idx in [e_lo, e_hi] with woff[idx] > g0 (woff[e_hi] = w_hi > g0)
    while (lo < hi) {
      const uint64_t mid = (lo + hi) >> 1;
      if (A.woff[mid] <= g0) lo = mid + 1; else hi = mid;
    }
    e_first = lo - 1;  // (woff[e_lo] <= g0)
    skip = g0 - A.woff[e_first];
    // every entry has a wedge, so the tile ends inside entries e_first .. e_first + TRI_TW - 1 at the latest
    nwin = (uint32_t)(e_hi - e_first + 1 < TRI_TW + 1 ? e_hi - e_first + 1 : TRI_TW + 1);
    for (uint32_t i = lane; i < nwin; i += 64) {
      const uint64_t w = A.woff[e_first + i];
      s_w[i] = w > g0 ? (uint32_t)(w - g0 < TRI_TW ? w - g0 : TRI_TW) : 0u;
    }
    const uint32_t in_lo = A.ioff[a];
    in_n = A.ioff[a + 1] - in_lo;
    in_row = A.inbr + in_lo;
    staged = in_n <= A.lds_cap;  // (lds_cap <= TRI_LDS_IN)
    if (staged)
      for (uint32_t i = lane; i < in_n; i += 64) s_in[i] = in_row[i];
  }
  __syncthreads();
  uint64_t rows = 0;
  uint32_t dig = 0;
  if (live) {
    uint64_t obase = WRITE ? A.tile_rows[t] : 0;
    const uint64_t qa = dig_q((uint64_t)a, 0);
    const int64_t id_a = WRITE ? A.vid[a] : 0;
    for (uint32_t q0 = 0; q0 < n; q0 += 64) {  // (whole wavefront: n is uniform)
      const uint32_t q = q0 + (uint32_t)lane;
      uint32_t m = 0, b = 0, c = 0, first = 0, ent = 0, kb = 0;
      if (q < n) {
        uint32_t lo = 1, hi = nwin - 1;  // first idx in [1, nwin) with s_w[idx] > q: s_w[nwin - 1] >= n > q
        while (lo < hi) {
          const uint32_t mid = (lo + hi) >> 1;
          if (s_w[mid] <= q) lo = mid + 1; else hi = mid;
        }
        const uint32_t idx = lo - 1;
        const uint64_t k = (uint64_t)(q - s_w[idx]) + (idx == 0 ? skip : 0);  // < |out(b)|
        b = A.ent_b[e_first + idx];
        c = A.fnbr[(uint64_t)A.foff[b] + k];
        m = staged ? tri_run((const uint32_t *)s_in, in_n, c, first) : tri_run(in_row, in_n, c, first);
        if (EDGES) ent = idx, kb = (uint32_t)k;
      }
      if (WRITE) {  // (fewer than 2^32 rows in all, or the rows are not written: 32-bit prefixes are exact)
        const uint32_t incl = wave_scan_incl(m);
        uint64_t pos = obase + (incl - m);
        if (m) {
          const int64_t id_b = A.vid[b], id_c = A.vid[c];
          int64_t e1 = 0, e2 = 0;
          const uint32_t *run_pos = nullptr;
          if (EDGES) {  // (ent < nwin - 1 entries of the source, kb < |out(b)|, first + m <= in_n: all inside their arrays)
            uint32_t p1 = X.ent_pos[e_first + ent], p2 = A.foff[b] + kb;
            if (X.fmap) p1 = X.fmap[p1], p2 = X.fmap[p2];
            e1 = X.eid ? X.eid[p1] : (int64_t)X.epos[p1];
            e2 = X.eid ? X.eid[p2] : (int64_t)X.epos[p2];
            run_pos = X.imap + (in_row - A.inbr) + first;  // the run's entries of a's in-row, in append order
          }
          for (uint32_t r = 0; r < m; r++, pos++) {
            A.out_a[pos] = id_a;
            A.out_b[pos] = id_b;
            A.out_c[pos] = id_c;
            if (EDGES) {
              const uint32_t p3 = run_pos[r];
              X.out_e1[pos] = e1;
              X.out_e2[pos] = e2;
              X.out_e3[pos] = X.eid ? X.eid[p3] : (int64_t)X.epos[p3];
            }
          }
        }
        obase += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
      } else if (m) {
        rows += m;
        dig += m * (uint32_t)dig_leaf(dig_q(dig_leaf(qa, b), 1), c);
      }
    }
  }
  if (!WRITE) {
    rows = wave_reduce_add_u64(rows);
    dig = wave_total_u32(dig);
    if (live && lane == 0) {
      if (A.tile_rows) A.tile_rows[t] = rows;
      if (rows) {
        atomicAdd(&A.stats[0], (unsigned long long)rows);
        atomicAdd(&A.stats[1], (unsigned long long)dig);
      }
    }
  }
}

template <int MODE>
int tri_launch(gg_ctx *ctx, const TriArgs &args, uint64_t n_tiles, const TriEdges &edges = TriEdges{}) {
  const uint64_t groups = (n_tiles + TRI_WAVES - 1) / TRI_WAVES;
  const uint64_t per_launch = ctx->max_grid_tiles && ctx->max_grid_tiles < TRI_MAX_GROUPS ? ctx->max_grid_tiles : TRI_MAX_GROUPS;
  for (uint64_t g0 = 0; g0 < groups; g0 += per_launch) {
    const uint64_t ng = groups - g0 < per_launch ? groups - g0 : per_launch;
    const uint64_t t0 = g0 * TRI_WAVES, nt = n_tiles - t0 < ng * TRI_WAVES ? n_tiles - t0 : ng * TRI_WAVES;
    GG_LAUNCH(ctx, MODE == TRI_WRITE_EDGES ? "k_tri_write_edges" : MODE == TRI_WRITE ? "k_tri_write" : "k_tri_count",
              (k_tri_tiles<MODE>), dim3((unsigned)ng), dim3(256), 0, args, t0, nt, edges);
  }
  return GG_OK;
}

// rank[v] = position of vid[v] among the ids ascending (signed): four stable sorts by 16-bit pieces, lowest first
int tri_ranks(gg_ctx *ctx, const gg_csr *csr, uint32_t **rank_out) {
  const uint64_t V = csr->V;
  uint32_t *key = nullptr, *val = nullptr, *key2 = nullptr, *perm = nullptr, *rank = nullptr;
  for (uint32_t **p : {&key, &val, &key2, &perm, &rank}) GG_TRY(ctx->dev_alloc((void **)p, V * sizeof(uint32_t)));
  for (uint32_t shift = 0; shift < 64; shift += TRI_RANK_PIECE_BITS) {
    GG_LAUNCH(ctx, "k_tri_rank_key", k_tri_rank_key, stride_grid(ctx, V), dim3(256), 0, (const int64_t *)csr->vid,
              shift ? (const uint32_t *)perm : (const uint32_t *)nullptr, V, shift, key, val);
    GG_TRY(sort_pairs_by_key(ctx, key, val, V, TRI_RANK_PIECE_BITS, key2, perm));
  }
  GG_LAUNCH(ctx, "k_tri_rank_scatter", k_tri_rank_scatter, stride_grid(ctx, V), dim3(256), 0, (const uint32_t *)perm, V,
            rank);
  *rank_out = rank;
  return GG_OK;
}

// the entries y of every row with rank(y) > rank(row), in the row's order: count, scan, write.  pos_out (nullable): also
// the forward CSR position of every entry kept — pos_in's, or the entry's own index where pos_in is null
int tri_filter_rows(gg_ctx *ctx, const uint32_t *off, const uint32_t *nbr, const uint32_t *rank, uint64_t V, uint64_t E,
                    uint32_t **off_out, uint32_t **nbr_out, const uint32_t *pos_in = nullptr, uint32_t **pos_out = nullptr) {
  GG_TRY(ctx->dev_alloc((void **)off_out, (V + 1) * sizeof(uint32_t)));
  GG_TRY(ctx->dev_alloc((void **)nbr_out, (E ? E : 1) * sizeof(uint32_t)));
  if (pos_out) GG_TRY(ctx->dev_alloc((void **)pos_out, (E ? E : 1) * sizeof(uint32_t)));
  GG_LAUNCH(ctx, "k_tri_filter_count", k_tri_filter_count, stride_grid(ctx, V + 1), dim3(256), 0, off, nbr, rank, V,
            *off_out);
  GG_TRY(scan_exclusive_u32(ctx, *off_out, *off_out, V + 1, nullptr));
  if (pos_out)
    GG_LAUNCH(ctx, "k_tri_filter_write", k_tri_filter_write<true>, stride_grid(ctx, V), dim3(256), 0, off, nbr, rank, V,
              (const uint32_t *)*off_out, *nbr_out, pos_in, *pos_out);
  else
    GG_LAUNCH(ctx, "k_tri_filter_write", k_tri_filter_write<false>, stride_grid(ctx, V), dim3(256), 0, off, nbr, rank, V,
              (const uint32_t *)*off_out, *nbr_out, (const uint32_t *)nullptr, (uint32_t *)nullptr);
  return GG_OK;
}

// gg_triangles (mode TRI_COUNT / TRI_WRITE) and gg_triangles_edges (TRI_WRITE_EDGES); `fn` names the caller in errors
int tri_call(gg_ctx *ctx, const gg_csr *csr_c, const int64_t *src_ids, uint64_t n_src, int order, TriMode mode,
             gg_tri_stats *stats, gg_result **out_result, const char *fn) {
  const bool materialise = mode != TRI_COUNT, edges = mode == TRI_WRITE_EDGES;
  if (out_result) *out_result = nullptr;
  if (!stats || (materialise && !out_result)) {
    set_error("%s: bad argument", fn);
    return GG_ERR_INVALID_ARG;
  }
  memset(stats, 0, sizeof(*stats));
  GG_TRY(check_whole_csr(ctx, csr_c));
  if (order != 0 && order != 1) {
    set_error("%s: order %d (0: every row, 1: id(a) < id(b) < id(c))", fn, order);
    return GG_ERR_INVALID_ARG;
  }
  if (edges && !csr_c->has_rowid) {
    set_error("%s needs a CSR built with edge rowids (gg_ctx_set_edge_rowid(ctx, 1))", fn);
    return GG_ERR_STATE;
  }
  gg_csr *csr = const_cast<gg_csr *>(csr_c);
  GG_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const uint64_t V = csr->V, E = csr->E;
  ResultOwner res;
  // table 2: (a, b, c), with edges also ecols (e1, e2, e3)
  if (materialise) res = make_result(ctx, ResultKind::TABLES, 2, 2);
  if (edges) res->tri_edges = true;
  const bool all = src_ids == nullptr;
  if (all) n_src = V;
  if (V && E && n_src) {
    GG_TRY(ensure_reverse_by_source(ctx, csr));
    if (edges) GG_TRY(ensure_reverse_pos_by_source(ctx, csr));
    TriArgs args{};
    TriEdges eargs{};
    args.n_src = n_src;
    args.foff = csr->off, args.fnbr = csr->nbr, args.ioff = csr->roff, args.inbr = csr->rnbr_by_src;
    eargs.imap = csr->rpos_by_src;  // (null unless edges)
    if (order == 1) {
      uint32_t *rank = nullptr, *off1 = nullptr, *nbr1 = nullptr, *ioff1 = nullptr, *inbr1 = nullptr;
      uint32_t *fmap = nullptr, *imap = nullptr;
      GG_TRY(tri_ranks(ctx, csr, &rank));
      GG_TRY(tri_filter_rows(ctx, csr->off, csr->nbr, rank, V, E, &off1, &nbr1, nullptr, edges ? &fmap : nullptr));
      GG_TRY(tri_filter_rows(ctx, csr->roff, csr->rnbr_by_src, rank, V, E, &ioff1, &inbr1, csr->rpos_by_src,
                             edges ? &imap : nullptr));
      args.foff = off1, args.fnbr = nbr1, args.ioff = ioff1, args.inbr = inbr1;
      eargs.fmap = fmap, eargs.imap = imap;
    }
    if (!all) {
      uint32_t *sdense = nullptr;
      GG_TRY(upload_ids(ctx, csr, src_ids, n_src, &sdense));
      args.sdense = sdense;
    }
    uint64_t *eoff = nullptr, *toff = nullptr, *totals = nullptr;
    GG_TRY(ctx->dev_alloc((void **)&eoff, (n_src + 1) * sizeof(uint64_t)));
    GG_TRY(ctx->dev_alloc((void **)&toff, (n_src + 1) * sizeof(uint64_t)));
    GG_TRY(ctx->dev_alloc((void **)&totals, 4 * sizeof(uint64_t)));  // entries, tiles; rows, digest
    GG_HIP(hipMemsetAsync(totals, 0, 4 * sizeof(uint64_t), st));
    GG_LAUNCH(ctx, "k_tri_src_count", k_tri_src_count, stride_grid(ctx, n_src + 1), dim3(256), 0, args.sdense, n_src, V,
              args.foff, args.fnbr, eoff, toff);
    GG_TRY(scan_exclusive_u64(ctx, eoff, eoff, n_src + 1, totals));
    GG_TRY(scan_exclusive_u64(ctx, toff, toff, n_src + 1, totals + 1));
    uint64_t h[2];
    GG_TRY(read_back(ctx, {{totals, sizeof(h), h}}));
    const uint64_t n_ent = h[0], n_tiles = h[1];
    if (n_tiles) {
      uint32_t *ent_b = nullptr, *ent_pos = nullptr;
      uint64_t *woff = nullptr, *tile_rows = nullptr;
      GG_TRY(ctx->dev_alloc((void **)&ent_b, n_ent * sizeof(uint32_t)));
      GG_TRY(ctx->dev_alloc((void **)&woff, (n_ent + 1) * sizeof(uint64_t)));
      if (edges) {
        GG_TRY(ctx->dev_alloc((void **)&ent_pos, n_ent * sizeof(uint32_t)));
        GG_LAUNCH(ctx, "k_tri_src_write", k_tri_src_write<true>, stride_grid(ctx, n_src + 1), dim3(256), 0, args.sdense,
                  n_src, V, args.foff, args.fnbr, (const uint64_t *)eoff, ent_b, woff, ent_pos);
      } else {
        GG_LAUNCH(ctx, "k_tri_src_write", k_tri_src_write<false>, stride_grid(ctx, n_src + 1), dim3(256), 0, args.sdense,
                  n_src, V, args.foff, args.fnbr, (const uint64_t *)eoff, ent_b, woff, (uint32_t *)nullptr);
      }
      GG_TRY(scan_exclusive_u64(ctx, woff, woff, n_ent + 1, nullptr));
      if (materialise) GG_TRY(ctx->dev_alloc((void **)&tile_rows, n_tiles * sizeof(uint64_t)));
      args.eoff = eoff, args.woff = woff, args.toff = toff, args.ent_b = ent_b, eargs.ent_pos = ent_pos;
      args.lds_cap = ctx->tri_lds_entries && ctx->tri_lds_entries < (uint32_t)TRI_LDS_IN ? ctx->tri_lds_entries
                                                                                        : (uint32_t)TRI_LDS_IN;
      args.stats = (unsigned long long *)(totals + 2);
      args.tile_rows = tile_rows;
      GG_TRY(tri_launch<TRI_COUNT>(ctx, args, n_tiles));
      GG_TRY(read_back(ctx, {{totals + 2, sizeof(h), h}, {woff + n_ent, sizeof(uint64_t), &stats->wedges}}));
      stats->rows = h[0];
      stats->digest = (uint64_t)(uint32_t)h[1];
      if (materialise && stats->rows) {
        if (stats->rows >= (1ull << 32)) {
          set_error("%s: %llu rows to materialise (2^32 or more); count them, or pass source lists", fn,
                    (unsigned long long)stats->rows);
          return GG_ERR_TOO_LARGE;
        }
        GG_TRY(scan_exclusive_u64(ctx, tile_rows, tile_rows, n_tiles, nullptr));
        for (int c = 0; c < 3; c++) GG_TRY(ctx->dev_alloc((void **)&res->cols[2][c], stats->rows * sizeof(int64_t)));
        args.vid = csr->vid;
        args.out_a = res->cols[2][0], args.out_b = res->cols[2][1], args.out_c = res->cols[2][2];
        int rc;
        if (edges) {
          for (int c = 0; c < 3; c++) GG_TRY(ctx->dev_alloc((void **)&res->ecols[2][c], stats->rows * sizeof(int64_t)));
          eargs.epos = csr->epos, eargs.eid = csr->eid;
          eargs.out_e1 = res->ecols[2][0], eargs.out_e2 = res->ecols[2][1], eargs.out_e3 = res->ecols[2][2];
          rc = tri_launch<TRI_WRITE_EDGES>(ctx, args, n_tiles, eargs);
        } else {
          rc = tri_launch<TRI_WRITE>(ctx, args, n_tiles);
        }
        if (rc == GG_OK) {
          for (int c = 0; c < 3; c++) {
            ctx->keep(res->cols[2][c]);
            if (edges) ctx->keep(res->ecols[2][c]);
          }
          res->rows[2] = stats->rows;
        } else {
          for (int c = 0; c < 3; c++) res->cols[2][c] = res->ecols[2][c] = nullptr;  // (not kept: the ApiScope frees them)
          return rc;
        }
        GG_TRY(sync_checked(ctx));
      }
    }
  }
  if (materialise) *out_result = res.release();
  return GG_OK;
}

}  // namespace

extern "C" int gg_triangles(gg_ctx *ctx, const gg_csr *csr, const int64_t *src_ids, uint64_t n_src, int order,
                            int materialise, gg_tri_stats *stats, gg_result **out_result) {
  ApiScope scope(ctx);
  return tri_call(ctx, csr, src_ids, n_src, order, materialise ? TRI_WRITE : TRI_COUNT, stats, out_result, "gg_triangles");
}

extern "C" int gg_triangles_edges(gg_ctx *ctx, const gg_csr *csr, const int64_t *src_ids, uint64_t n_src, int order,
                                  gg_tri_stats *stats, gg_result **out_result) {
  ApiScope scope(ctx);
  return tri_call(ctx, csr, src_ids, n_src, order, TRI_WRITE_EDGES, stats, out_result, "gg_triangles_edges");
}

extern "C" int gg_triangles_fetch_edges(const gg_result *res, uint64_t offset, uint32_t max_rows, int64_t *const *ecols,
                                        uint32_t *n_out) {
  if (!res || !ecols || !n_out || !ecols[0] || !ecols[1] || !ecols[2]) return GG_ERR_INVALID_ARG;
  if (!res->tri_edges) {
    set_error("gg_triangles_fetch_edges: the result carries no triangle edge columns (gg_triangles_edges makes them)");
    return GG_ERR_STATE;
  }
  int64_t *const *col = res->ecols[2];
  return fetch_slice(res->ctx, res->rows[2], offset, max_rows, {{ecols[0], col[0]}, {ecols[1], col[1]}, {ecols[2], col[2]}},
                     n_out);
}

extern "C" int gg_debug_triangle_tile(gg_ctx *ctx, uint32_t lds_entries) {
  if (!ctx) return GG_ERR_INVALID_ARG;
  ctx->tri_lds_entries = lds_entries;
  return GG_OK;
}
