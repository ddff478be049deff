// gg_internal.h — shared internals of libgg.so (HIP, gfx950 only; not part of the C-ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <atomic>
#include <condition_variable>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "gg.h"

namespace gg {

void set_error(const char *fmt, ...);

#define GG_HIP(call)                                                                               \
  do {                                                                                             \
    hipError_t e_ = (call);                                                                        \
    if (e_ != hipSuccess) {                                                                        \
      gg::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__);    \
      return (e_ == hipErrorOutOfMemory) ? GG_ERR_OOM : GG_ERR_HIP;                                \
    }                                                                                              \
  } while (0)

#define GG_TRY(call)            \
  do {                          \
    int rc_ = (call);           \
    if (rc_ != GG_OK) return rc_; \
  } while (0)

constexpr uint32_t INVALID_U32 = 0xFFFFFFFFu;
constexpr int64_t HT_EMPTY = INT64_MIN;  // empty-slot sentinel of the id hash table

// digest constants — must match oracle/gg_oracle.c (DESIGN.md "Row digest")
constexpr uint32_t DIG_K32 = 0x9E3779B1u;
constexpr uint64_t DIG_GOLD = 0x9E3779B97F4A7C15ULL;

struct DevBlock {
  void *ptr;
  size_t size;
  bool in_use;
  uint64_t serial;  // allocation number (ApiScope frees what an API call allocated and did not keep)
  bool keep;        // owned by a long-lived object (gg_csr, gg_result)
  bool reserved = false;  // member of a placed column set (gg_ctx::dev_alloc_columns): only handed out with its set
};

struct ProfRec {
  int name_idx;
  hipEvent_t start, stop;
};

struct alignas(16) HtSlot {
  int64_t key;
  uint32_t val;
  uint32_t pad;
};

struct Column {
  int64_t *dev = nullptr;
  size_t cap = 0;  // rows
};

struct BuildStatus {  // device-side status block of a CSR build, copied back once per build
  unsigned long long dup_vertex;   // !=0: duplicate vertex id seen
  long long min_idx;               // dense index of the vertex with id == HT_EMPTY, or -1
  unsigned long long kept;         // edges kept in the forward CSR (both endpoints are vertices, source owned)
  unsigned long long kept_rev;     // edges kept in the reverse CSR (shard builds; destination owned)
  unsigned long long owned;        // vertices owned by this shard
  unsigned long long scan_error;   // !=0: a chained scan gave up waiting for a predecessor tile (gg_runtime.hip)
  unsigned long long dict_mode;    // bucketed build: DictMode the edge densification used (DICT_WIDE16: csr->ht is built)
  unsigned long long rev_derived;  // bucketed build: !=0: every row i + E/2 mirrors row i and the reverse CSR was derived
                                   // from the forward rows (gg_csr_fast.hip "Derived reverse"); final behind k_col_scan
};

// id -> dense index dictionary used while densifying edge rows, chosen on the device from the vertex ids'
// min/max (no host synchronisation): a direct-address array, a hash table of packed 8-byte slots, or the
// general 16-byte-slot table (gg_csr.hip, gg_csr_fast.hip)
constexpr uint64_t DIRECT_MAX_RANGE = 1u << 20;
enum DictMode : unsigned long long { DICT_WIDE16 = 0, DICT_PACKED8 = 1, DICT_DIRECT = 2 };
struct DirectMap {
  long long min_id;              // INT64_MAX until k_id_minmax ran
  long long max_id;
  unsigned long long enabled;    // ids span < DIRECT_MAX_RANGE values (mode == DICT_DIRECT)
  unsigned long long mode;       // DictMode
  unsigned long long idx_bits;   // packed slots: bits of the dense index field
  unsigned long long span_bits;  // bits of max_id - min_id
  unsigned long long pairs;      // packed table: number of 16-byte slot pairs (any number, gg_dict.h)
  unsigned long long decided;    // the mode chosen from min/max (mode may fall back to DICT_WIDE16 afterwards)
};

}  // namespace gg

namespace gg {
// Guards the few words an edge-row reservation touches.  Sink threads take it once per DataChunk; with a
// sleeping mutex 64+ of them form a convoy (measured: 40 M rows staged in 33 ms by 8 threads, 600 ms by
// 256), so the hot path spins for its ~50 ns critical section and only block switches use mu/cv.
// Test-and-test-and-set with a growing pause: 255 waiters that all WRITE the lock word (a bare test_and_set loop)
// keep its cache line away from the one thread that wants to release it.
struct SpinLock {
  std::atomic<bool> held{false};
  void lock() {
    for (unsigned spins = 1;; spins = spins < 64 ? spins * 2 : 64) {
      if (!held.exchange(true, std::memory_order_acquire)) return;
      do {
        for (unsigned i = 0; i < spins; i++) __builtin_ia32_pause();
      } while (held.load(std::memory_order_relaxed));
    }
  }
  void unlock() { held.store(false, std::memory_order_release); }
};
}  // namespace gg

struct gg_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  int num_cus = 256;

  // ---- staging ----
  // mu: vertex staging, device columns, block flushes and everything slow.  edge_spin: the reservation
  // state of the edge blocks (cur_e, fill, base, has_rowid, OPEN/CLOSED, n_edges, implicit ranges).
  // Lock order: mu before edge_spin.
  std::mutex mu;
  gg::SpinLock edge_spin;
  std::condition_variable cv;                    // an edge block became FREE / the open block changed
  gg::Column c_vid, c_src, c_dst, c_rowid;
  uint64_t n_vertices = 0, n_edges = 0;          // rows resident, in flight to the device or reserved in a block
  bool rowid_explicit = false;                   // some append passed explicit rowids
  // rows appended without rowids, as merged (first row, count) ranges: their rowid is their position and
  // is only written (on the device, at build time) if some other append did pass rowids
  std::vector<std::pair<uint64_t, uint64_t>> implicit_rowid_ranges;
  static constexpr size_t STAGE_ROWS = 1u << 20; // rows per pinned staging block
  int64_t *pin_v[2] = {nullptr, nullptr};        // vertex ids
  hipEvent_t pin_v_free[2] = {nullptr, nullptr};
  int cur_v = 0;
  size_t fill_v = 0;
  // Edge blocks: [src | dst | rowid], each STAGE_ROWS.  Appenders reserve a row range under mu and copy
  // into the block OUTSIDE the lock (concurrent Sink calls overlap their memcpys); whoever reserves the
  // last row closes the block, opens the other one for everybody else, waits for the block's other
  // writers and sends it to the device.
  struct EdgeBlock {
    int64_t *pin = nullptr;
    hipEvent_t free_ev = nullptr;  // recorded after the block's H2D copies
    size_t fill = 0;               // rows reserved
    uint64_t base = 0;             // position of the block's first row in the staged columns
    std::atomic<int> writers{0};   // reservations whose memcpy has not finished (not guarded by mu)
    bool has_rowid = false;        // some reservation in the block carries explicit rowids
    enum State { OPEN, CLOSED, FREE } state = FREE;
  };
  // A ring of blocks (two: a ring of four staged SF100's edge table no faster, 33 GB/s on the box where both were
  // measured — 8 MB copies back to back reach 54 GB/s, scripts/ubench_h2d.hip: it is the host side that fills the
  // blocks at that pace, not the copy engine that waits for it)
  static constexpr int EDGE_BLOCKS = 2;
  EdgeBlock eblk[EDGE_BLOCKS];
  int cur_e = 0;                                 // the OPEN block

  // ---- pinned host buffers handed out by gg_host_alloc (guarded by host_mu) ----
  struct HostBlock {
    void *ptr;
    size_t bytes;
    bool in_use;
  };
  std::mutex host_mu;
  std::vector<HostBlock> host_blocks;

  // ---- caching device allocator ----
  // pool_mu: compute calls on one context are externally serialised, but results of earlier calls are
  // destroyed (their blocks freed) from whatever thread finishes with them
  mutable std::mutex pool_mu;  // (mutable: gg_debug_pool_fill reads the counters of a const context under it)
  std::vector<gg::DevBlock> blocks;
  size_t bytes_allocated = 0;

  // ---- profiling ----
  int force_frontier = 0;  // gg_debug_force_frontier: 1 frontier kernels only, 2 product form of the last hop at any size
  bool rank_mode_forced = false;  // rank_mode was set by gg_debug_rank_mode, not decided by the probe
  int rank_mode = 0;            // gg_debug_rank_mode: 0 probe the LDS atomic order once, 1 ds_add_rtn ranks, 2 match masks
  bool legacy_build = false;    // gg_debug_force_legacy_build: the multi-pass LSD build (also taken for > 2^22 vertices)
  bool keep_edge_rowid = true;  // gg_ctx_set_edge_rowid
  bool mirror_pairs = true;     // GG_MIRROR_PAIRS=0 at context creation: whole builds and the endpoint set never pair row i
                                // with row i + E/2 (gg_csr_fast.hip, k_set_insert2); results are the same either way
  bool mirror_reverse = true;   // GG_MIRROR_REVERSE=0 at context creation (GG_MIRROR_PAIRS=0 implies it): the bucketed build
                                // never derives the reverse CSR of a fully mirrored table from its forward rows
  uint64_t max_grid_tiles = 0;  // gg_debug_max_grid_tiles: workgroups per expansion launch (0: the hardware bound)
  int reach_visited_mode = 0;   // gg_debug_reach_visited: 0 the budget decides, 1 bitmap, 2 hash set (gg_reach.hip)
  uint64_t reach_hash_slots = 0;  // gg_debug_reach_visited: the hash set's first capacity (0: from the seed count)
  int levels_set_mode = 0;      // gg_debug_level_sets: 0 the budget decides, 1 bitmap, 2 hash set (gg_levels.hip)
  int levels_order_mode = 0;    // gg_debug_level_sets: 0 the byte model decides per level, 1 sort, 2 compact
  uint32_t tri_lds_entries = 0; // gg_debug_triangle_tile: entries of an in-row gg_triangles may stage in LDS (0: the default)
  uint32_t agg_long_row = 0;    // gg_debug_aggregate_long_row: rows of more entries go to a workgroup each (0: the default)
  int agg_top_route = 0;        // gg_debug_aggregate_top: 0 the survivor count decides, 1 the LDS sort, 2 the global passes
  uint32_t agg_top_floor = 0;   // gg_debug_aggregate_top: candidates at which the selection compacts them (0: the default)
  uint32_t pc_long_row = 0;     // gg_debug_pair_counts: in-rows of more entries go to a workgroup each (0: the default)
  int pc_gather_mode = 0;       // gg_debug_pair_counts: 0 entries whose mask is 0 are skipped, 1 every state row is read
  uint32_t cp_long_row = 0;     // gg_debug_cheapest: in-rows of more entries go to a workgroup each (0: the default)
  int cp_gather_mode = 0;       // gg_debug_cheapest: 0 entries whose mask is 0 are skipped, 1 every entry counts as live
  int cc_init_mode = 0;         // gg_debug_components: 0 the default start of the forest, 1 every vertex its own root (the same)
  uint32_t cc_jumps_per_check = 0;  // gg_debug_components: pointer-doubling launches per look at the changed word (0: the default)
  uint32_t extend_tile_rows = 0;    // gg_debug_extend: output rows per workgroup of gg_result_extend_edge's write pass (0: the default)
  int group_route = 0;              // gg_debug_group: 0 the key count decides, 1 the LDS table where it fits, 2 the global cells
  uint32_t group_lds_keys = 0;      // gg_debug_group: keys the workgroup-private table of gg_result_group_by may hold (0: the default)
  int val_top_route = 0;            // gg_debug_value_top: as agg_top_route, for gg_result_top_rows
  uint32_t val_top_floor = 0;       // gg_debug_value_top: as agg_top_floor
  uint64_t distinct_slots = 0;      // gg_debug_distinct: slots of gg_result_distinct's table (0: the default), rounded up there
  int distinct_combine = 0;         // gg_debug_distinct: 0 adjacent equal lanes are combined, 1 every row probes
  int tuple_route = 0;              // gg_debug_group_tuples: 0 the group count decides, 1 the LDS cells where they fit, 2 the global cells
  uint32_t tuple_lds_groups = 0;    // gg_debug_group_tuples: groups the workgroup-private cells of gg_result_group_tuples may hold (0: the default)
  bool cc_size_fold = true;     // GG_CC_SIZE_FOLD=0 at context creation: gg_components adds sizes per lane, never per wave
                                // (a measurement switch, scripts/bench_components.py; sizes are the same either way)
  uint64_t agg_top_listed = 0;  // gg_debug_aggregate_top_listed: list entries the last gg_khop_aggregate_top compacted to
  std::vector<uint64_t> bfs_steps;  // gg_debug_bfs_steps: (n_active, te, reached, cur) of levels 0..ran of the last bfs_run
  int bfs_cell_bytes = 0;           // gg_debug_bfs_steps: sizeof(DistT) of that run (0: no run since the last reset)
  bool profiling = false;
  std::vector<std::string> prof_names;
  std::vector<uint64_t> prof_launches;
  std::vector<double> prof_ms;
  std::vector<gg::ProfRec> prof_pending;
  std::vector<hipEvent_t> prof_event_pool;   // events are reused: creating two per launch costs more than timing
  std::vector<std::string> prof_selected;    // gg_profile_select: time only these kernels (empty: all)

  // small pinned scratch for D2H of counters: 64 x u64, laid out per call by gg::read_back (word 63: copy of dev_err).
  // The only other users are the multi-pass build's H2D seeds (gg_csr.hip) and the bucketed build's early status below.
  uint64_t *pin_scratch = nullptr;
  // the bucketed build's status words are final long before its last kernel: copied to pin_scratch behind the
  // column scan, status_ev recorded behind the copy — gg_csr_build waits for that, not for the stream
  hipEvent_t status_ev = nullptr;
  bool status_early = false;
  unsigned long long *dev_err = nullptr;  // device word: != 0 after a chained scan gave up waiting
  bool scan_pending = false;              // a chained scan was launched since dev_err was last fetched (gg::read_back)
  uint32_t scan_spin_limit = 1u << 24;    // polls per predecessor before a scan tile gives up
  uint64_t scan_mute_tile = ~0ull;        // gg_debug_scan_fault: this scan tile never publishes (tests)

  unsigned long long *stats_dev = nullptr;  // gg_expand_khop_dev: the six result words of the last such call (8 x u64)
  hipEvent_t xstream_event = nullptr;       // gg_stream_wait
  // Result fetches (gg_result_fetch[_edges]) go over FETCH_LANES streams of their own, round robin: the pipeline's
  // threads drain a result in copies of ~1 MB per column, and one stream moves copies of that size at 33-37 GB/s
  // (a gap between copies; profiles/r04_ubench_h2d_numa.txt: 1 MiB pieces 36.6 GB/s on one stream, 51-55 on two or
  // four), so the lanes overlap one copy's tail with the next one's head.  A lane is ordered behind the library's
  // stream by an event per call (the result may still be in flight there) and serialises its own callers.
  static constexpr int FETCH_LANES = 4;
  struct FetchLane {
    hipStream_t stream = nullptr;
    hipEvent_t ready = nullptr;
    std::mutex mu;
  };
  FetchLane fetch_lane[FETCH_LANES];
  std::atomic<uint32_t> fetch_next{0};
  uint32_t fetch_lanes_used = FETCH_LANES;  // GG_FETCH_LANES (1..FETCH_LANES)
  // copy n_cols column slices to the host over one lane and wait for them (dst[c] <- src[c], bytes each)
  int fetch_columns(void *const *dst, const void *const *src, int n_cols, size_t bytes);

  uint64_t next_serial = 1;
  // GG_POOL_FILL=<0..255> at context creation: every block dev_alloc hands out, fresh or recycled, is set to that byte over
  // its whole size first (DESIGN.md "Scratch is never assumed zero"); -1: off.  gg_debug_reset leaves it alone.
  int pool_fill = -1;
  uint64_t pool_blocks_filled = 0, pool_bytes_filled = 0;  // since the context was created (gg_debug_pool_fill)
  int fill_block(void *p, size_t size);
  int dev_alloc(void **out, size_t bytes);
  // Three result columns of col_bytes each that will be written in lockstep (k_mat_mid2).  Small ones share one pooled
  // block; large ones are three blocks chosen so that they lie in different memory ranks (gg_runtime.hip "Placement"),
  // kept together as a set and recycled as a set.  cols[0..2] are freed individually with dev_free.
  int dev_alloc_columns(void **cols, size_t col_bytes);
  struct PlacedSet {
    void *col[3];
    size_t bytes;  // per column
  };
  std::vector<PlacedSet> placed_sets;
  int place_probes = 12;                                       // GG_PLACE_PROBES: at most this many candidate blocks per set (<= 3: no probing)
  uint64_t placed_built = 0, placed_fast_pairs = 0;            // diagnostics: sets built, fast pairs in the last one
  void dev_free(void *p);
  void keep(void *p);  // the block outlives the API call that allocated it
  int prof_begin(const char *name);
  void prof_end(int rec);
  int prof_flush();
};

struct gg_csr {
  gg_ctx *ctx = nullptr;
  uint64_t V = 0, E = 0, dropped = 0;
  uint64_t E_cap = 0;          // allocation size of the per-edge arrays (= staged edge rows)
  uint64_t E_rev = 0;          // entries of the reverse CSR (== E unless this is a shard)
  uint64_t owned_vertices = 0; // vertices owned by this shard (== V unless this is a shard)
  int part = 0, n_parts = 1;   // shard identity (gg_csr_build_shard)
  bool has_rowid = true;       // epos/eid valid (gg_ctx_set_edge_rowid, never for shards)
  uint32_t *off = nullptr;     // V+1 row offsets
  uint32_t *nbr = nullptr;     // E   dense neighbour (destination) per entry
  uint32_t *row = nullptr;     // E   dense source per entry (COO view, sorted by source)
  uint32_t *epos = nullptr;    // E   append position of the edge row (implicit rowid)
  int64_t *eid = nullptr;      // E   explicit edge rowids (only if the Sink passed rowids), else null
  int64_t *vid = nullptr;      // V   vertex ids by dense index
  gg::HtSlot *ht = nullptr;    // id hash table (open addressing, 16-byte slots: one line per probe)
  bool ht_built = false;       // filled at build time only if the densification needed it; else on first use (ensure_ht)
  uint64_t ht_cap = 0;         // slots; slot = mulhi(key * GOLD, ht_cap)
  int64_t ht_min_idx = -1;     // dense index of the vertex whose id == HT_EMPTY, if any
  // reverse CSR (in-neighbours): row x lists the sources u of every edge u->x — in ascending (u, rowid) order when
  // ensure_reverse() built it lazily, in rowid order when the bucketed build made it (gg_csr_fast.hip)
  uint32_t *roff = nullptr;    // V+1
  // E   source u of the reverse entry.  NULL on a derived build (rev_derived) until ensure_reverse() rotates the
  // forward rows into it: every reader goes through ensure_reverse() first; ensure_reverse_index() does not write it
  uint32_t *rnbr_rows = nullptr;
  // E   destination x of the reverse entry (COO view, sorted by x): the row-index expansion of roff.  NULL on a derived
  // build until ensure_reverse_index() expands the offsets into it: every reader goes through that (or ensure_reverse())
  // first; ensure_reverse_offsets() does not write it, and the counting 2-hop expansion never reads it
  uint32_t *rrow_index = nullptr;
  bool rev_derived = false;    // the bucketed build derived roff from the forward rows (fully mirrored table): roff == off
  // V   derived builds: |A| of every vertex, the first-half entries its forward row starts with.  The reverse row is
  // the forward row rotated by it (B ++ A), which is what ensure_reverse() writes on first use
  uint32_t *rot = nullptr;
  // the reverse rows again with their sources ascending (gg_paths.hip: ensure_reverse_by_source, whole CSRs, on first
  // use by gg_bfs64_paths or gg_triangles): the bucketed build leaves rnbr's rows in rowid order, which a pull does not mind and a path trace does
  uint32_t *rnbr_by_src = nullptr;  // E
  // the forward CSR position of every entry of rnbr_by_src (gg_paths.hip: ensure_reverse_pos_by_source, on first use by
  // gg_triangles_edges only): equal sources of a row stand in ascending forward position, which is append order
  uint32_t *rpos_by_src = nullptr;  // E
  // the reverse entries grouped by SOURCE (gg_bfs.hip: ensure_push_in, shards only, on first use): row u lists
  // the owned destinations of u's edges, so a shard can push a light frontier into the words it owns
  uint32_t *pin_off = nullptr; // V+1
  uint32_t *pin_nbr = nullptr; // E_rev
};

// What a device result holds and which calls read it.  The kinds from AGGREGATE on were born with a refusal contract:
// every call but their own answers them with GG_ERR_STATE, and theirs answer every other kind so (gg::expect_kind).
enum class ResultKind { TABLES, WALK_CLOSURE, REACH, LEVEL_SETS, PATHS, AGGREGATE, PAIR_COUNTS, COMPONENTS, ALL_PATHS, CHEAPEST,
                        CHEAPEST_PATHS, TUPLE_GROUPS };

// kind          tables and columns (h: a level in k_min..k_max)                     read by
// TABLES        rows[h], cols[h][0..h] = ids v0..vh; ecols[h][j] = rowid of the     gg_result_rows / _fetch / _fetch_edges /
//               (j + 1)-th edge if asked for; tri_edges: ecols[2][0..2] = e1, e2,   _digest / _filter_* / _extend_edge,
//               e3 of a triangle row                                                gg_triangles_fetch_edges, gg_result_group_by,
//                                                                                   gg_result_top_rows, gg_result_distinct,
//                                                                                   gg_result_group_tuples
// WALK_CLOSURE  rows[0] walks level by level, level_rows[L - 1] those of L edges;   gg_walk_closure_levels / _fetch
//               cols[0][0..1] = index of the seed, rowid of the last edge
// REACH         the same; cols[0][0..1] = class, vertex id of level L's new pairs   gg_reach_closure_levels / _fetch
// LEVEL_SETS    the same; cols[0][0..1] = class, vertex id of level L's members     gg_level_sets_levels / _fetch
// PATHS         rows[PATHS_TABLE], cols[..][0..3] = pair index, vertex id, step     gg_bfs64_paths_rows / _fetch
//               (int32 cells), edge rowid if asked for
// AGGREGATE     rows[h] groups, cols[h][0..3] = vertex id, walks, total low, high   gg_khop_aggregate_rows / _fetch / _top
//               (gg_khop_aggregate_top: one level, in rank order; gg_result_group_by: one level)
// PAIR_COUNTS   rows[h] pairs, cols[h][0..2] = source index, vertex id, walks       gg_khop_pair_counts_rows / _fetch
// COMPONENTS    rows[0] = V, cols[0][0..2] = vertex id, component id, size;         gg_components_rows / _fetch / _fetch_sizes
//               rows[1] components, cols[1][0..1] = component id, size
// ALL_PATHS     rows[AP_PAIRS_TABLE], cols[..][0..3] = pair index, hops (int32      gg_bfs64_all_paths_rows / _fetch_pairs /
//               cells), paths, kept; rows[AP_ROWS_TABLE], cols[..][0..4] = pair     _fetch
//               index, path index, step (int32 cells), vertex id, edge rowid if
//               asked for
// CHEAPEST      rows[0], cols[0][0..3] = source index, vertex id, cost, hops (int32     gg_cheapest64_rows / _fetch
//               cells)
// CHEAPEST_PATHS  rows[CPP_PAIRS_TABLE], cols[..][0..3] = pair index, cost, hops,     gg_cheapest64_paths_rows / _fetch_pairs /
//               traced (both int32 cells); rows[CPP_ROWS_TABLE], cols[..][0..4] =    _fetch
//               pair index, step (int32 cells), vertex id, edge rowid if asked for,
//               cost
// TUPLE_GROUPS  rows[0] groups, k_min = k_max = key columns - 1; cols[0][j] = key      gg_tuple_groups_rows / _fetch
//               column j; cols[1][0..5] = rows, valued, sum low, sum high, min, max
//               (the count form has cols[1][0] alone: the others read as 0)
struct gg_result {
  gg_ctx *ctx = nullptr;
  ResultKind kind = ResultKind::TABLES;
  int k_min = 0, k_max = -1;  // the levels that have a table (TABLES, AGGREGATE, PAIR_COUNTS; none otherwise)
  uint64_t rows[GG_MAX_HOPS + 1] = {0};
  int64_t *cols[GG_MAX_HOPS + 1][GG_MAX_HOPS + 1] = {{nullptr}};   // cols[h][c], device
  int64_t *ecols[GG_MAX_HOPS + 1][GG_MAX_HOPS + 1] = {{nullptr}};  // ecols[h][j], device
  std::vector<uint64_t> level_rows;  // the closures and the level sets: rows of level L at [L - 1]
  bool tri_edges = false;            // TABLES of gg_triangles_edges
};

namespace gg {

// Put one at the top of every C-ABI entry point that allocates: whatever the call allocated from the pool
// and neither freed nor handed to a long-lived object (gg_ctx::keep) goes back to the pool when the call
// returns — including every early error return.
//
// The rules of an entry point: every launch goes through GG_LAUNCH; caller ids reach the device through upload_ids;
// a result (or any other C-ABI object) under construction is held by an Owner and release()d only on success;
// a result is made by make_result with its ResultKind, every call that reads one starts with expect_kind, and rows leave
// through fetch_slice;
// failures return at once through GG_TRY / GG_HIP, and the ApiScope frees the pool blocks; every host synchronisation
// of a compute call is read_back / sync_checked, which test the chained scans' error word whenever a scan ran.  An
// explicit dev_free is only worth writing where it lowers the pool's peak, i.e. before a later allocation in the same
// call.
// An operator over the rows of a walk table (gg_walk_table.h) checks its table through result_arg / walk_kind_arg / hops_arg
// / whole_csr_arg / column_arg / id_columns_present, in the order its checks always had (two faults at once are answered
// with the first check's code); takes a dictionary as a DictView from dict_view and a value column from value_column;
// allocates its result's columns with alloc_kept_columns and splits a launch with split_groups.
struct ApiScope {
  gg_ctx *ctx;
  uint64_t mark;
  explicit ApiScope(gg_ctx *c) : ctx(c), mark(c ? c->next_serial : 0) {}
  ~ApiScope() {
    if (!ctx) return;
    std::lock_guard<std::mutex> lk(ctx->pool_mu);
    for (auto &b : ctx->blocks)
      if (b.in_use && !b.keep && b.serial >= mark) b.in_use = false;
  }
};

// Owns a C-ABI object under construction: Destroy runs on every early return unless the object was release()d.
template <typename T, void (*Destroy)(T *)>
struct DestroyWith {
  void operator()(T *p) const { Destroy(p); }
};
template <typename T, void (*Destroy)(T *)>
using Owner = std::unique_ptr<T, DestroyWith<T, Destroy>>;
using ResultOwner = Owner<gg_result, gg_result_destroy>;

// The one rule for a result handed to a call that reads another kind (include/gg.h): GG_ERR_STATE if either kind was born
// with a refusal contract, GG_ERR_INVALID_ARG among the five older kinds, and for a NULL result.
struct KindName {
  const char *holds, *readers;
};
constexpr KindName KIND_NAMES[] = {
    {"fixed-length walk tables", "gg_result_rows / gg_result_fetch / gg_result_fetch_edges"},
    {"a walk closure", "gg_walk_closure_levels / gg_walk_closure_fetch"},
    {"a reach closure", "gg_reach_closure_levels / gg_reach_closure_fetch"},
    {"level sets", "gg_level_sets_levels / gg_level_sets_fetch"},
    {"shortest paths", "gg_bfs64_paths_rows / gg_bfs64_paths_fetch"},
    {"grouped aggregates", "gg_khop_aggregate_rows / gg_khop_aggregate_fetch"},
    {"pair counts", "gg_khop_pair_counts_rows / gg_khop_pair_counts_fetch"},
    {"components", "gg_components_rows / gg_components_fetch[_sizes]"},
    {"all shortest paths", "gg_bfs64_all_paths_rows / _fetch_pairs / _fetch"},
    {"cheapest path costs", "gg_cheapest64_rows / gg_cheapest64_fetch"},
    {"cheapest paths", "gg_cheapest64_paths_rows / _fetch_pairs / _fetch"},
    {"aggregates per key tuple", "gg_tuple_groups_rows / gg_tuple_groups_fetch"},
};
static_assert(sizeof(KIND_NAMES) / sizeof(KIND_NAMES[0]) == (size_t)ResultKind::TUPLE_GROUPS + 1, "a name per kind");
inline int expect_kind(const gg_result *res, ResultKind want, const char *fn) {
  if (!res) return GG_ERR_INVALID_ARG;
  if (res->kind == want) return GG_OK;
  if (res->kind < ResultKind::AGGREGATE && want < ResultKind::AGGREGATE) return GG_ERR_INVALID_ARG;
  const KindName &has = KIND_NAMES[(int)res->kind];
  set_error("%s reads %s, but the result holds %s (%s read it)", fn, KIND_NAMES[(int)want].holds, has.holds, has.readers);
  return GG_ERR_STATE;
}

inline ResultOwner make_result(gg_ctx *ctx, ResultKind kind, int k_min = 0, int k_max = -1) {
  ResultOwner res(new gg_result());
  res->ctx = ctx;
  res->kind = kind;
  res->k_min = k_min;
  res->k_max = k_max;
  return res;
}

// Rows [offset, offset + max_rows) of a table of `total` rows to the host: the range is clamped to the table, *n_out is
// its length, and every column that has both a destination and a device array is copied — one fetch_columns call per cell
// width, as many as the readers ever made (gg_runtime.hip).  A reader keeps its own required-argument checks.
struct SliceCol {
  void *dst;         // host, NULL: not asked for
  const void *base;  // device, row 0 of the column; NULL: the result has none
  size_t cell = sizeof(int64_t);  // bytes per cell: 8 or 4
};
int fetch_slice(gg_ctx *ctx, uint64_t total, uint64_t offset, uint32_t max_rows, const SliceCol *cols, int n_cols,
                uint32_t *n_out);
inline int fetch_slice(gg_ctx *ctx, uint64_t total, uint64_t offset, uint32_t max_rows, std::initializer_list<SliceCol> cols,
                       uint32_t *n_out) {
  return fetch_slice(ctx, total, offset, max_rows, cols.begin(), (int)cols.size(), n_out);
}

// RAII-free helper: launch wrapper that records events when profiling is on.
// (A launch of 2^32 threads or more is not refused by the runtime: the global size WRAPS and the kernel silently covers
// a fraction of its input — seen with one thread per endpoint of 2.4 G edge rows.  Kernels over that many items stride;
// the macro refuses whatever would still get there.)
#define GG_LAUNCH(ctx, name, kernel, grid, block, shmem, ...)                         \
  do {                                                                                \
    {                                                                                 \
      const dim3 g_ = (grid), b_ = (block);                                           \
      if ((unsigned long long)g_.x * g_.y * g_.z * b_.x * b_.y * b_.z >= (1ULL << 32)) { \
        set_error(name ": a launch of 2^32 threads or more");                         \
        return GG_ERR_TOO_LARGE;                                                      \
      }                                                                               \
    }                                                                                 \
    int prof_rec_ = (ctx)->profiling ? (ctx)->prof_begin(name) : -1;                  \
    hipLaunchKernelGGL(kernel, grid, block, shmem, (ctx)->stream, __VA_ARGS__);       \
    if (prof_rec_ >= 0) (ctx)->prof_end(prof_rec_);                                   \
    GG_HIP(hipGetLastError());                                                        \
  } while (0)

// Load-balanced expansion over a flattened frontier (gg_khop.hip, gg_closure.hip): entry i of a frontier owns the child
// positions [foff[i], foff[i+1]); a workgroup of XT threads takes XT consecutive positions, tile_entry[t] being the
// entry that tile t starts in (make_tiles_u64: one binary search per tile).
constexpr int XT = 256;  // child positions per tile == threads per workgroup
int make_tiles_u64(gg_ctx *ctx, const uint64_t *foff, uint64_t n_entries, uint64_t M, uint32_t **tile_entry,
                   uint64_t *n_tiles);
// GG_ERR_INVALID_ARG for a bad context / CSR pair, GG_ERR_STATE for a shard (gg_csr_build_shard): calls that need a
// whole CSR
int check_whole_csr(gg_ctx *ctx, const gg_csr *csr);

// exclusive scan of n uint32 values (in place allowed: out may equal in); writes the grand
// total (as uint64) to *total_dev if non-null.  One hand-written kernel, tiles chained by decoupled
// look-back (gg_runtime.hip).  Sums are kept in 64 bits: the u32 form writes each prefix mod 2^32 and the total exactly.
// The grand total must stay below 2^62 — a tile's status word carries its flag in the top two bits and its sum or prefix
// in the other 62, so a larger sum would be read as another flag; no caller sums anything but counts of rows.
int scan_exclusive_u32(gg_ctx *ctx, const uint32_t *in, uint32_t *out, uint64_t n, uint64_t *total_dev);
// exclusive scan of n uint64 values
int scan_exclusive_u64(gg_ctx *ctx, const uint64_t *in, uint64_t *out, uint64_t n, uint64_t *total_dev);

// The host synchronisation of a compute call: the items' D2H copies (through consecutive 8-byte-aligned words of
// ctx->pin_scratch) are queued on ctx->stream, the stream is synchronised ONCE, and the words are copied to each `host`.
// If a chained scan ran since the last such synchronisation, its error word travels along and a scan that gave up makes
// this GG_ERR_HIP.  More bytes than the scratch holds below the error word are refused (GG_ERR_STATE).
struct ReadBack {
  const void *dev;
  size_t bytes;
  void *host;
};
int read_back(gg_ctx *ctx, const ReadBack *items, size_t n_items);
inline int read_back(gg_ctx *ctx, std::initializer_list<ReadBack> items) {
  return read_back(ctx, items.begin(), items.size());
}
inline int sync_checked(gg_ctx *ctx) { return read_back(ctx, nullptr, 0); }
// scan_exclusive_* with the grand total read back to *total_host (one read_back, `extra` items riding on it);
// append_total: out has n + 1 entries and out[n] = the total
int scan_total_u32(gg_ctx *ctx, const uint32_t *in, uint32_t *out, uint64_t n, uint64_t *total_host);
int scan_total_u64(gg_ctx *ctx, const uint64_t *in, uint64_t *out, uint64_t n, uint64_t *total_host,
                   bool append_total = false, std::initializer_list<ReadBack> extra = {});
// degrees (u64, n entries) -> exclusive offsets (n + 1 entries) in place, *total_host their sum
inline int offsets_from_deg(gg_ctx *ctx, uint64_t *deg_then_off /* n+1 */, uint64_t n, uint64_t *total_host,
                            std::initializer_list<ReadBack> extra = {}) {
  return scan_total_u64(ctx, deg_then_off, deg_then_off, n, total_host, true, extra);
}

// id -> dense lookup of n device ids; writes dense (uint32, INVALID_U32 if absent) to out_dev
int lookup_ids(gg_ctx *ctx, const gg_csr *csr, const int64_t *ids_dev, uint64_t n, uint32_t *out_dev);
// Caller ids -> dense indices: allocates *dense (and the device copy of the ids, handed back in *ids_dev if that is
// non-null) from the pool, n entries but at least one, and enqueues the copy of `ids` and lookup_ids.  It does NOT
// synchronise: `ids` is caller memory, and every entry point that calls this reaches a stream synchronisation before
// it returns, so the copy has read it by then.
int upload_ids(gg_ctx *ctx, const gg_csr *csr, const int64_t *ids, uint64_t n, uint32_t **dense,
               int64_t **ids_dev = nullptr);
// n (key, value) pairs of u32 sorted by key < 2^key_bits, stably, into (key_out, val_out) — device arrays (gg_csr.hip).
// The contract, for the triples as well:
//   - key 0xFFFFFFFF (INVALID_U32) means "no element" to the radix kernels, whatever key_bits says: such an element is
//     not counted and not written, the elements after it move up, the outputs' last slots keep what they held, and the
//     passes after the first see only the others.  A caller either has no such key or means exactly that (the builds'
//     dropped edges) and then knows the number of valid keys from elsewhere: these two entry points do not report it.
//   - so a whole 32-bit word can NOT be a key.  key_bits >= 32 is refused (GG_ERR_INVALID_ARG, "internal: ..."); wider
//     keys are sorted in pieces of fewer bits, lowest piece first (gg_triangles.hip's ranks, gg_aggregate_top.hip, the id
//     sort of gg_csr.hip), which is what stability is for.  key_bits < 1 counts as 1.  The callers that sort by dense
//     vertex index (gg_khop.hip, gg_reach.hip, gg_paths.hip) take their bits from V, so a graph of more than 2^31
//     vertices meets this refusal there; its indices would never be 0xFFFFFFFF (V <= 2^32 - 2), but no such graph has
//     been built, and two pieces are the way to serve it.
//   - bits of a valid key at or above key_bits are ignored, not refused: elements that differ only there keep their
//     input order.
//   - n < 2^32 (positions are 32-bit counters); no output may alias an input; n == 0 launches nothing.
int sort_pairs_by_key(gg_ctx *ctx, const uint32_t *key, const uint32_t *val, uint64_t n, int key_bits, uint32_t *key_out,
                      uint32_t *val_out);
int sort_triples_by_key(gg_ctx *ctx, const uint32_t *key, const uint32_t *a, const uint32_t *b, uint64_t n, int key_bits,
                        uint32_t *key_out, uint32_t *a_out, uint32_t *b_out);
// make a staged column hold need_rows rows, keeping the first live_rows (gg_runtime.hip; caller holds mu)
int grow_column(gg_ctx *ctx, Column &c, size_t live_rows, size_t need_rows);
// GG_STAGING_TRACE=1: print and reset the edge staging's waiting-time counters (gg_runtime.hip)
void staging_trace_print();
// The reverse CSR at three levels (gg_csr.hip); each builds what is absent and includes the levels above it.
// offsets: csr->roff only, for callers that read nothing else (the counting 2-hop expansion, the work estimate of
// gg_khop_partition_mid).  A derived build has them: nothing is launched.
int ensure_reverse_offsets(gg_ctx *ctx, gg_csr *csr);
// index: csr->roff and csr->rrow_index, for callers that read the COO column but not the reverse rows.  On a derived
// build without the index: one kernel on the context's stream that expands the offsets into it, no host synchronisation
int ensure_reverse_index(gg_ctx *ctx, gg_csr *csr);
// rows: csr->roff, csr->rrow_index and csr->rnbr_rows.  A derived build left csr->rot: the rows are then the index
// kernel and one rotation kernel on the context's stream, no host synchronisation
int ensure_reverse(gg_ctx *ctx, gg_csr *csr);
// build csr->rnbr_by_src if absent: the reverse rows with their sources ascending, under csr->roff (gg_paths.hip)
int ensure_reverse_by_source(gg_ctx *ctx, gg_csr *csr);
// build csr->rpos_by_src if absent: the same sort carrying the forward CSR position (gg_paths.hip)
int ensure_reverse_pos_by_source(gg_ctx *ctx, gg_csr *csr);
// fill csr->ht from csr->vid if the build did not need it (gg_csr.hip); every ht_lookup user calls this first
int ensure_ht(gg_ctx *ctx, gg_csr *csr);
// bucketed two-level build of forward + reverse CSR (gg_csr_fast.hip); *taken = 0 if the graph is outside
// its range (> 2^22 vertices) and nothing was launched
int csr_build_fast(gg_ctx *ctx, gg_csr *csr, BuildStatus *st, int *taken);

__device__ __forceinline__ uint64_t fmix64(uint64_t x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdULL;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ULL;
  x ^= x >> 33;
  return x;
}
__device__ __forceinline__ uint64_t dig_q(uint64_t p, int j) { return fmix64(p + DIG_GOLD * (uint64_t)(j + 1)); }
__device__ __forceinline__ uint64_t dig_leaf(uint64_t q, uint32_t d) {
  return q ^ ((uint64_t)d * (uint64_t)DIG_K32);  // one v_mad_u64_u32
}

// slot of a key in a table of `cap` slots (any capacity, not only powers of two): multiplicative hash,
// then multiply-high range reduction; linear probing wraps at cap
__device__ __forceinline__ uint64_t ht_slot(int64_t key, uint64_t cap) {
  // Fibonacci hashing.  Database keys are mostly (pieces of) arithmetic progressions, which one odd multiplication
  // spreads almost evenly — shorter probe runs than a random function gives at the same load factor (measured at
  // SF100: a murmur-style finaliser here made the inserts 2.4x and the edge densification 2.7x slower).
  return __umul64hi((uint64_t)key * DIG_GOLD, cap);
}
__device__ __forceinline__ uint64_t ht_next(uint64_t slot, uint64_t cap) { return slot + 1 == cap ? 0 : slot + 1; }

__device__ __forceinline__ uint32_t ht_lookup(const HtSlot *__restrict__ ht, uint64_t cap,
                                              int64_t min_idx, int64_t key) {
  if (key == HT_EMPTY) return min_idx >= 0 ? (uint32_t)min_idx : INVALID_U32;
  uint64_t slot = ht_slot(key, cap);
  while (true) {
    // one 16-byte load per probe: key and value share a cache line
    const uint4 raw = *reinterpret_cast<const uint4 *>(&ht[slot]);
    const int64_t k = (int64_t)(((uint64_t)raw.y << 32) | raw.x);
    if (k == key) return raw.z;
    if (k == HT_EMPTY) return INVALID_U32;
    slot = ht_next(slot, cap);
  }
}

// finish a lookup whose first probe (slot, raw) is already loaded; continues linear probing on a miss
__device__ __forceinline__ uint32_t ht_resolve(const HtSlot *__restrict__ ht, uint64_t cap, int64_t min_idx,
                                               int64_t key, uint64_t slot, uint4 raw) {
  if (key == HT_EMPTY) return min_idx >= 0 ? (uint32_t)min_idx : INVALID_U32;
  while (true) {
    const int64_t k = (int64_t)(((uint64_t)raw.y << 32) | raw.x);
    if (k == key) return raw.z;
    if (k == HT_EMPTY) return INVALID_U32;
    slot = ht_next(slot, cap);
    raw = *reinterpret_cast<const uint4 *>(&ht[slot]);
  }
}

// Mirrored halves: an undirected edge table loaded twice, the second time with the id columns swapped, has row i + h =
// (dst[i], src[i]) for h = E / 2.  Whole builds look at up to MIRROR_SAMPLES rows spread over [0, h) first (threads
// i < n of some grid, whole waves calling): tally[0] += rows looked at, tally[1] += rows mirrored; they pair rows only if
// mirror_pays(tally) — on a table without such pairs the paired walk costs a few percent.
constexpr uint64_t MIRROR_SAMPLES = 4096;
__device__ __forceinline__ void mirror_sample(const int64_t *__restrict__ src, const int64_t *__restrict__ dst, uint64_t h,
                                              uint64_t i, uint64_t nthreads, uint32_t *__restrict__ tally) {
  uint64_t n = h < MIRROR_SAMPLES ? h : MIRROR_SAMPLES;
  n = n < nthreads ? n : nthreads;
  bool m = false;
  if (i < n) {
    const uint64_t r = i * h / n;
    m = src[r + h] == dst[r] && dst[r + h] == src[r];
  }
  const uint64_t in = __ballot(i < n), mm = __ballot(m);
  if ((threadIdx.x & 63) == 0 && in) {
    atomicAdd(&tally[0], (uint32_t)__popcll(in));
    if (mm) atomicAdd(&tally[1], (uint32_t)__popcll(mm));
  }
}
__device__ __forceinline__ bool mirror_pays(const uint32_t *__restrict__ tally) {  // a quarter of the rows or more
  return tally[1] > 0 && 4ull * tally[1] >= tally[0];
}

// shard ownership of a vertex id: independent of table order, so every rank decides it alone
__device__ __forceinline__ bool owns(int64_t id, uint32_t part, uint32_t n_parts) {
  // owner = floor(h32 * n_parts / 2^32) with h32 the high half of the multiplicative hash (no division)
  return n_parts <= 1 || (uint32_t)((((((uint64_t)id * DIG_GOLD) >> 32)) * (uint64_t)n_parts) >> 32) == part;
}

// Digest sums are 32-bit: the LOW half of each row hash, summed mod 2^32 (carried in u64 fields whose
// high half stays zero).  One v_xad_u32 (xor + add) per walk in the product kernel.
__host__ __device__ __forceinline__ uint64_t dsum_add(uint64_t a, uint64_t b) {
  return (uint64_t)(uint32_t)((uint32_t)a + (uint32_t)b);
}
__host__ __device__ __forceinline__ uint64_t dsum_sub(uint64_t a, uint64_t b) {
  return (uint64_t)(uint32_t)((uint32_t)a - (uint32_t)b);
}

// Inclusive prefix sums (mod 2^32) across the wave's lanes with data-parallel-primitive moves instead of
// ds_bpermute: four shifts inside each row of 16 lanes, then the totals of rows 0 / 2 into rows 1 / 3 and the total
// of the lower half into the upper.  Call with the whole wave active.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_or_zero(uint32_t v) {  // the moved value; 0 where no lane feeds this one
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xF, false);
}
__device__ __forceinline__ uint32_t row_scan_incl(uint32_t v) {  // within rows of 16 lanes
  v += dpp_or_zero<0x111, 0xF>(v);  // row_shr:1
  v += dpp_or_zero<0x112, 0xF>(v);  // row_shr:2
  v += dpp_or_zero<0x114, 0xF>(v);  // row_shr:4
  v += dpp_or_zero<0x118, 0xF>(v);  // row_shr:8
  return v;
}
__device__ __forceinline__ uint32_t wave_scan_incl(uint32_t v) {
  v = row_scan_incl(v);
  v += dpp_or_zero<0x142, 0xA>(v);  // row_bcast:15 into rows 1 and 3
  v += dpp_or_zero<0x143, 0xC>(v);  // row_bcast:31 into rows 2 and 3
  return v;
}

// The last x in [0, V) with offs[x] <= p, for ascending offsets with offs[0] <= p < offs[V]: the row of a CSR that holds
// entry p, rows without entries skipped.  A 64-way search by one wave (every lane probes, the ballot counts the probes at
// or below p): 19 bits of V take four rounds.  Call with the whole wave active; the result is the same in every lane.
__device__ __forceinline__ uint32_t wave_find_row(const uint32_t *__restrict__ offs, uint32_t V, uint32_t p) {
  const uint32_t lane = threadIdx.x & 63;
  uint32_t lo = 0, n = V;  // the answer lies in [lo, lo + n)
  while (n > 1) {
    const uint32_t step = (n + 63) >> 6;
    const uint64_t k = (uint64_t)(lane + 1) * step;  // (64 steps may pass 2^32 where V nearly fills 32 bits)
    const bool le = k < n && offs[lo + (uint32_t)k] <= p;  // (ascending: the yeses are a prefix)
    const uint32_t c = (uint32_t)__popcll(__ballot(le));
    lo += c * step;
    n = n - c * step < step ? n - c * step : step;
  }
  return lo;
}

// sums over the wave with the DPP scan: the total is the last lane's prefix.  Call with the whole wave active.
__device__ __forceinline__ uint32_t wave_total_u32(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_readlane((int)wave_scan_incl(v), 63);
}
__device__ __forceinline__ uint64_t wave_reduce_dsum(uint64_t v) { return (uint64_t)wave_total_u32((uint32_t)v); }
// a count below 2^50 per lane: two 32-bit totals (24 low bits, the rest)
__device__ __forceinline__ uint64_t wave_total_u50(uint64_t v) {
  const uint32_t lo = wave_total_u32((uint32_t)v & 0xFFFFFFu), hi = wave_total_u32((uint32_t)(v >> 24));
  return ((uint64_t)hi << 24) + lo;
}

__device__ __forceinline__ uint64_t wave_reduce_add_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Locate the frontier entry that owns flattened child position p.  s_foff holds foff[i0..i0+XT]
// (UINT64_MAX past the end).  Returns entry index and writes the position inside the entry.
template <typename OffT>
__device__ __forceinline__ uint64_t locate_entry(const uint64_t *s_foff, const OffT *__restrict__ foff,
                                                 uint64_t n_entries, uint64_t i0, uint64_t p, uint64_t *k) {
  uint32_t lo = 0, hi = XT + 1;  // first idx in [0, XT+1) with s_foff[idx] > p
  while (lo < hi) {
    uint32_t mid = (lo + hi) >> 1;
    if (s_foff[mid] <= p)
      lo = mid + 1;
    else
      hi = mid;
  }
  uint64_t idx = i0 + lo - 1;
  uint64_t start = s_foff[lo - 1];
  if (lo == XT + 1) {  // window exhausted by zero-degree entries: finish the search in global memory
    uint64_t glo = i0 + XT, ghi = n_entries;
    while (glo < ghi) {
      uint64_t mid = (glo + ghi) >> 1;
      if ((uint64_t)foff[mid] <= p)
        glo = mid + 1;
      else
        ghi = mid;
    }
    idx = glo - 1;
    start = (uint64_t)foff[idx];
  }
  *k = p - start;
  return idx;
}

template <typename OffT>
__device__ __forceinline__ void load_window(uint64_t *s_foff, const OffT *__restrict__ foff, uint64_t n_entries,
                                            uint64_t i0) {
  for (uint32_t t = threadIdx.x; t <= XT; t += XT) {
    uint64_t gi = i0 + t;
    s_foff[t] = gi <= n_entries ? (uint64_t)foff[gi] : UINT64_MAX;
  }
}

// ---- sets of (class, vertex) pairs and the per-level steps gg_reach.hip and gg_levels.hip share
constexpr unsigned long long REACH_EMPTY = ~0ull;  // no key: a vertex index is never INVALID_U32

struct Visited {
  uint32_t *bits = nullptr;           // bitmap form: bit class * V + vertex
  uint64_t V = 0;
  unsigned long long *slots = nullptr;  // hash form: cap slots of class << 32 | vertex
  uint64_t cap = 0;
};

// true for the one caller that put (c, v) into the set.  Each form reads first and only does the atomic if the entry
// may still be absent: on a mirrored graph most children are visited already.
__device__ __forceinline__ bool claim(const Visited &vs, uint32_t c, uint32_t v) {
  if (vs.bits) {
    const uint64_t b = (uint64_t)c * vs.V + v;
    const uint32_t mask = 1u << (b & 31);
    if (__atomic_load_n(&vs.bits[b >> 5], __ATOMIC_RELAXED) & mask) return false;
    return !(atomicOr(&vs.bits[b >> 5], mask) & mask);
  }
  const unsigned long long key = ((unsigned long long)c << 32) | v;
  uint64_t s = __umul64hi(fmix64(key), vs.cap);
  while (true) {
    unsigned long long old = __atomic_load_n(&vs.slots[s], __ATOMIC_RELAXED);
    if (old == REACH_EMPTY) old = atomicCAS(&vs.slots[s], REACH_EMPTY, key);
    if (old == REACH_EMPTY) return true;
    if (old == key) return false;
    s = s + 1 == vs.cap ? 0 : s + 1;
  }
}

inline dim3 stride_grid(gg_ctx *ctx, uint64_t n) {  // 256-thread workgroups for a kernel that strides over n items
  const uint64_t want = (n + 255) / 256, cap = (uint64_t)ctx->num_cus * 32;
  return dim3((unsigned)(want < cap ? (want ? want : 1) : cap));
}
inline int bits_for(uint64_t n) {  // bits of the largest value below n
  int b = 1;
  while (b < 64 && (1ull << b) < n) b++;
  return b;
}

struct PairLevel {  // the rows of one level, device arrays, ascending by (class, vertex index)
  uint32_t *cls, *vtx;
  uint64_t n;
};
// foff[0..n_parent]: the exclusive prefix of the out-degrees of fvtx (INVALID_U32: 0), from the pool; *M = their sum
// (one host round trip).  The caller frees *foff.  (gg_reach.hip)
int frontier_offsets(gg_ctx *ctx, const gg_csr *csr, const uint32_t *fvtx, uint64_t n_parent, uint64_t **foff, uint64_t *M);
// one thread per child of the frontier claims (class, child) in vs; the winners, appended through `count` (a device
// word) and sorted by (class, vertex index), are *out (n == 0: no array allocated)  (gg_reach.hip)
int expand_claim_sorted(gg_ctx *ctx, const gg_csr *csr, const uint32_t *fcls, const uint32_t *fvtx, const uint64_t *foff,
                        uint64_t n_parent, uint64_t M, const Visited &vs, uint32_t n_classes, uint32_t *count,
                        PairLevel *out);
// the levels' rows as the result's kept int64 columns (cols[0][0]: class, cols[0][1]: vertex id); synchronises
int emit_pair_levels(gg_ctx *ctx, const gg_csr *csr, const std::vector<PairLevel> &levels, gg_result *res);
// the two kept columns of rows[0] = the sum of level_rows rows each, allocated (gg_closure.hip, emit_pair_levels)
int alloc_level_columns(gg_ctx *ctx, gg_result *res);
// the bodies of the _levels / _fetch readers of the walk closure, the reach closure and the level sets, after their kind
// check: both columns of cols[0] and, if asked for, every row's level from level_rows
int level_rows_levels(const gg_result *res, uint64_t *rows_per_level, int capacity, int *n_levels);
int level_rows_fetch(const gg_result *res, uint64_t offset, uint32_t max_rows, int64_t *col0, int64_t *col1, int32_t *level,
                     uint32_t *n_out);

// ---- shortest paths off a finished BFS batch (gg_paths.hip; called by bfs_run in gg_bfs.hip)
constexpr int PATHS_TABLE = 3;  // the gg_result table that holds the path rows
struct PathsRequest {
  const uint32_t *pair_lane;    // host, n_pairs: the pair's source as an index into the batch's source list
  const int64_t *pair_dst_ids;  // host, n_pairs
  uint64_t n_pairs;
  bool want_edges;
  gg_result *res;
};
// dist: the batch's [V][64] distance cells of cell_bytes (1 or 2) each, on the device.  Fills rq.res; synchronises.
int paths_emit(gg_ctx *ctx, gg_csr *csr, const void *dist, size_t cell_bytes, const PathsRequest &rq);

// ---- all shortest paths and their number off a finished BFS batch (gg_all_paths.hip; called by bfs_run in gg_bfs.hip)
constexpr int AP_PAIRS_TABLE = 0, AP_ROWS_TABLE = 1;  // the gg_result tables of the reached pairs and of the path rows
struct AllPathsRequest {
  const int64_t *src_ids;       // host, n_src: the batch's sources (the seeds of the count)
  int n_src;
  const uint32_t *pair_lane;    // host, n_pairs: the pair's source as an index into the batch's source list
  const int64_t *pair_dst_ids;  // host, n_pairs
  uint64_t n_pairs;
  uint64_t path_limit;          // 0: none
  bool want_edges;
  bool materialise;
  gg_all_paths_stats *stats;    // nullable; its bfs member is left alone
  gg_result *res;               // nullable: totals only
};
// dist: as paths_emit; levels: the BFS levels that ran.  Fills rq.stats and rq.res; synchronises.
int all_paths_emit(gg_ctx *ctx, gg_csr *csr, const void *dist, size_t cell_bytes, uint32_t levels,
                   const AllPathsRequest &rq);
// gg_bfs64's dispatch (8-bit cells, 16-bit rerun) with the request handed to bfs_run (gg_bfs.hip)
int bfs64_all_paths_run(gg_ctx *ctx, const gg_csr *csr, const int64_t *src_ids, int n_src, int max_hops,
                        gg_bfs_stats *stats, const AllPathsRequest &rq);

// ---- the cheapest paths off a finished gg_cheapest64 batch (gg_cheapest.hip)
constexpr int CPP_PAIRS_TABLE = 0, CPP_ROWS_TABLE = 1;  // the gg_result tables of the reached pairs and of the path rows

}  // namespace gg
