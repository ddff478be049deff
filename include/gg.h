/* gg.h — C-ABI of the MI355X-native graph pattern-matching hot path ("gg" = GPU graph).
 *
 * This is the drop-in boundary between DuckDB-style host operators (C++, see
 * duckdb_pgq_amd/host/) and the hand-written HIP kernels for gfx950 (duckdb_pgq_amd/csrc/).
 * Plain pointers and sizes only: no C++ types, no torch types, no exceptions cross it.
 *
 * What each entry point replaces in the reference (cwida/duckdb-pgq.old, paths relative to
 * /root/reference; the reference has no C ABI at operator level — SURVEY.md §8b — so these are
 * the calls our PhysicalOperator subclasses make where the reference's operators call their
 * CPU data structures):
 *
 *   gg_vertices_append / gg_edges_append
 *        <- PhysicalHashJoin::Sink -> JoinHashTable::Build      src/execution/operator/join/physical_hash_join.cpp:128-154,
 *                                                               src/execution/join_hashtable.cpp:150-238
 *           (called concurrently from Sink threads, one call per <=1024-row DataChunk column set)
 *   gg_csr_build
 *        <- PhysicalHashJoin::Finalize -> JoinHashTable::Finalize/InsertHashes
 *                                                               physical_hash_join.cpp:165-185, join_hashtable.cpp:240-302
 *           (single-threaded finalize of the adjacency index keyed on the source vertex)
 *   gg_expand_khop / gg_result_fetch
 *        <- PhysicalHashJoin::Execute -> JoinHashTable::Probe + ScanStructure::NextInnerJoin (chain of k joins)
 *                                                               physical_hash_join.cpp:217-254, join_hashtable.cpp:304-476
 *           (fixed-length path expansion; fetch hands back <=1024-row slices = one DataChunk)
 *   gg_bfs64 / gg_bfs64_pairs / gg_bfs_sharded_* (one BFS over a vertex-partitioned graph, several GPUs)
 *        <- PhysicalRecursiveCTE::{Sink,GetData,ExecuteRecursivePipelines} + GroupedAggregateHashTable::FindOrCreateGroups
 *           + PhysicalHashAggregate (min(hopCount) GROUP BY start, friend)
 *                                                               src/execution/operator/set/physical_recursive_cte.cpp:48-139,
 *                                                               src/execution/aggregate_hashtable.cpp:367-504,
 *                                                               src/execution/operator/aggregate/physical_hash_aggregate.cpp:152-266
 *           (the friends/friends_shortest CTE pair of benchmark/ldbc/queries/bi-10-shortestpath.sql:8-31)
 *   gg_bfs64_paths / gg_bfs64_paths_rows / gg_bfs64_paths_fetch
 *        <- no relation of the reference: bi-10-shortestpath.sql:26-31 stops at min(hopCount).  With its operators a path
 *           is one more hash join of friends_shortest with knows per step under a min(rowid) aggregate
 *                                                               physical_hash_join.cpp:217-254, join_hashtable.cpp:304-476,
 *                                                               physical_hash_aggregate.cpp:152-266
 *   gg_bfs64_all_paths / gg_bfs64_all_paths_rows / gg_bfs64_all_paths_fetch_pairs / gg_bfs64_all_paths_fetch
 *        <- ALL SHORTEST and its count: PhysicalRecursiveCTE (UNION ALL) over friends_shortest joined with knows once per
 *           level, a hash aggregate above it for the count
 *                                                               physical_recursive_cte.cpp:60-139, join_hashtable.cpp:304-476,
 *                                                               physical_hash_aggregate.cpp:152-266
 *   gg_walk_endpoints
 *        <- PhysicalUnion + the hash-aggregate dedupe above it (friends UNION friends of friends)
 *                                                               src/execution/physical_plan/plan_distinct.cpp:12-78,
 *                                                               physical_hash_aggregate.cpp:152-266
 *   gg_vertices_from_edges
 *        <- the implicit vertex set of a join chain over an edge table alone (interactive-complex-3.sql:9-11)
 *   gg_result_filter_common_neighbour
 *        <- the six monitoredBy hash joins of benchmark/trainbenchmark/queries/connectedsegments.sql:1-25
 *   gg_result_filter_edge
 *        <- an edge condition between two columns of rows that are already joined: the last hash join of a chain carrying
 *           two conditions (k4.dst = k1.src), Probe + ScanStructure::NextInnerJoin        join_hashtable.cpp:304-476;
 *           NOT EXISTS (... knows WHERE k_person1id = C AND k_person2id = k2.k_person2id),
 *           ScanStructure::ScanKeyMatches + NextAntiJoin                                  join_hashtable.cpp:478-540
 *           (benchmark/ldbc/queries/interactive-complex-10.sql:19-24); EXISTS, NextSemiJoin   join_hashtable.cpp:522
 *           (interactive-complex-7.sql:5, interactive-short-7.sql:3)
 *   gg_result_extend_edge
 *        <- the next hash join of a chain over a DIFFERENT build table, its payload gathered by rowid: Probe +
 *           ScanStructure::NextInnerJoin + GatherResult                                   join_hashtable.cpp:304-476
 *           (knows -> message on k_person2id = m_creatorid, benchmark/ldbc/queries/interactive-complex-2.sql:2-7;
 *           knows -> message -> message_tag, interactive-complex-4.sql:2-8; interactive-complex-9.sql:13-15,
 *           interactive-complex-6.sql:14-17; a branch off a middle column, interactive-complex-5.sql:15)
 *   gg_result_group_by
 *        <- PhysicalHashAggregate above the last hash join of such a chain: GROUP BY one column of the joined rows
 *                                                               physical_hash_aggregate.cpp:152-266,
 *                                                               src/execution/aggregate_hashtable.cpp:367-504,
 *                                                               join_hashtable.cpp:442-476
 *           (count(*) GROUP BY tag over knows [-> knows] -> message -> message_tag, interactive-complex-4.sql:1-22,
 *           interactive-complex-6.sql:1-22; by forum, interactive-complex-5.sql; a score summed per person, bi-8.sql:41-53)
 *   gg_result_filter_value / gg_result_top_rows
 *        <- a comparison on a payload column of the joined rows, run inside the scan, and PhysicalTopN above the last hash
 *           join                                     src/execution/operator/order/physical_top_n.cpp:238-293, 421-454
 *           (m_creationdate < :date ... ORDER BY m_creationdate DESC, m_messageid ASC LIMIT 20,
 *           benchmark/ldbc/queries/interactive-complex-2.sql:5,8-9, interactive-complex-9.sql:16-18; a date range before the
 *           GROUP BY, interactive-complex-4.sql:9,18, interactive-complex-3.sql:20,27; k2.k_person2id <> :person,
 *           interactive-complex-9.sql:12)
 *   gg_result_distinct
 *        <- PhysicalHashAggregate without aggregates above a join chain (SELECT DISTINCT / UNION)
 *                                                               src/execution/physical_plan/plan_distinct.cpp:12-78,
 *                                                               physical_hash_aggregate.cpp:152-266
 *           (SELECT DISTINCT k2.k_person2id, benchmark/ldbc/queries/interactive-complex-10.sql:19-24; the friends UNION of
 *           interactive-complex-6.sql:3-12 before it is joined with message; SELECT DISTINCT p1.personid, p2.personid,
 *           bi-14.sql:30-102; count(DISTINCT m_messageid), interactive-complex-10.sql:2-9)
 *   gg_result_group_tuples / gg_tuple_groups_rows / gg_tuple_groups_fetch
 *        <- PhysicalHashAggregate above a join chain: GROUP BY several columns of the joined rows, raw cells as keys,
 *           count / sum / min / max                             physical_hash_aggregate.cpp:152-266
 *           (GROUP BY m.friendid, t.t_name, benchmark/ldbc/queries/bi-10-shortestpath.sql:74; min(hopCount) GROUP BY
 *           startPerson, friend, bi-10-shortestpath.sql:28-30; GROUP BY person1id, person2id, bi-14.sql:111;
 *           max(l_creationdate) GROUP BY l_personid, interactive-complex-7.sql:7-12)
 *   gg_csr_lookup
 *        <- JoinHashTable::Probe of plain keys                 join_hashtable.cpp:304-330
 *   gg_walk_closure / gg_walk_closure_levels / gg_walk_closure_fetch
 *        <- PhysicalRecursiveCTE over a UNION ALL arm that joins the CTE with one table (the join rebuilt per level)
 *                                                               src/execution/operator/set/physical_recursive_cte.cpp:60-139
 *           (the post_all / chain reply trees of benchmark/ldbc/queries/bi-9.sql, interactive-short-6.sql)
 *   gg_reach_closure / gg_reach_closure_levels / gg_reach_closure_fetch
 *        <- PhysicalRecursiveCTE over a UNION arm that joins the CTE with one table: every produced row probed against
 *           a hash table of the rows emitted so far     src/execution/operator/set/physical_recursive_cte.cpp:47-139
 *           (reachability over knows, extended_tags of benchmark/ldbc/queries/interactive-complex-12.sql)
 *   gg_level_sets / gg_level_sets_levels / gg_level_sets_fetch
 *        <- PhysicalRecursiveCTE over a UNION arm with a depth counter: rows deduplicated inside a level only
 *                                                               src/execution/operator/set/physical_recursive_cte.cpp:47-139
 *           (the friends CTE of benchmark/ldbc/queries/bi-10-shortestpath.sql:8-25 under any consumer)
 *   gg_triangles
 *        <- the chain of three hash joins whose last join carries two conditions (k2.dst = k3.src AND k3.dst = k1.src):
 *           PhysicalHashJoin::Execute -> JoinHashTable::Probe + ScanStructure::NextInnerJoin
 *                                                               physical_hash_join.cpp:217-254, join_hashtable.cpp:304-476
 *           ("Friend triangles", benchmark/ldbc/queries/bi-11.sql:22-33)
 *
 * Conventions
 *   - every int-returning function returns GG_OK (0) or a negative GG_ERR_*; the message is
 *     available from gg_last_error() (thread-local).  The C++ operators turn a non-zero status
 *     into a duckdb::IOException, mirroring how the reference reports operator errors.
 *   - all pointers are HOST memory unless the name ends in _dev; inputs are copied, outputs are
 *     written into caller-allocated arrays.
 *   - thread safety: gg_vertices_append / gg_edges_append (concurrent Sink calls), gg_result_rows /
 *     gg_result_fetch / gg_result_destroy (several pipeline threads drain one result into their own buffers)
 *     and gg_host_alloc / gg_host_free may be called concurrently on one gg_ctx; they use nothing but
 *     their own locks and thread-safe HIP calls.  Everything else on one gg_ctx is externally serialised
 *     (DuckDB calls Finalize single-threaded per operator; the source operators hold the graph's lock
 *     around expansion calls).
 *   - vertex ids are arbitrary int64 (LDBC person ids are sparse); the *dense index* of a vertex
 *     is its 0-based position in the vertex table as appended (= DuckDB rowid of the vertex row).
 *   - an edge whose src or dst id is not in the vertex table is dropped (inner-join semantics of
 *     `person p1, knows k, person p2 WHERE p1.id = k.src AND k.dst = p2.id`).
 *   - there is no CPU fallback: without a usable HIP device every compute call fails.
 */
#ifndef GG_H
#define GG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GG_OK 0
#define GG_ERR_INVALID_ARG (-1)
#define GG_ERR_HIP (-2)
#define GG_ERR_OOM (-3)
#define GG_ERR_DUPLICATE_VERTEX (-4)
#define GG_ERR_TOO_LARGE (-5) /* > 2^32-2 edge rows or distinct ids; a frontier LEVEL of >= 2^32 walks in an expansion that must
                               materialise it (k >= 4, or k = 3 from a source list with the frontier forms forced); one result
                               part of that many rows from the row-at-a-time kernels — refused, never wrapped */
#define GG_ERR_STATE (-6)
#define GG_ERR_NO_DEVICE (-7)

#define GG_MAX_HOPS 8    /* longest fixed-length pattern gg_expand_khop accepts */
#define GG_BFS_LANES 64  /* sources per bitset-BFS batch (one bit lane each) */
#define GG_CHUNK_ROWS 1024 /* STANDARD_VECTOR_SIZE, src/include/duckdb/common/vector_size.hpp:17 */

typedef struct gg_ctx gg_ctx;       /* device, stream, staging buffers; caller-owned */
typedef struct gg_csr gg_csr;       /* device-resident CSR adjacency index; caller-owned */
typedef struct gg_result gg_result; /* device-resident materialised path rows; caller-owned */

/* ---- library / context ------------------------------------------------------------------ */
const char *gg_version(void);
const char *gg_last_error(void);
int gg_device_count(int *out_count);
int gg_ctx_create(int device, gg_ctx **out);
void gg_ctx_destroy(gg_ctx *ctx);
/* Page-locked host memory for result slabs: gg_result_fetch into such a buffer runs at PCIe rate (into
 * pageable memory the runtime bounces through its own staging buffers, ~5 GB/s measured).  Freed buffers
 * are kept by the context and reused; gg_ctx_destroy releases them.  Thread-safe. */
int gg_host_alloc(gg_ctx *ctx, uint64_t bytes, void **out);
void gg_host_free(gg_ctx *ctx, void *ptr);

/* ---- staging: base-table columns -> HBM (Sink side) -------------------------------------- */
/* Append n vertex ids (vertex-table key column, in table order). */
int gg_vertices_append(gg_ctx *ctx, const int64_t *id, uint64_t n);
/* Append n edge rows.  rowid may be NULL (then the edge's 0-based append position is its rowid). */
int gg_edges_append(gg_ctx *ctx, const int64_t *src, const int64_t *dst, const int64_t *rowid, uint64_t n);
/* Block until every appended row is resident in HBM (bench: the timed region starts after this). */
int gg_staging_sync(gg_ctx *ctx);
int gg_staging_counts(gg_ctx *ctx, uint64_t *n_vertices, uint64_t *n_edges);
int gg_staging_clear(gg_ctx *ctx);

/* ---- CSR build (Finalize side) ------------------------------------------------------------ */
/* Whether later builds carry the edge rowid per CSR entry (default 1).  A MATCH that binds no edge
 * variable — e.g. count(*) or Person-KNOWS*1..2-Person returning persons — does not need it, exactly as
 * the reference's hash-join build side only carries the columns the query references; the build then
 * sorts 8 instead of 12 bytes per edge ("+8E if edge rowid kept").  With 0, gg_csr_export
 * reports -1 as rowid. */
int gg_ctx_set_edge_rowid(gg_ctx *ctx, int keep);
/* Densify ids (device hash table), histogram + prefix-scan + stable LSD radix scatter by source.
 * Within a CSR row, neighbours are in ascending edge-rowid (append) order: the build is
 * deterministic.  Staged columns stay resident, so the build can be repeated.
 * Fails with GG_ERR_DUPLICATE_VERTEX if the vertex key column is not unique.
 * Returns as soon as the build's outcome is known (duplicate ids, kept edges); the last kernels may still be
 * queued on the context's stream, behind which every later call on the context is ordered. */
int gg_csr_build(gg_ctx *ctx, gg_csr **out);
/* Multi-GPU sharding of the whole hot path with NO data-path collective: every rank stages the vertex
 * table and (at least) the edge rows with an endpoint it owns, and builds only the CSR rows of the vertices
 * it owns (owner = hash(vertex id) mod n_parts): forward rows of owned sources, reverse rows of owned
 * destinations.  Other edge rows are skipped before the id lookups, so staging the whole table works too.
 * gg_expand_khop(all sources, k_min..2, count) on a shard returns the walks whose MIDDLE vertex (1-hop
 * rows: destination) is owned; over all parts the counts add and the digests add mod 2^32.  gg_bfs_sharded_*
 * runs a BFS over the shards; other operations reject a shard (GG_ERR_STATE). */
int gg_csr_build_shard(gg_ctx *ctx, int part, int n_parts, gg_csr **out);
void gg_csr_destroy(gg_csr *csr);
/* Probe the CSR's id dictionary: dense_out[i] = dense index (vertex-table position) of ids[i], or
 * 0xFFFFFFFF if ids[i] is not a vertex — what probing the build side's hash table with n keys does in the
 * reference (JoinHashTable::Probe, src/execution/join_hashtable.cpp:304-330). */
int gg_csr_lookup(gg_ctx *ctx, const gg_csr *csr, const int64_t *ids, uint64_t n, uint32_t *dense_out);
int gg_csr_info(const gg_csr *csr, uint64_t *n_vertices, uint64_t *n_edges_kept, uint64_t *n_edges_dropped);
/* Probe of a batch of keys against the index keyed on the edge rows' source column, with the matches' rowids: for the
 * n keys (host memory; a key that is no vertex matches nothing) table 1 of *out_result gets one row (i, rowid) per
 * edge row whose source equals keys[i] — i the position in `keys` — in ascending i, a key's rows in rowid order; fetch
 * with gg_result_rows(res, 1, &m) / gg_result_fetch(res, 1, offset, max, cols[2], &got).  This is the device side of a
 * generic single-key inner hash join: JoinHashTable::Probe + ScanStructure::NextInnerJoin for one probe chunk
 * (src/execution/join_hashtable.cpp:304-476); the host operator (PhysicalGGKeyJoin) slices the probe chunk by i and
 * fetches the build side's columns by rowid.  The CSR must have been built with edge rowids kept.  A batch of 2^32
 * matches or more returns GG_ERR_TOO_LARGE: probe it in smaller batches. */
int gg_join_probe(gg_ctx *ctx, const gg_csr *csr, const int64_t *keys, uint64_t n, uint64_t *n_matches,
                  gg_result **out_result);
/* Parity export.  off: V+1 entries; nbr: E_kept dense neighbour indices; eid: E_kept edge rowids
 * (may be NULL); vid: V vertex ids by dense index (may be NULL). */
int gg_csr_export(const gg_csr *csr, int64_t *off, int64_t *nbr, int64_t *eid, int64_t *vid);

/* ---- fixed-length path expansion (k-hop MATCH) -------------------------------------------- */
typedef struct gg_khop_stats {
  uint64_t rows[GG_MAX_HOPS + 1];   /* rows[h] = number of h-hop walks emitted (h in k_min..k_max) */
  uint64_t digest[GG_MAX_HOPS + 1]; /* digest[h] = sum over those rows of the LOW 32 BITS of the gg row hash (DESIGN.md "Row digest"), mod 2^32, in a u64 field */
  uint64_t traversed_edges;         /* TE = adjacency entries read over all hops */
  uint64_t frontier_entries;        /* path prefixes whose adjacency list was expanded */
} gg_khop_stats;

/* All walks  s -> v1 -> ... -> vh  with h in [k_min, k_max] (1 <= k_min <= k_max <= GG_MAX_HOPS),
 * s drawn from the source list (with multiplicity).  src_ids == NULL: every vertex is a source.
 * Source ids absent from the vertex table contribute nothing.
 * materialise == 0: count + digest only (out_result may be NULL).
 * materialise != 0: rows are written to HBM as int64 vertex ids, one table per length h with h+1
 *                   columns, and handed back through *out_result. */
int gg_expand_khop(gg_ctx *ctx, const gg_csr *csr, const int64_t *src_ids, uint64_t n_src, int k_min, int k_max,
                   int materialise, gg_khop_stats *stats, gg_result **out_result);
/* Only the NUMBER of h-hop walks for h in [k_min, k_max] (rows[h]; other entries 0), computed from degrees: with
 * w_0(v) = how often v is a source and w_h(v) = sum over in-neighbours u of w_{h-1}(u), rows_h = sum_v w_{h-1}(v) *
 * outdeg(v) — from every vertex two passes over offset arrays for h <= 2, one pull over the reverse rows per further
 * hop.  This is what `SELECT count(*)` over the join chain asks for: the reference's aggregate above the hash joins
 * consumes chunk cardinalities, never the rows (src/execution/operator/aggregate/physical_simple_aggregate.cpp, fed by
 * ScanStructure::NextInnerJoin, src/execution/join_hashtable.cpp:442-476).  Equal to gg_khop_stats.rows of
 * gg_expand_khop with the same arguments (also on a shard: the walks whose middle vertex is owned); no digest. */
int gg_khop_count(gg_ctx *ctx, const gg_csr *csr, const int64_t *src_ids, uint64_t n_src, int k_min, int k_max,
                  uint64_t *rows /* GG_MAX_HOPS + 1 entries */);
/* Same, sources = dense vertex indices [src_lo, src_hi) — the multi-GPU sharding entry point
 * (each rank takes one contiguous range; no data-path collective). */
int gg_expand_khop_range(gg_ctx *ctx, const gg_csr *csr, uint64_t src_lo, uint64_t src_hi, int k_min, int k_max,
                         int materialise, gg_khop_stats *stats, gg_result **out_result);
/* Split [0,V) into n_parts contiguous source ranges of near-equal 2-hop work (sum over u of
 * sum over v in adj(u) of (1+deg(v))).  bounds: n_parts+1 entries. */
int gg_khop_partition(gg_ctx *ctx, const gg_csr *csr, int n_parts, uint64_t *bounds);

/* 2-hop walks (and, if k_min == 1, the 1-hop rows) of ALL sources whose MIDDLE vertex (1-hop rows:
 * destination) has dense index in [mid_lo, mid_hi).  k_max must be 2.  Disjoint ranges partition the
 * result of gg_expand_khop(all sources, k_min..2): counts add, digests add mod 2^32.  This is the
 * multi-GPU sharding entry point of the 2-hop product kernel (reads each CSR row once per shard). */
int gg_expand_khop_mid(gg_ctx *ctx, gg_csr *csr, uint64_t mid_lo, uint64_t mid_hi, int k_min, int k_max,
                       gg_khop_stats *stats);
/* The same rows MATERIALISED (int64 id columns in HBM, fetched with gg_result_fetch): the 2-hop rows u -> x -> w of
 * all sources with x in [mid_lo, mid_hi) and, if k_min == 1, the 1-hop rows u -> x into the range.  Disjoint ranges
 * partition the materialised result of gg_expand_khop(all sources, k_min..2) — how a result larger than device
 * memory (SF100: 12.8 G rows, 306 GB) is produced part by part, each part through the product kernel.  On a shard
 * (gg_csr_build_shard) the rows are those whose middle vertex is owned AND in the range: N ranks that each materialise
 * [0, V) of their shard — in gg_khop_partition_mid parts if need be — produce the whole result once, no exchange. */
int gg_expand_khop_mid_result(gg_ctx *ctx, gg_csr *csr, uint64_t mid_lo, uint64_t mid_hi, int k_min,
                              gg_khop_stats *stats /* nullable: no counts + digests in front of the rows */,
                              gg_result **out_result);
/* gg_expand_khop(all sources, k_min..2, count) with the result LEFT ON THE DEVICE and no host synchronisation: six
 * uint64 words (rows of 1-hop walks, rows of 2-hop walks, digest 1, digest 2, traversed edges, frontier entries; the
 * digests 32-bit sums in the low half) in a buffer owned by the context (*stats_dev; overwritten by the next such call).
 * For the ranks of a sharded query (gg_csr_build_shard): each rank's words are added by ONE collective on the device
 * (RCCL SUM through torch.distributed on a view of that memory — the library owns no communicator) and cross to the host
 * once, instead of host -> device -> all-reduce -> host per rank.  Order the collective's stream behind the library's
 * with gg_stream_wait. */
int gg_expand_khop_dev(gg_ctx *ctx, gg_csr *csr, int k_min, void **stats_dev);
/* Stream ordering without the host: direction 0 — everything queued on `other_stream` (a hipStream_t, e.g. torch's
 * current stream) from now on waits for everything queued on the context's stream so far; direction 1 — the reverse. */
int gg_stream_wait(gg_ctx *ctx, void *other_stream, int direction);
/* Split [0,V) into n_parts contiguous middle-vertex ranges of near-equal product work. */
int gg_khop_partition_mid(gg_ctx *ctx, gg_csr *csr, int n_parts, uint64_t *bounds);

/* A result answers the calls of its own kind only.  The five older kinds — fixed-length walk tables, walk closure, reach
 * closure, level sets, paths — refuse one another with GG_ERR_INVALID_ARG; the kinds that state a refusal contract of their
 * own (grouped aggregates, pair counts, components, all shortest paths, cheapest costs and paths, aggregates per key
 * tuple) are refused by every other call, and their calls
 * refuse every other result, with GG_ERR_STATE.  A fixed-length walk table (a result of gg_expand_khop*, gg_bfs64_pairs*,
 * gg_walk_endpoints, gg_join_probe, gg_triangles*, the filters or gg_result_extend_edge) answers gg_result_rows,
 * gg_result_fetch, gg_result_fetch_edges and gg_result_digest for the levels it holds; a closure, level-set or paths result
 * is GG_ERR_INVALID_ARG to them for every `hops`. */
int gg_result_rows(const gg_result *res, int hops, uint64_t *n_rows);
/* Copy rows [offset, offset+max_rows) of the h-hop table into cols[0..h] (host arrays of >= max_rows).  Destinations
 * in page-locked memory (gg_host_alloc) are filled over the context's fetch lanes (concurrent callers
 * overlap their copies: ~44 GB/s in 2 MB pieces); any other destination over the library's stream. */
int gg_result_fetch(const gg_result *res, int hops, uint64_t offset, uint32_t max_rows, int64_t *const *cols,
                    uint32_t *n_out);
/* k-hop walks with the ROWID of every edge taken (src_ids NULL: from every vertex): table k of the result has the id
 * columns v0..vk (gg_result_fetch) and the edge columns e1..ek (gg_result_fetch_edges: the rowid the Sink passed with
 * the edge row, or its append position if it passed none).  This is what a late join with the edge table's payload
 * columns needs (the reference gathers build-side columns per match, src/execution/join_hashtable.cpp:466-473).  The
 * CSR must have been built with edge rowids kept (gg_ctx_set_edge_rowid(ctx, 1), the default).  stats: rows[k] only. */
int gg_expand_khop_edges(gg_ctx *ctx, const gg_csr *csr, const int64_t *src_ids, uint64_t n_src, int k,
                         gg_khop_stats *stats, gg_result **out_result);
/* Copy rows [offset, offset+max_rows) of the edge columns e1..e_hops into ecols[0..hops-1]. */
int gg_result_fetch_edges(const gg_result *res, int hops, uint64_t offset, uint32_t max_rows, int64_t *const *ecols,
                          uint32_t *n_out);
/* Checksum of the `hops`-hop rows (k_min <= hops <= k_max of the result, so 0 — a one-column table of
 * gg_result_distinct, whose row hash is the dense index itself — up to GG_MAX_HOPS) as they stand in HBM:
 * every id of every row is mapped back to its dense index and the rows' hashes are summed exactly as
 * gg_khop_stats.digest[hops] sums them, so a materialising expansion can be compared with the count-only expansion (and
 * with the oracle) over ALL its rows without fetching them.  Fails with GG_ERR_STATE if a row holds an id that is not a
 * vertex of `csr`. */
int gg_result_digest(gg_ctx *ctx, const gg_csr *csr, const gg_result *res, int hops, uint64_t *n_rows,
                     uint64_t *digest);
void gg_result_destroy(gg_result *res);
/* gg_expand_khop with the result left on the device for further operators (same arguments; only the
 * handle is returned, nothing is copied to the host). */
int gg_expand_khop_result(gg_ctx *ctx, const gg_csr *csr, const int64_t *src_ids, uint64_t n_src, int k_min, int k_max,
                          gg_khop_stats *stats, gg_result **out_result);
/* Same-neighbour filter (Train Benchmark ConnectedSegments: six segments monitored by one sensor).
 * Input: the `hops`-hop table of `res` (columns v0..vh).  `filter` is a CSR over a vertex table that
 * contains the path vertices' ids and the filter targets (e.g. TrackElements and Sensors; edges =
 * monitoredBy).  Output table (fetch it with hops+1): one row (w, v0..vh) for every filter neighbour w
 * common to ALL of v0..vh, with the multiplicity the chained joins would give. */
int gg_result_filter_common_neighbour(gg_ctx *ctx, const gg_result *res, int hops, const gg_csr *filter,
                                      gg_result **out);
/* Edge condition between two columns of a materialised walk table, as an inner, semi or anti join.
 * What it replaces in the reference: the last hash join of a chain when it carries two conditions — `k4.dst = k1.src`
 * closes a 4-walk, and likewise any longer one (PhysicalHashJoin::Execute -> JoinHashTable::Probe +
 * ScanStructure::NextInnerJoin, src/execution/join_hashtable.cpp:304-476); `NOT EXISTS (SELECT * FROM knows WHERE
 * k_person1id = C AND k_person2id = k2.k_person2id)`, "friends of friends who are not friends"
 * (benchmark/ldbc/queries/interactive-complex-10.sql:19-24: ScanStructure::ScanKeyMatches + NextAntiJoin,
 * join_hashtable.cpp:478-540); and `EXISTS (SELECT 1 FROM knows WHERE k_person1id = C AND k_person2id = p_personid)`
 * (interactive-complex-7.sql:5, interactive-short-7.sql:3: NextSemiJoin, join_hashtable.cpp:522).
 * Input: the `hops`-hop table of `res` with its id columns v0..v_hops — from gg_expand_khop_result,
 * gg_expand_khop(materialise), gg_expand_khop_mid_result, gg_triangles(materialise) or an earlier call of this function.
 * `csr` is the graph the condition is asked of: usually the one the walks came from, but any whole CSR of the same context
 * is accepted (walks over one edge table, condition over another).  The cells are looked up in csr's id dictionary exactly
 * as gg_csr_lookup does.  For a row, m = the number of kept edge rows of csr with source v_from_col and destination
 * v_to_col; m = 0 if either id is no vertex of csr.  from_col == to_col is allowed: a self-loop test.
 *   GG_EDGE_INNER: m copies of the row (the join's multiplicity); GG_EDGE_SEMI: the row once if m > 0; GG_EDGE_ANTI: the
 *   row once if m == 0 — so a row with an id unknown to csr survives anti and nothing else, as NOT EXISTS demands.
 * Output: table `hops` of *out_result (k_min = k_max = hops) with the same hops + 1 int64 id columns and no edge columns,
 * for gg_result_rows / gg_result_fetch / gg_result_digest, this function again and gg_result_filter_common_neighbour.
 * Row order is the input's: surviving rows keep their relative order and the m copies of a row are consecutive.  The rows
 * are placed by count, scan, write — no atomics-ordered append — so placement is identical on every run.
 * materialise == 0: only `stats` is filled (out_result may be NULL); 64-bit counters, no size limit.  stats may be NULL when
 * materialising.  Chords are two calls in a row; closed walks of k edges from a source list are the (k - 1)-hop table
 * filtered with from_col = k - 1, to_col = 0, inner; for hops = 2, from 2, to 0, inner over all sources the rows are
 * gg_triangles(order = 0)'s.  Whole-graph triangles stay gg_triangles' business: it never materialises the wedges.
 * Errors: NULL ctx / res / csr, objects of another context, hops outside the result's k_min..k_max, a column outside
 * 0..hops, a mode outside {0, 1, 2}, materialise != 0 with NULL out_result: GG_ERR_INVALID_ARG.  A shard CSR, or a result
 * without fixed-length tables (closures, level sets, paths): GG_ERR_STATE.  2^32 output rows or more when materialising:
 * GG_ERR_TOO_LARGE (count them, or filter a smaller table).  After every error the context stays usable.
 * The first call on a CSR sorts a copy of its reverse rows by source (gg_bfs64_paths' and gg_triangles' copy: 4 bytes per
 * edge, kept with the CSR) and, if the build did not need the 16-byte id table, fills it. */
#define GG_EDGE_INNER 0   /* one output row per matching edge row (join multiplicity) */
#define GG_EDGE_SEMI  1   /* the row once if at least one edge row matches (EXISTS) */
#define GG_EDGE_ANTI  2   /* the row once if no edge row matches (NOT EXISTS) */
typedef struct gg_edge_filter_stats {
  uint64_t rows_in;   /* rows of the input table */
  uint64_t rows_out;  /* rows that pass, with multiplicity in inner mode */
  uint64_t matches;   /* sum over input rows of the number of edge rows v_from -> v_to (= rows_out in inner mode) */
} gg_edge_filter_stats;
int gg_result_filter_edge(gg_ctx *ctx, const gg_result *res, int hops, const gg_csr *csr, int from_col, int to_col,
                          int mode, int materialise, gg_edge_filter_stats *stats, gg_result **out_result);
/* One more hop over a second edge table: every row of a materialised walk table joined with the edge rows of `csr` whose
 * source is the row's cell in from_col.
 * What it replaces in the reference: the next hash join of a chain when its build table is a different one — `knows k,
 * message m WHERE m.m_creatorid = k.k_person2id` (benchmark/ldbc/queries/interactive-complex-2.sql:2-7), knows -> message ->
 * message_tag (interactive-complex-4.sql:2-8), friends and friends of friends, their messages, their tags
 * (interactive-complex-9.sql:13-15, interactive-complex-6.sql:14-17), forum_person joined on a middle column
 * (interactive-complex-5.sql:15) — PhysicalHashJoin::Execute -> JoinHashTable::Probe + ScanStructure::NextInnerJoin, with
 * the payload columns (m_creationdate, m_content) gathered by row in ScanStructure::GatherResult
 * (src/execution/join_hashtable.cpp:304-476).  Without it such a plan leaves the device after the last knows hop.
 * Input: the `hops`-hop table of `res` with its id columns v0..v_hops — whatever gg_result_filter_edge accepts, or an earlier
 * result of this function, so patterns chain and branch; from_col is any column 0..hops.  `csr` is any whole CSR of the same
 * context, usually over another edge table; the cell is looked up in its id dictionary exactly as gg_csr_lookup does, and an
 * id that is no vertex of csr matches nothing.
 * Output: table hops + 1 of *out_result (k_min = k_max = hops + 1): the input's hops + 1 columns and a new last column w, one
 * row per kept edge row v_from_col -> w of csr.  Input rows keep their order; the copies of one input row are consecutive
 * and in CSR order (the append order of the edge rows, the order gg_csr_export shows).  Rows are placed by count, scan,
 * write — no atomics-ordered append — so they are identical on every run and for every gg_debug_extend tile.
 * want_edges != 0: the output carries edge columns e1..e_{hops+1} for gg_result_fetch_edges; e_{hops+1} is the rowid of the
 * joined edge row (the rowid the Sink passed, or the append position), e1..e_hops are the input's edge columns if it has
 * them and -1 otherwise.  It needs a csr built with rowids (GG_ERR_STATE otherwise, as gg_expand_khop_edges).
 * materialise == 0: only `stats` is filled, from degrees: 64-bit counters, no size limit, nothing kept per row; out_result
 * may be NULL.  stats may be NULL when materialising.
 * The result answers gg_result_rows, gg_result_fetch, gg_result_fetch_edges, gg_result_digest, gg_result_filter_edge,
 * gg_result_filter_common_neighbour and this function again.
 * Errors: NULL ctx / res / csr, objects of another context, hops outside the result's k_min..k_max, hops + 1 > GG_MAX_HOPS,
 * from_col outside 0..hops, materialise != 0 with NULL out_result: GG_ERR_INVALID_ARG.  A shard CSR, or a result without
 * fixed-length tables: GG_ERR_STATE.  2^32 output rows or more when materialising: GG_ERR_TOO_LARGE.  After every error the
 * context stays usable.  An empty input table, a csr without edge rows and an input of which no row matches give GG_OK and an
 * empty table.  If the build did not need the 16-byte id table, the first call on a CSR fills it. */
typedef struct gg_extend_stats {
  uint64_t rows_in;      /* rows of the input table */
  uint64_t rows_out;     /* sum over input rows of the kept edge rows of csr whose source is v_from_col */
  uint64_t rows_matched; /* input rows with at least one such edge row */
} gg_extend_stats;
int gg_result_extend_edge(gg_ctx *ctx, const gg_result *res, int hops, const gg_csr *csr, int from_col, int want_edges,
                          int materialise, gg_extend_stats *stats, gg_result **out_result);
/* GROUP BY one column of a materialised walk table: count(*) and sum(weight) per key, left on the device as an aggregate
 * result.
 * What it replaces in the reference: PhysicalHashAggregate (src/execution/operator/aggregate/physical_hash_aggregate.cpp:
 * 152-266, GroupedAggregateHashTable::FindOrCreateGroups, src/execution/aggregate_hashtable.cpp:367-504) fed by the last
 * hash join's ScanStructure::NextInnerJoin (src/execution/join_hashtable.cpp:442-476) — the end of
 * benchmark/ldbc/queries/interactive-complex-4.sql:1-22 and interactive-complex-6.sql:1-22 (knows [-> knows] -> message ->
 * message_tag under count(*) GROUP BY tag ORDER BY 2 DESC, name LIMIT 10), of interactive-complex-5.sql (by forum) and of
 * bi-8.sql:41-53 (a score summed per person above a mixed chain).  gg_khop_aggregate groups the walks of ONE CSR by their
 * first or last vertex and never sees a table; this groups whatever table the expansion, the filters and
 * gg_result_extend_edge left in HBM, so expand -> filter -> extend -> group -> gg_khop_aggregate_top runs without a row
 * leaving the device.
 * Input: the `hops`-hop table of `res` with its id columns v0..v_hops — whatever gg_result_extend_edge accepts, its own
 * output and the filters' included; edge columns are ignored.  Tables of 2^32 rows or more are accepted: every counter is
 * 64-bit and the kernels stride.
 * Key: the cell of key_col is looked up in key_csr's id dictionary exactly as gg_csr_lookup does; a row whose key is no
 * vertex of key_csr forms no group (the inner join with the key's table) and shows as rows_in - rows_grouped.
 * Aggregates per group: walks = the number of its rows, exact; total = the sum over its rows of weights[dense index in
 * weight_csr (NULL: key_csr) of the cell of weight_col], a weight cell that is no vertex of weight_csr weighing 0 (the host
 * operators' NULL convention), as a 128-bit two's-complement integer wrapping mod 2^128 like gg_khop_aggregate's.
 * weight_col == -1 (then weights must be NULL): total = walks and no sum is formed.  weights: V(weight_csr) int64 in
 * vertex-table order, host memory.
 * Output: an aggregate result of the single level `hops` (k_min = k_max = hops), one row (vertex id, walks, total lo, total
 * hi) per key that occurs, ascending by dense index in key_csr, placed by count, scan, write.  It answers
 * gg_khop_aggregate_rows / gg_khop_aggregate_fetch / gg_khop_aggregate_top (with csr = key_csr the bias is per key) and is
 * refused by every other reader, this function included, with GG_ERR_STATE.  The rows are identical on every run, on both
 * routes and under every testing knob: the sums are integer additions mod 2^64 and mod 2^128.
 * Two routes, chosen per call (stats->route): a workgroup-private table in LDS when key_csr's vertices fit it, flushed with
 * one global atomic per non-zero cell and workgroup; global cells otherwise.  On both, lanes of a wavefront that hold the
 * same key in adjacent rows are combined first, so a hub key costs one atomic per wavefront.
 * stats (nullable) and out_result (NULL: stats only) as gg_khop_aggregate's; one host synchronisation per call.
 * Errors: NULL ctx / res / key_csr, objects of another context, hops outside the result's k_min..k_max, key_col outside
 * 0..hops, weight_col outside -1..hops, weights NULL with weight_col >= 0 or non-NULL with weight_col == -1, stats and
 * out_result both NULL: GG_ERR_INVALID_ARG.  A shard CSR in either role, or a result without fixed-length tables:
 * GG_ERR_STATE.  Per-key state that does not fit: GG_ERR_OOM.  After every error the context stays usable.  An empty input
 * table, or a key_csr without vertices, gives GG_OK and an empty level.  If the build did not need the 16-byte id table, the
 * first call on a CSR fills it. */
typedef struct gg_group_stats {
  uint64_t rows_in;       /* rows of the input table */
  uint64_t rows_grouped;  /* of those, rows whose key cell is a vertex of key_csr (= the sum of the groups' walks) */
  uint64_t groups;        /* rows of the output */
  uint32_t route;         /* 0: nothing to do (no input rows / V == 0), 1: workgroup-private LDS table, 2: global cells */
} gg_group_stats;
int gg_result_group_by(gg_ctx *ctx, const gg_result *res, int hops, int key_col, const gg_csr *key_csr,
                       int weight_col /* -1: none */, const gg_csr *weight_csr /* NULL: key_csr */,
                       const int64_t *weights /* V(weight_csr) entries, host; NULL iff weight_col == -1 */,
                       gg_group_stats *stats /* nullable */, gg_result **out_result /* NULL: stats only */);
/* A value predicate on one column of a materialised walk table, and (gg_result_top_rows below) the best n rows by that
 * value.
 * What it replaces in the reference: a comparison on a payload column of the joined rows, evaluated inside the scan of the
 * payload's table below the last hash join — `m_creationdate < :date` (benchmark/ldbc/queries/interactive-complex-2.sql:5,
 * interactive-complex-9.sql:16), the half-open date range before the GROUP BY (interactive-complex-4.sql:9,18,
 * interactive-complex-3.sql:20,27) and `k2.k_person2id <> :person` (interactive-complex-9.sql:12).  Without it the only way
 * to apply one to the rows gg_result_extend_edge left in HBM is to drain them.
 * The value of a row (shared with gg_result_top_rows): `values` is V(value_csr) int64 in vertex-table order, host memory, as
 * gg_result_group_by's weights; `valid` (nullable) holds ceil(V / 64) uint64 words, bit i of word i / 64 saying that vertex i
 * has a value, NULL: every vertex has one.  The cell of value_col (0..hops) is looked up in value_csr's id dictionary exactly
 * as gg_csr_lookup does; the row has the value x = values[d] iff the cell is a vertex d of value_csr and d's valid bit is
 * set.  A row without a value behaves as SQL's NULL under a comparison: it passes no predicate in either mode and is never a
 * candidate of the top.  The message of an extended row is its last column and a vertex of the extension's CSR, so
 * m_creationdate per message is such a column; a person's property is one over the walk CSR.  Values keyed by edge rowid
 * (k_creationdate) are out of scope here (gg_edge_weights keys one by edge rowid, for gg_cheapest64 alone), and so is a device-resident value column shared between calls: each call uploads its
 * 8 V bytes (and V / 8 of valid), as gg_result_group_by does.
 * Predicate: GG_VALUE_IN keeps a row iff it has a value x and lo <= x <= hi (signed); GG_VALUE_NOT_IN iff it has a value x
 * and (x < lo or x > hi).  lo > hi: IN keeps nothing, NOT_IN every valued row.  `<` and `>=` are bounds +- 1 on the caller's
 * side, `<>` is NOT_IN with lo == hi.
 * Input: the `hops`-hop table of `res` — whatever gg_result_extend_edge accepts, its own output, the filters' and
 * gg_result_top_rows' included.  Tables of 2^32 rows or more are accepted when counting.
 * Output: table `hops` of *out_result (k_min = k_max = hops) with the same hops + 1 id columns and, unlike
 * gg_result_filter_edge, the input's edge columns e1..e_hops when it has them (the rowid of an extension survives the
 * filter); a gg_triangles_edges table loses its triangle edge columns, as under every filter.  Surviving rows keep the
 * input's order.  Placement is count, scan, write — no atomics-ordered append — so the rows are identical on every run and
 * under gg_debug_max_grid_tiles.  The result answers every reader of a walk table: gg_result_rows, gg_result_fetch,
 * gg_result_fetch_edges, gg_result_digest, both filters, gg_result_extend_edge, gg_result_group_by, this call and
 * gg_result_top_rows.
 * materialise == 0: only `stats` is filled (out_result may be NULL); 64-bit counters, no size limit, one host
 * synchronisation.  stats may be NULL when materialising, which synchronises twice (the total, the rows).
 * Errors: NULL ctx / res / value_csr / values, objects of another context, hops outside the result's k_min..k_max, value_col
 * outside 0..hops, a mode outside {0, 1}, materialise != 0 with NULL out_result: GG_ERR_INVALID_ARG.  A shard CSR, or a
 * result without fixed-length tables (gg_result's kinds, above): GG_ERR_STATE.  2^32 output rows or more when materialising:
 * GG_ERR_TOO_LARGE.  After every error the context stays usable.  An empty input table, a value_csr without vertices and a
 * predicate no row passes give GG_OK and an empty table.  If the build did not need the 16-byte id table, the first call on
 * a CSR fills it. */
#define GG_VALUE_IN     0  /* keep a row iff it has a value x and lo <= x <= hi (signed) */
#define GG_VALUE_NOT_IN 1  /* keep a row iff it has a value x and (x < lo or x > hi) */
typedef struct gg_value_filter_stats {
  uint64_t rows_in;     /* rows of the input table */
  uint64_t rows_valued; /* of those, rows that have a value */
  uint64_t rows_out;    /* rows that pass the predicate */
} gg_value_filter_stats;
int gg_result_filter_value(gg_ctx *ctx, const gg_result *res, int hops, int value_col, const gg_csr *value_csr,
                           const int64_t *values, const uint64_t *valid /* nullable */, int64_t lo, int64_t hi,
                           int mode, int materialise, gg_value_filter_stats *stats, gg_result **out_result);
/* The best n rows of a materialised walk table by the value of a row, among the rows gg_result_filter_value would keep:
 * `WHERE value BETWEEN lo AND hi ORDER BY value [DESC], id LIMIT n` in one upload and one pass over the cells.
 * What it replaces in the reference: PhysicalTopN (src/execution/operator/order/physical_top_n.cpp:238-293 heap sink /
 * reduce, :421-454 Sink / Combine) above the last hash join, with the scan's filter below it — the tail `ORDER BY
 * m_creationdate DESC, m_messageid ASC LIMIT 20` of benchmark/ldbc/queries/interactive-complex-2.sql:8-9 and
 * interactive-complex-9.sql:17-18.
 * Input, the value of a row, lo / hi / mode: as gg_result_filter_value; lo = INT64_MIN, hi = INT64_MAX, GG_VALUE_IN means
 * every valued row.  The candidates are the rows that filter would keep.
 * Order: row a comes before row b iff x(a) is better than x(b) — greater if descending != 0, else smaller, signed; or the
 * values are equal and a's cell in tie_col is the smaller signed int64 (in both directions: ORDER BY value [DESC], id); or
 * those are equal too, or tie_col == -1, and a is the earlier input row.  Walk tables hold duplicate rows and one message is
 * reached over many walks, so (value, tie id) is not unique; the row number as the last key word makes the key unique, the
 * n-th key exist and the output fully determined.
 * Output: table `hops` of *out_result (k_min = k_max = hops) with exactly min(n, candidates) rows in rank order: the id
 * columns gathered, and the edge columns if the input has them (a gg_triangles_edges table loses its own).  It is an
 * ordinary walk table, answered by every reader gg_result_filter_value's is, so it can be extended again (to fetch the
 * person).  n == 0 gives an empty table, n >= candidates every candidate, ordered.  LIMIT n OFFSET o is n + o here and a
 * fetch from offset o.
 * One host synchronisation per call: the number of candidates stays on the device, the rank selected there is min(n,
 * candidates), and the buffers and the sort route (stats->sort_route) follow min(n, rows_in), which the host knows.
 * stats->select_passes: the digit passes that ran — bytes that are zero in every key (the row number's above
 * bits_for(rows), the tie word without a tie column) get none.
 * Errors: as gg_result_filter_value, and NULL out_result or tie_col outside -1..hops: GG_ERR_INVALID_ARG.  An input table
 * of 2^32 rows or more (which min(n, candidates) >= 2^32 needs): GG_ERR_TOO_LARGE — row numbers are 32-bit here; filter
 * first.  An empty input table, a value_csr without vertices, n == 0 and no candidate give GG_OK and an empty table. */
typedef struct gg_value_top_stats {
  uint64_t rows_in;       /* rows of the input table */
  uint64_t rows_valued;   /* of those, rows that have a value */
  uint64_t candidates;    /* rows that pass the predicate */
  uint64_t rows_out;      /* min(n, candidates) */
  uint32_t select_passes; /* digit passes the selection ran (as gg_top_stats) */
  uint32_t sort_route;    /* 0: none needed (fewer than two rows), 1: one workgroup in LDS, 2: global passes */
} gg_value_top_stats;
int gg_result_top_rows(gg_ctx *ctx, const gg_result *res, int hops, int value_col, const gg_csr *value_csr,
                       const int64_t *values, const uint64_t *valid /* nullable */, int64_t lo, int64_t hi, int mode,
                       int descending, int tie_col /* -1: none */, uint64_t n, gg_value_top_stats *stats /* nullable */,
                       gg_result **out_result);
/* SELECT DISTINCT over chosen columns of a materialised walk table: projection plus DISTINCT, on the device.
 * What it replaces in the reference: the hash aggregate without aggregates that SELECT DISTINCT and UNION plan
 * (src/execution/physical_plan/plan_distinct.cpp:12-78) above a join chain — `SELECT DISTINCT k2.k_person2id`
 * (benchmark/ldbc/queries/interactive-complex-10.sql:19-24), the friends UNION of interactive-complex-3/5/6/9/11 before it
 * is joined with message, `SELECT DISTINCT p1.personid, p2.personid` above chains that leave knows (bi-14.sql:30-102), and
 * count(DISTINCT m_messageid) per person (interactive-complex-10.sql:2-9): this call over (person, message), then
 * gg_result_group_by.  A 2-hop walk table holds a friend of a friend once per middle vertex; without this call every later
 * join and count sees that person once per walk.
 * Input: the `hops`-hop table of `res` — whatever gg_result_filter_value accepts: plain, filtered, extended and
 * gg_result_top_rows tables and this call's own output.
 * Columns: `cols` holds n_cols pairwise different column numbers in 0..hops, in any order, 1 <= n_cols <= hops + 1.  Their
 * order is the output's column order: the call is a projection too.
 * Equality: two rows are equal iff their int64 cells are equal in every chosen column — raw 64-bit values, no id
 * dictionary, no CSR; a cell that is a vertex of nothing, INT64_MIN and -1 are values like any other.
 * Output: table n_cols - 1 of *out_result (k_min = k_max = n_cols - 1), whose column j is the input's column cols[j]; no
 * edge columns (the projection drops them).  n_cols == 1 gives a one-column table 0.  One row per distinct tuple: the first
 * input row that holds it, and the rows stay in input order — placed by count, scan, write, so they are identical on every
 * run, for every slot count and under every testing knob.  The result answers every reader of a walk table: gg_result_rows,
 * gg_result_fetch, gg_result_digest, both filters, gg_result_extend_edge, gg_result_group_by, gg_result_filter_value,
 * gg_result_top_rows and this call.
 * materialise == 0: only `stats` is filled (out_result may be NULL) — count(DISTINCT ...) in 64-bit counters.  stats may be
 * NULL when materialising.  One host synchronisation when counting, two when rows are written.
 * How: an open-addressing table of 32-bit row numbers (4 bytes per slot whatever n_cols is, no sentinel among the ids), a
 * power of two strictly greater than rows_in — the next power of two >= 2 rows_in by default, at most 2^32 — so an empty
 * slot always exists; the probe loop is bounded by the slot count all the same, and a row that exhausts it makes the call
 * GG_ERR_STATE.
 * Errors: NULL ctx / res / cols, an object of another context, hops outside the result's k_min..k_max, n_cols outside
 * 1..hops + 1, a column outside 0..hops or repeated, materialise != 0 with NULL out_result, stats and out_result both NULL:
 * GG_ERR_INVALID_ARG.  A result of another kind: GG_ERR_INVALID_ARG or GG_ERR_STATE by the rule of gg_result's kinds
 * (above).  An input of 2^32 rows or more: GG_ERR_TOO_LARGE — row numbers are 32-bit here, as in gg_result_top_rows.  A
 * table that does not fit: GG_ERR_OOM.  After every error the context stays usable.  An empty input gives GG_OK, an empty
 * table and slots == 0. */
typedef struct gg_distinct_stats {
  uint64_t rows_in;      /* rows of the input table */
  uint64_t rows_out;     /* distinct tuples over the chosen columns */
  uint64_t slots;        /* slots of the table the call used (0: nothing to do) */
  uint64_t probe_steps;  /* slots inspected by the insert pass, a diagnostic: may differ from run to run */
} gg_distinct_stats;
int gg_result_distinct(gg_ctx *ctx, const gg_result *res, int hops, const int *cols, int n_cols,
                       int materialise, gg_distinct_stats *stats /* nullable when materialising */,
                       gg_result **out_result /* NULL allowed iff materialise == 0 */);
/* GROUP BY several columns of a materialised walk table: count(*), count(x), sum(x), min(x) and max(x) per tuple, on the
 * device.
 * What it replaces in the reference: PhysicalHashAggregate (src/execution/operator/aggregate/physical_hash_aggregate.cpp:
 * 152-266) above a join chain whose statement groups by more than one column, by a cell that is a vertex of no CSR, or
 * under min / max — `GROUP BY m.friendid, t.t_name` under count(*) (benchmark/ldbc/queries/bi-10-shortestpath.sql:74),
 * `min(hopCount) ... GROUP BY startPerson, friend` (bi-10-shortestpath.sql:28-30), `GROUP BY person1id, person2id` with a
 * summed score (bi-14.sql:111) and `max(l_creationdate) ... GROUP BY l_personid` (interactive-complex-7.sql:7-12).
 * gg_result_group_by groups by exactly one column whose cells are vertices of a CSR and forms count(*) and sum only.
 * Input, cols, equality: exactly gg_result_distinct's — whatever walk table that call accepts, its own output included;
 * `cols` holds n_cols pairwise different column numbers in 0..hops, 1 <= n_cols <= hops + 1, in output order; cells are raw
 * int64 values, no dictionary, no CSR.
 * The value of a row: exactly gg_result_filter_value's — `values` is V(value_csr) int64 in vertex-table order, host memory,
 * `valid` (nullable) its bits; the cell of value_col is looked up as gg_csr_lookup does, and the row has the value iff the
 * cell is a vertex whose valid bit is set.  value_col may be one of the key columns or any other column in 0..hops.
 * value_col == -1 is the count form and requires value_csr, values and valid all NULL: no lookup, no sum / min / max state.
 * Aggregates per group, by SQL's NULL rules: rows = count(*); valued = count(x), the group's rows that have a value; sum
 * over the valued rows as a 128-bit two's-complement integer mod 2^128 (sum_lo, sum_hi), like gg_result_group_by's total;
 * min / max signed over the valued rows.  A group with valued == 0 reports sum 0 and min = max = 0: the reader tells NULL
 * from valued.  In the count form valued, sum_lo, sum_hi, min and max are all 0 (no sum is formed); fetching them gives
 * zeros.
 * Output: a result of the kind "aggregates per key tuple", one row per distinct tuple.  Key column j is the input's column
 * cols[j], taken from the first input row that holds the tuple, and the rows are in input order of those first rows:
 * exactly the rows and the order gg_result_distinct returns for the same cols.  Placement is count, scan, write.  The rows
 * and every aggregate are identical on every run, on both routes, for every slot count, under gg_debug_distinct's and
 * gg_debug_group_tuples' knobs and under gg_debug_max_grid_tiles: everything is integer addition mod 2^64 / 2^128 and
 * integer min / max.  Only gg_tuple_groups_rows / gg_tuple_groups_fetch answer the result; every other reader refuses it
 * with GG_ERR_STATE, and those two refuse every other kind so (gg_result's kinds, above).
 * How: gg_result_distinct's table of 32-bit row numbers gives every tuple one slot and its first row; count and scan give
 * a first row its rank; a second pass over the rows adds each run of equal adjacent rows of a wavefront to the cell of
 * its tuple's rank — state is sized by the number of groups, not of slots.  Two routes, chosen per call
 * (stats->route): workgroup-private cells in LDS when the groups fit 48 KiB (1024 valued cells, 6144 count cells), flushed
 * with one set of global atomics per touched cell and workgroup; global cells otherwise.
 * stats (nullable) and out_result (NULL: stats only — then no aggregate is formed, rows_valued is counted by a pass of its
 * own and route says what the groups would have taken).  One host synchronisation when only stats are asked for, two when
 * rows are written.
 * Errors: NULL ctx / res / cols, an object of another context, hops outside the result's k_min..k_max, n_cols outside
 * 1..hops + 1, a column outside 0..hops or repeated, value_col outside -1..hops, value_col >= 0 with NULL value_csr or
 * values, value_col == -1 with a non-NULL value_csr, values or valid, stats and out_result both NULL:
 * GG_ERR_INVALID_ARG.  A result of another kind: GG_ERR_INVALID_ARG or GG_ERR_STATE by the rule of gg_result's kinds.  A
 * shard CSR: GG_ERR_STATE.  An input of 2^32 rows or more: GG_ERR_TOO_LARGE.  State that does not fit: GG_ERR_OOM.  A row
 * that exhausts the probe bound of the tuple table (which always has an empty slot): GG_ERR_STATE.  After every error the
 * context stays usable.  An empty input gives GG_OK, zero groups and slots == 0. */
typedef struct gg_group_tuples_stats {
  uint64_t rows_in;      /* rows of the input table */
  uint64_t rows_valued;  /* of those, rows that have a value (0 without a value column) */
  uint64_t groups;       /* rows of the output = distinct tuples over the chosen columns */
  uint64_t slots;        /* slots of the tuple table (0: nothing to do) */
  uint64_t probe_steps;  /* diagnostic, may differ from run to run */
  uint32_t route;        /* 0 nothing to do, 1 workgroup-private LDS cells, 2 global cells */
} gg_group_tuples_stats;
int gg_result_group_tuples(gg_ctx *ctx, const gg_result *res, int hops, const int *cols, int n_cols,
                           int value_col /* -1: none */, const gg_csr *value_csr, const int64_t *values,
                           const uint64_t *valid /* nullable */, gg_group_tuples_stats *stats /* nullable */,
                           gg_result **out_result /* NULL: stats only */);
/* The readers of gg_result_group_tuples' result.  _rows: the number of groups and of key columns (either pointer may be
 * NULL, not both).  _fetch: rows [offset, offset + max_rows) clamped to the result, *n_out their number; `keys` holds
 * n_key_cols pointers (NULL: no key column is asked for), each nullable, and every other column pointer is nullable too.
 * The 128-bit sum of a row is sum_hi * 2^64 + (uint64_t)sum_lo.  A result of another kind: GG_ERR_STATE; NULL res or
 * n_out: GG_ERR_INVALID_ARG. */
int gg_tuple_groups_rows(const gg_result *res, uint64_t *n_rows, int *n_key_cols);
int gg_tuple_groups_fetch(const gg_result *res, uint64_t offset, uint32_t max_rows,
                          int64_t *const *keys /* n_key_cols pointers, each nullable */,
                          uint64_t *rows, uint64_t *valued, int64_t *sum_lo, int64_t *sum_hi,
                          int64_t *min, int64_t *max /* each nullable */, uint32_t *n_out);
/* Forget the staged edge rows but keep the staged vertex table (several edge tables, one vertex set). */
int gg_staging_clear_edges(gg_ctx *ctx);
/* Replace the staged vertex table by the distinct endpoint ids of the staged edge rows, in ascending
 * (signed) order — the vertex set a join chain over the edge table ALONE ranges over
 * (`knows k1, knows k2 WHERE k1.k_person2id = k2.k_person1id`, benchmark/ldbc/queries/
 * interactive-complex-3.sql:9-11: no vertex table in the pattern, so every id that occurs is a vertex
 * and no edge row is dropped).  keep_staged_vertices != 0: the new table is the UNION of the ids already
 * staged as vertices and the endpoints (several edge tables over one id space: derive from the first,
 * gg_staging_clear_edges, stage the next, derive again with keep).  Computed on the device (hash set +
 * radix sort); *n_vertices (nullable) receives the number of distinct ids. */
int gg_vertices_from_edges(gg_ctx *ctx, int keep_staged_vertices, uint64_t *n_vertices);

/* ---- triangles (closed 3-edge walks) --------------------------------------------------------- */
typedef struct gg_tri_stats {
  uint64_t rows;     /* triangle rows */
  uint64_t digest;   /* sum of the low 32 bits of the gg row hash of (a,b,c) as a 2-hop row, mod 2^32 */
  uint64_t wedges;   /* 2-hop walks a->b->c whose closing edge was looked for */
} gg_tri_stats;
/* The rows of
 *   knows k1, knows k2, knows k3 WHERE k1.dst = k2.src AND k2.dst = k3.src AND k3.dst = k1.src
 * with every endpoint in the vertex table: a triangle row is a triple of kept edge rows e1: a->b, e2: b->c, e3: c->a,
 * reported as (a, b, c).  The reference runs this as three hash joins, the last on two conditions
 * (src/execution/operator/join/physical_hash_join.cpp:217-254, src/execution/join_hashtable.cpp:304-476
 * Probe + NextInnerJoin); benchmark/ldbc/queries/bi-11.sql:22-33 is this chain under count(*).
 * These are closed WALKS, not simple cycles: parallel edge rows multiply (a row per choice of e1, e2, e3); a self-loop
 * a->a is the one row (a, a, a); a 2-cycle a<->b with a self-loop on a contributes (a, a, b), (a, b, a), (b, a, a) as
 * well; and every rotation of a directed 3-cycle is a row of its own.
 * order = 0: every row.  order = 1: only rows with id(a) < id(b) < id(c), the int64 vertex ids compared as signed
 * integers (not the dense indices) — bi-11's filter for counting each triangle once.  On a simple undirected graph stored
 * mirrored, order = 0 gives 6 rows per triangle and order = 1 gives 1.
 * src_ids == NULL: every vertex may be a.  Otherwise a ranges over the list, with multiplicity; ids that are not vertices
 * contribute nothing (as in gg_expand_khop).
 * stats->wedges: the 2-hop walks a->b->c the call looked at — order = 0: all those of the sources; order = 1: those with
 * id(a) < id(b) < id(c), the rest is pruned before any search.
 * materialise == 0: count and digest only (out_result may be NULL); 64-bit counters, no size limit.
 * materialise != 0: the rows are table 2 of *out_result — three int64 id columns a, b, c for gg_result_rows /
 * gg_result_fetch / gg_result_digest (whose digest equals stats->digest).  Row order is unspecified, but the rows are
 * placed by count, scan, write — no atomics-ordered append — so it is the same on every run.  2^32 rows or more fail with
 * GG_ERR_TOO_LARGE (count them, or pass source lists).
 * A shard CSR fails with GG_ERR_STATE, an order outside {0, 1} with GG_ERR_INVALID_ARG.  Edge rowids are not needed: a CSR
 * built without them is accepted (the rows with the rowids of their three edges: gg_triangles_edges).  Cycles longer than
 * 3 and shards are not served.
 * The first call on a CSR sorts a copy of its reverse rows by source (gg_bfs64_paths' copy: 4 bytes per edge, kept with
 * the CSR); order = 1 ranks the vertex ids and filters both row sets once per call. */
int gg_triangles(gg_ctx *ctx, const gg_csr *csr, const int64_t *src_ids, uint64_t n_src, int order, int materialise,
                 gg_tri_stats *stats, gg_result **out_result);
/* gg_triangles(..., materialise = 1, ...) with the ROWID of the three edge rows of every triangle row: same arguments
 * (sources with multiplicity, ids that are not vertices contribute nothing, order 0 or 1), same stats (rows, digest and
 * wedges equal gg_triangles' for the same arguments), same errors and limits (a shard CSR: GG_ERR_STATE; an order outside
 * {0, 1}: GG_ERR_INVALID_ARG; 2^32 rows or more: GG_ERR_TOO_LARGE), and like gg_expand_khop_edges it needs a CSR built
 * with edge rowids kept (GG_ERR_STATE otherwise).  This is what a late join with the payload columns of k1, k2, k3 needs:
 * the reference gathers build-side columns per match (ScanStructure::GatherResult in NextInnerJoin,
 * src/execution/join_hashtable.cpp:442-476), and two parallel rows c -> a give two result rows that are equal as ids.
 * Table 2 of the result holds the id columns a, b, c exactly as gg_triangles materialises them — the same rows at the same
 * positions — for gg_result_rows / gg_result_fetch / gg_result_digest, and three int64 edge columns: e1 the rowid of the
 * edge row a -> b, e2 of b -> c, e3 of c -> a (the rowid the Sink passed with the row, or its append position — counting
 * rows dropped as dangling — if it passed none).  The rows are exactly the distinct triples (e1, e2, e3) of kept edge rows
 * that close, one row per triple (order = 1: those with id(a) < id(b) < id(c)).  The rows of a wedge a -> b -> c with
 * several parallel closing rows c -> a are consecutive and their e3 ascends in append order; otherwise the row order is
 * unspecified and the same on every run.  gg_result_fetch_edges(res, 2, ...) hands back e1, e2, the edges of the 2-hop
 * walk a -> b -> c.
 * The first call on a CSR sorts the forward positions of its entries by destination (4 bytes per edge, kept with the
 * CSR); gg_triangles and gg_bfs64_paths never build that array. */
int gg_triangles_edges(gg_ctx *ctx, const gg_csr *csr, const int64_t *src_ids, uint64_t n_src, int order,
                       gg_tri_stats *stats, gg_result **out_result);
/* Copy rows [offset, offset+max_rows) of the edge columns e1, e2, e3 of a gg_triangles_edges result into ecols[0..2]
 * (gg_result_fetch's conventions: *n_out = 0 past the end; gg_host_alloc destinations go over the fetch lanes).  A NULL
 * result, ecols or n_out: GG_ERR_INVALID_ARG; a result without triangle edge columns: GG_ERR_STATE. */
int gg_triangles_fetch_edges(const gg_result *res, uint64_t offset, uint32_t max_rows, int64_t *const *ecols /* 3 */,
                             uint32_t *n_out);

/* ---- grouped aggregates over walks (count and sum per start or end vertex) --------------------- */
/* count(*) and sum(weight) over the h-hop walks, grouped by one end of the walk — what the reference computes with
 * PhysicalHashAggregate (src/execution/operator/aggregate/physical_hash_aggregate.cpp:152-266) above a chain of hash joins
 * (ScanStructure::NextInnerJoin, src/execution/join_hashtable.cpp:442-476) for statements like
 * benchmark/ldbc/queries/bi-8.sql:41-53 (sum(f.score) ... GROUP BY p.personid), forming every walk row only to fold it
 * away.  The result is GROUP BY over the table gg_expand_khop(csr, src_ids, n_src, h, h, materialise) would produce, for
 * every h in [k_min, k_max]: one row (vertex id, walks, total) per group,
 *   GG_GROUP_START  the group is v0; walks = the h-hop rows with that v0, total = the sum of weight[v_h] over them
 *   GG_GROUP_END    the group is v_h; total = the sum of weight[v0]
 * Sources count with multiplicity, ids that are no vertices contribute nothing, src_ids NULL means every vertex once.
 * weights: V int64 in vertex-table order (host memory); NULL: every weight is 1, total = walks, and no sum is formed.
 * Parallel edge rows and self-loops multiply as in the walk table.  walks is a u64 and wraps mod 2^64 like gg_khop_count's
 * counters; a group exists iff its wrapped count is not 0.  total is a 128-bit two's-complement integer (sum_lo, sum_hi)
 * wrapping mod 2^128: the reference's own type, sum(BIGINT) -> HUGEINT (src/function/aggregate/distributive/sum.cpp:
 * 115-118, 140-143).  The rows of a level come in ascending dense index (vertex-table order), placed by count, scan,
 * write: the same on every run and on every route.
 * Cost: k_max passes over all E entries of the CSR (the forward rows for START, the reverse rows for END) whatever the
 * source count — a caller with a handful of sources and a small k may do better expanding and grouping the rows.  Rows of
 * more entries than a threshold (gg_debug_aggregate_long_row) are reduced by a whole workgroup each.
 * stats (nullable): per level the groups and the sum of their walks; out_result (NULL: stats only) answers
 * gg_khop_aggregate_rows / gg_khop_aggregate_fetch only — gg_result_rows, gg_result_fetch and the other fetchers refuse it
 * with GG_ERR_STATE, and the two calls refuse every other result with GG_ERR_STATE.  Edge rowids are not needed.
 * GG_ERR_INVALID_ARG: NULL ctx or csr, objects of another context, hops outside 1..GG_MAX_HOPS, k_min > k_max, a group_by
 * other than the two, stats and out_result both NULL; GG_ERR_STATE: a shard CSR.  The context stays usable. */
#define GG_GROUP_START 0
#define GG_GROUP_END   1
typedef struct gg_agg_stats {
  uint64_t groups[GG_MAX_HOPS + 1];  /* rows of level h */
  uint64_t walks[GG_MAX_HOPS + 1];   /* sum of the groups' walks, mod 2^64 (= gg_khop_count's rows[h]) */
  uint64_t entries_pulled;           /* CSR entries read over all passes */
} gg_agg_stats;
int gg_khop_aggregate(gg_ctx *ctx, const gg_csr *csr, const int64_t *src_ids, uint64_t n_src, int k_min, int k_max,
                      int group_by, const int64_t *weights /* V entries or NULL */, gg_agg_stats *stats /* nullable */,
                      gg_result **out_result /* NULL: stats only */);
/* groups of level `hops` (inside the call's [k_min, k_max], else GG_ERR_INVALID_ARG) */
int gg_khop_aggregate_rows(const gg_result *res, int hops, uint64_t *n_rows);
/* Copy rows [offset, offset+max_rows) of level `hops`, in row order, into host arrays of >= max_rows entries (sum_lo and
 * sum_hi may be NULL).  *n_out = rows copied, 0 past the end (gg_result_fetch's conventions, its fetch lanes included). */
int gg_khop_aggregate_fetch(const gg_result *res, int hops, uint64_t offset, uint32_t max_rows, int64_t *vertex_id,
                            uint64_t *walks, uint64_t *sum_lo, int64_t *sum_hi /* nullable */, uint32_t *n_out);

/* The best n groups of level `hops` of an aggregate result, in rank order — the `ORDER BY <aggregate> [DESC], <id> LIMIT n`
 * that ends bi-8.sql:41-53 and the other aggregating LDBC statements, which the reference runs as PhysicalTopN
 * (src/execution/operator/order/physical_top_n.cpp:238-293, 421-454) directly above PhysicalHashAggregate.  Row a comes
 * before row b iff key(a) is better than key(b) — greater if descending != 0, else smaller — or the keys are equal and a's
 * vertex id is the smaller one as a signed int64 (in both directions: ORDER BY key [DESC], id).  Ids are unique within a
 * level, so the output is fully determined.
 *   GG_TOP_BY_WALKS  key = walks, an unsigned 64-bit value (it wraps mod 2^64 and may exceed 2^63)
 *   GG_TOP_BY_TOTAL  key = total + bias[dense index of the row's vertex], the bias sign-extended to 128 bits, the sum
 *                    wrapping mod 2^128 and compared signed.  bias: V int64 in vertex-table order like `weights` (host
 *                    memory), bi-8's `p.score +`; NULL: no bias, and csr may be NULL too.  The rows' ids are mapped
 *                    through csr's id dictionary; an id that is no vertex of csr is GG_ERR_STATE (checked when n > 0).
 * `agg` comes from gg_khop_aggregate or from this function; it is not modified.  *out_result is an aggregate result of
 * the one level `hops` with min(n, rows) rows (vertex id, walks, total) — the unbiased total as the input held it — in
 * columns of exactly that many rows; it answers gg_khop_aggregate_rows / gg_khop_aggregate_fetch and this function again.
 * n == 0: an empty result; n >= rows: every group, ordered.  LIMIT n OFFSET o is n + o here and a fetch from offset o.
 * The selection is a most-significant-byte-first radix select driven from the device, the order a one-workgroup LDS
 * sort up to GG_CHUNK_ROWS rows and stable radix passes on a permutation above; one host
 * synchronisation per call.
 * GG_ERR_INVALID_ARG: NULL ctx / agg / out_result, objects of another context, hops outside the input's levels, an
 * order_by other than the two, a bias without csr or with GG_TOP_BY_WALKS; GG_ERR_STATE: a result that is no aggregate, a
 * shard CSR, a group id unknown to csr.  The context stays usable. */
#define GG_TOP_BY_TOTAL 0 /* key = total (+ bias): 128-bit two's complement, compared SIGNED */
#define GG_TOP_BY_WALKS 1 /* key = walks: u64, compared UNSIGNED */
typedef struct gg_top_stats {
  uint64_t rows_in;       /* groups of the level */
  uint64_t rows_out;      /* min(n, rows_in) */
  uint32_t select_passes; /* digit passes the selection ran (0: nothing to select, n >= rows_in or n == 0) */
  uint32_t sort_route;    /* 0: none needed (fewer than two rows), 1: one workgroup in LDS, 2: global passes */
} gg_top_stats;
int gg_khop_aggregate_top(gg_ctx *ctx, const gg_result *agg, int hops, int order_by, int descending, uint64_t n,
                          const gg_csr *csr /* needed iff bias */, const int64_t *bias /* V entries or NULL */,
                          gg_top_stats *stats /* nullable */, gg_result **out_result);

/* ---- walks counted per (source, end vertex) pair, 64 sources a pass -------------------------------- */
/* count(*) over the h-hop walks grouped by BOTH ends — the pair form of benchmark/ldbc/queries/bi-14.sql:103-112
 * (GROUP BY person1id, person2id); with h = 2 over a mirrored knows the mutual-friend count behind
 * interactive-complex-10.sql:19-24; and, as the rows with walks != 0, the SELECT DISTINCT p1, p2 of bi-14.sql:30-102.  The
 * reference computes it with PhysicalHashAggregate on two keys
 * (src/execution/operator/aggregate/physical_hash_aggregate.cpp:152-266) above a chain of hash joins
 * (ScanStructure::NextInnerJoin, src/execution/join_hashtable.cpp:442-476), forming every walk row only to fold it away.
 * Lane i is src_ids[i] (1 <= n_src <= GG_BFS_LANES): each listed position is its own lane, so a duplicate id gives two
 * lanes with equal rows, and a source that is not a vertex has no rows.  Level h in [k_min, k_max] has one row
 * (i, id(v), walks) per lane i and vertex v whose walks != 0, walks being the number of h-walks src_ids[i] -> v.  Parallel
 * edge rows and self-loops multiply as in the walk table.  walks is a u64 and wraps mod 2^64 like gg_khop_count's counters;
 * a pair exists iff its wrapped count is not 0.
 * Targets: dst_ids NULL: every vertex may end a row; else only the vertices whose id is listed may (ids that are no
 * vertices are ignored, duplicates collapse, n_dst == 0 gives no rows — gg_bfs64's convention).  The filter applies to the
 * rows reported, never to the recurrence.
 * The rows of a level ascend by (source index, dense index of the end vertex) — gg_reach_closure's (class, vertex) order —
 * placed by count, scan, write: the same on every run, on every route and under every knob.
 * Cost: k_max passes over all E reverse entries whatever the source count; an entry none of whose 64 lanes is alive costs
 * its 4-byte index and an 8-byte mask, a live one a 512-byte row of the state.  State: 2 x 512 V bytes on the device.
 * stats (nullable): per level the rows and the sum of their walks (without targets walks[h] equals
 * gg_khop_count(csr, src_ids, n_src, h, h)'s rows[h]), the reverse entries looked at and how many of them were gathered.
 * out_result (NULL: stats only) answers gg_khop_pair_counts_rows / gg_khop_pair_counts_fetch only — every other fetcher
 * refuses it with GG_ERR_STATE, and the two calls refuse every other result with GG_ERR_STATE.  Edge rowids are not needed.
 * GG_ERR_INVALID_ARG: NULL ctx, csr or src_ids, objects of another context, n_src outside 1..GG_BFS_LANES, hops outside
 * 1..GG_MAX_HOPS, k_min > k_max, dst_ids NULL with n_dst != 0, stats and out_result both NULL; GG_ERR_STATE: a shard CSR;
 * GG_ERR_TOO_LARGE: a level of 2^32 rows or more (decided from a 64-bit count); GG_ERR_OOM: the state does not fit.  The
 * context stays usable. */
typedef struct gg_pair_stats {
  uint64_t pairs[GG_MAX_HOPS + 1];   /* rows of level h */
  uint64_t walks[GG_MAX_HOPS + 1];   /* sum of those rows' walks, mod 2^64 */
  uint64_t entries_pulled;           /* reverse entries looked at over all passes */
  uint64_t rows_gathered;            /* of those, the ones whose 512-byte state row was read (mask != 0) */
} gg_pair_stats;
int gg_khop_pair_counts(gg_ctx *ctx, const gg_csr *csr, const int64_t *src_ids, int n_src /* 1..GG_BFS_LANES */,
                        int k_min, int k_max, const int64_t *dst_ids /* nullable */, uint64_t n_dst,
                        gg_pair_stats *stats /* nullable */, gg_result **out_result /* NULL: stats only */);
/* rows of level `hops` (inside the call's [k_min, k_max], else GG_ERR_INVALID_ARG) */
int gg_khop_pair_counts_rows(const gg_result *res, int hops, uint64_t *n_rows);
/* Copy rows [offset, offset+max_rows) of level `hops`, in row order, into host arrays of >= max_rows entries (any of the
 * three may be NULL).  *n_out = rows copied, 0 past the end (gg_result_fetch's conventions, its fetch lanes included). */
int gg_khop_pair_counts_fetch(const gg_result *res, int hops, uint64_t offset, uint32_t max_rows, int64_t *src_index,
                              int64_t *vertex_id, uint64_t *walks, uint32_t *n_out);

/* ---- cheapest paths over weighted edge rows, 64 sources a pass --------------------------------------- */
/* The weighted half of the shortest-path family: cheapest_path_length / ANY SHORTEST ... COST, and the hop-bounded
 * recursive CTE under min(cost).  Weights are int64 >= 0, one per kept edge row.  Lane i is src_ids[i] (1 <= n_src <=
 * GG_BFS_LANES): each listed position is its own lane, so a duplicate id gives two lanes with equal rows, and a source that
 * is no vertex has no rows.  For lane s and vertex x
 *     cost_0(s, s) = 0, every other cell unreached;
 *     cost_r(s, x) = min(cost_{r-1}(s, x), min over the entries u -> x of x's reverse row of cost_{r-1}(s, u) (+) w(entry))
 * where (+) is addition saturating at INT64_MAX, so a reported cost of INT64_MAX means "at least".  Saturating add and min
 * are monotone, associative and commutative: every route and every launch geometry gives the same bits.  The rounds are
 * strict Jacobi rounds: a cell of round r is never computed from a cell already updated in round r.
 * The answer is cost_R.  A round that lowers no cell is a fixpoint and ends the search; R is that round, or max_hops if
 * max_hops >= 0 comes first (max_hops < 0: no bound; round V can lower nothing, non-negative weights).  So max_hops means
 * exactly "the cheapest walk of at most max_hops edges" — the relation of a hop-bounded recursive CTE under min(cost) — and
 * max_hops 0 reports the sources alone.  hops(s, x) = the round in which the final cost was first attained: the fewest edges
 * of any cheapest walk within the bound (what a backward trace needs to terminate on zero-weight cycles).
 * Parallel rows: the cheapest wins.  A self-loop never lowers anything.
 * Targets: dst_ids NULL: every vertex may have a row; else only the vertices whose id is listed (ids that are no vertices
 * are ignored, duplicates collapse, n_dst == 0 gives no rows — gg_khop_pair_counts' convention).  The filter applies to the
 * rows reported, never to the recurrence.
 * Rows: one (source index, vertex id, cost, hops) per lane and reached vertex that passes the filter, the source itself
 * included (cost 0, hops 0); they ascend by (source index, dense index of the vertex), placed by count, scan, write: the
 * same on every run, on every route and under every knob.
 *
 * gg_edge_weights: a device-resident weight column bound to one whole CSR, made once and used by any number of
 * gg_cheapest64 calls.  GG_WEIGHTS_BY_ROWID: weights[r] belongs to the edge row whose reported rowid is r (the rowid the Sink
 * passed, else the append position); needs a CSR built with rowids (GG_ERR_STATE otherwise, as gg_expand_khop_edges); a kept
 * edge row whose rowid lies outside [0, n_weights) is GG_ERR_INVALID_ARG; weights of dropped edge rows are never read.
 * GG_WEIGHTS_BY_ENTRY: n_weights == E (else GG_ERR_INVALID_ARG), in the order gg_csr_export shows; works without rowids.  A
 * negative weight that is read is GG_ERR_INVALID_ARG (decided on the device by one reduction; the message names nothing but
 * the fact).  The object holds E x 8 bytes, the weights in reverse-entry order, and makes the CSR keep its reverse rows by
 * source and their forward positions (2 x 4 E bytes, shared with gg_bfs64_paths / gg_triangles_edges).  It must be destroyed
 * before its CSR.  Other errors: GG_ERR_INVALID_ARG for NULL ctx / csr / out, weights NULL with n_weights != 0, a csr of
 * another context, an unknown `by`; GG_ERR_STATE for a shard CSR. */
#define GG_WEIGHTS_BY_ROWID 0
#define GG_WEIGHTS_BY_ENTRY 1
typedef struct gg_edge_weights gg_edge_weights; /* device-resident edge weights of one CSR; caller-owned */
int gg_edge_weights_create(gg_ctx *ctx, const gg_csr *csr, const int64_t *weights, uint64_t n_weights, int by,
                           gg_edge_weights **out);
void gg_edge_weights_destroy(gg_edge_weights *weights);
/* Cost: `rounds` passes over all E reverse entries whatever the source count, one host synchronisation per round; an entry
 * none of whose 64 lanes was lowered in the round before costs its 4-byte index and an 8-byte mask, a live one its 8-byte
 * weight and a 512-byte row.  State: about 1.8 KiB per vertex on the device.
 * stats (nullable), all exact functions of the input: rounds = the pull rounds that ran (the last one of an unbounded search
 * lowers nothing; 0 on a graph without kept edges); reached_pairs = the (lane, vertex) cells with a cost, the filter not
 * applied; cells_lowered = the cell updates over all rounds, seeds not counted; entries_pulled = rounds x E; rows_gathered =
 * of those, the entries whose source had a lane lowered in the round before (round 1: was seeded).
 * out_result (NULL: stats only) answers gg_cheapest64_rows / gg_cheapest64_fetch only — every other reader refuses it with
 * GG_ERR_STATE, and the two calls refuse every other result with GG_ERR_STATE.
 * GG_ERR_INVALID_ARG: NULL ctx, csr, weights or src_ids, objects of another context, weights made for another CSR, n_src
 * outside 1..GG_BFS_LANES, dst_ids NULL with n_dst != 0, stats and out_result both NULL; GG_ERR_STATE: a shard CSR;
 * GG_ERR_TOO_LARGE: 2^32 rows or more (decided from a 64-bit count); GG_ERR_OOM: the state does not fit.  The context stays
 * usable. */
typedef struct gg_cheapest_stats {
  uint64_t rounds;          /* pull rounds that ran */
  uint64_t reached_pairs;   /* (lane, vertex) cells with a cost, sources included, before the target filter */
  uint64_t cells_lowered;   /* cell updates over all rounds */
  uint64_t entries_pulled;  /* reverse entries looked at over all rounds: rounds x E */
  uint64_t rows_gathered;   /* of those, the ones whose 512-byte row of lowered values was read (mask != 0) */
} gg_cheapest_stats;
int gg_cheapest64(gg_ctx *ctx, const gg_csr *csr, const gg_edge_weights *weights, const int64_t *src_ids,
                  int n_src /* 1..GG_BFS_LANES */, int64_t max_hops /* < 0: to the fixpoint */,
                  const int64_t *dst_ids /* nullable */, uint64_t n_dst, gg_cheapest_stats *stats /* nullable */,
                  gg_result **out_result /* NULL: stats only */);
int gg_cheapest64_rows(const gg_result *res, uint64_t *n_rows);
/* Copy rows [offset, offset+max_rows), in row order, into host arrays of >= max_rows entries (any of the four may be NULL).
 * *n_out = rows copied, 0 past the end (gg_result_fetch's conventions, its fetch lanes included). */
int gg_cheapest64_fetch(const gg_result *res, uint64_t offset, uint32_t max_rows, int64_t *src_index, int64_t *vertex_id,
                        int64_t *cost, int32_t *hops, uint32_t *n_out);

/* The cheapest paths themselves (ANY SHORTEST under a cost), read backwards off the cost and hops cells of one gg_cheapest64
 * batch while they are still on the device: the weighted twin of gg_bfs64_paths.  The batch is gg_cheapest64(src_ids,
 * n_src <= 64) run TO THE FIXPOINT; pair i asks for the path from src_ids[pair_lane[i]] to pair_dst_ids[i].  Which of the
 * cheapest paths is pinned: for lane s and a vertex x with hops(s, x) = h >= 1 and cost(s, x) = c < INT64_MAX,
 *     pred(s, x) = the first entry u -> x of x's reverse row that satisfies all of
 *                    u has a cost in lane s;
 *                    cost(s, u) (+) w(entry) == c, (+) the saturating add of gg_cheapest64;
 *                    hops(s, u) == h - 1;
 * "first" in ascending (dense index of the source u, forward CSR position of the entry) — the order of the reverse rows by
 * source.  So among equally good predecessors the one with the smallest vertex-table position wins, and among parallel rows
 * of one predecessor that qualify, the row appended first.  The step's edge is that entry, reported as the rowid the Sink
 * passed with the edge row, or its append position if it passed none.  The path is p_h = t, p_{i-1} = pred(s, p_i), p_0 = s,
 * and has exactly hops(s, t) edges: the fewest of any cheapest walk.  A zero-weight cycle cannot hold the trace, because
 * hops falls by one per step.  A qualifying entry always exists at the fixpoint when c < INT64_MAX.
 * Table 1, the path rows: one row per step i = 0..h,
 *     (pair index, step i, vertex id p_i, rowid of the edge into p_i or -1 at step 0, cost(s, p_i)),
 * ascending by (pair index, step), placed by length, scan, write.  The cost column is non-decreasing along a path and the
 * difference of two steps is the weight of the later step's edge row.
 * Table 0, the pair table: one row (pair index, cost, hops, traced) per pair whose target has a cost in the pair's lane,
 * ascending by pair index; traced = 1 if the pair has path rows.
 * Two cases are outside the relation on purpose.
 *   No hop bound.  The state a bounded search ends in cannot be traced: with rows 0->3 (10), 0->1 (1), 1->2 (1), 2->3 (1),
 *   3->4 (1) and max_hops = 3, gg_cheapest64 reports cost(4) = 11 in 2 hops, derived from cost_1(3) = 10 — which round 3 then
 *   overwrote with 3, so no entry of 4's reverse row qualifies.  This call therefore takes no max_hops; bounded costs stay what
 *   gg_cheapest64 reports.
 *   Saturated pairs.  A cost of INT64_MAX means "at least", and under saturation a qualifying entry need not exist.  Such a
 *   pair is never traced, whether or not it happens to be traceable: it is listed in table 0 with traced = 0 and has no path
 *   rows.
 * s == t and s a vertex: one row of step 0 with cost 0.  An unreached target, or s or t not a vertex: no rows in either
 * table.  Duplicate pairs each get their rows; two lanes may carry one source.
 * want_edges == 0: the edge column is not computed (gg_cheapest64_paths_fetch reports -1), which is how a CSR without edge
 * rowids (GG_WEIGHTS_BY_ENTRY weights) is served; want_edges != 0 on such a CSR is GG_ERR_STATE.
 * Cost: the rounds of gg_cheapest64, then per step the reverse row of the step's vertex up to the entry taken — per entry
 * looked at 4 B of entry, 8 B of weight and one gathered 64-byte line of cost (one more of hops where the cost matched).
 * Pairs are traced in parallel, the steps of one pair one after the other.
 * stats (nullable): search = the batch's rounds, as gg_cheapest64(max_hops = -1) reports them; the other fields are exact
 * functions of the input, entries_scanned included: per step the entries of the reverse row up to and including the one
 * taken, whatever the launch geometry.
 * The result answers gg_cheapest64_paths_rows / _fetch_pairs / _fetch only — every other reader refuses it with
 * GG_ERR_STATE, and the three calls refuse every other result with GG_ERR_STATE.
 * GG_ERR_INVALID_ARG: NULL ctx, csr, weights, src_ids or out_result, objects of another context, weights made for another
 * CSR, n_src outside 1..GG_BFS_LANES, n_pairs != 0 with a NULL pair array, a pair_lane[i] >= n_src; GG_ERR_STATE: a shard
 * CSR, want_edges on a CSR without rowids, and a reached vertex without a qualifying entry (the cost state and the CSR
 * disagree: never a loop); GG_ERR_TOO_LARGE: n_pairs >= 2^32 (decided before the arrays are read), or 2^32 path rows or more
 * (decided from a 64-bit total before anything is traced).  Both outputs are cleared first; the context stays usable. */
typedef struct gg_cheapest_paths_stats {
  gg_cheapest_stats search;   /* the batch's rounds, as gg_cheapest64(max_hops = -1) reports them */
  uint64_t pairs_reached;     /* pairs whose target has a cost in the pair's lane */
  uint64_t pairs_saturated;   /* of those, cost == INT64_MAX: listed, never traced */
  uint64_t rows;              /* path rows */
  uint64_t entries_scanned;   /* reverse entries the trace looked at (exact: a function of the input alone) */
} gg_cheapest_paths_stats;
int gg_cheapest64_paths(gg_ctx *ctx, const gg_csr *csr, const gg_edge_weights *weights, const int64_t *src_ids,
                        int n_src /* 1..GG_BFS_LANES */, const uint32_t *pair_lane, const int64_t *pair_dst_ids,
                        uint64_t n_pairs, int want_edges, gg_cheapest_paths_stats *stats /* nullable */,
                        gg_result **out_result);
/* rows of table 0 (the pair table) or 1 (the path rows); another table is GG_ERR_INVALID_ARG */
int gg_cheapest64_paths_rows(const gg_result *res, int table, uint64_t *n_rows);
/* Copy rows [offset, offset+max_rows) of table 0, in row order, into host arrays of >= max_rows entries (any of the four may
 * be NULL).  *n_out = rows copied, 0 past the end (gg_result_fetch's conventions, its fetch lanes included). */
int gg_cheapest64_paths_fetch_pairs(const gg_result *res, uint64_t offset, uint32_t max_rows, int64_t *pair_index,
                                    int64_t *cost, int32_t *hops, int32_t *traced, uint32_t *n_out);
/* The same for table 1 (edge_rowid and cost may be NULL). */
int gg_cheapest64_paths_fetch(const gg_result *res, uint64_t offset, uint32_t max_rows, int64_t *pair_index, int32_t *step,
                              int64_t *vertex_id, int64_t *edge_rowid, int64_t *cost, uint32_t *n_out);

/* ---- weakly connected components: a label and a size per vertex ------------------------------------ */
/* "Which vertices hang together, and how big is each piece."  In the reference that is a UNION recursive CTE under an
 * aggregate,
 *     WITH RECURSIVE cc(v, root) AS (SELECT id, id FROM vertices
 *                                    UNION SELECT u.b, cc.root FROM cc, und u WHERE cc.v = u.a)   -- und: both directions
 *     SELECT v, min(root), count(*) FROM cc GROUP BY v
 * PhysicalRecursiveCTE (src/execution/operator/set/physical_recursive_cte.cpp:47-139) re-runs the arm's hash join once per
 * level and probes sum |component|^2 rows against one GroupedAggregateHashTable
 * (src/execution/aggregate_hashtable.cpp:367-504) before PhysicalHashAggregate
 * (src/execution/operator/aggregate/physical_hash_aggregate.cpp:152-266) folds them: quadratic in the size of the giant
 * component.  gg_reach_closure with one class per vertex would need V x V visited bits, gg_bfs64 V / 64 passes.  Here it is
 * one pass over the edge entries with a lock-free union-find, a pointer-doubling flatten and a count.
 * Two vertices are in one component iff a path of kept edge rows joins them, direction ignored: u -> v alone joins u and v.
 * Self-loops and parallel rows change nothing; rows dropped as dangling at build time do not exist; a vertex without kept
 * edges is a component of one.  The representative of a component is its member with the smallest dense index
 * (vertex-table position) and component_id is that vertex's id: the answer is a function of the tables alone, the same on
 * every run, on every build form and under every knob.
 * Table 0: V rows (vertex id, component_id, size of its component) in dense-index order.  Table 1: one row (component_id,
 * size) per component, ascending by the representative's dense index, placed by count, scan, write.
 * Cost: the E edge entries once (8 B each), 12 V bytes per pointer-doubling launch, 28 V bytes for sizes and table 0.
 * Edge rowids are not needed.  V == 0: GG_OK with two empty tables.
 * out_result (NULL: stats only) answers gg_components_rows / gg_components_fetch / gg_components_fetch_sizes only — every
 * other fetcher refuses it with GG_ERR_STATE, and the three calls refuse every other result with GG_ERR_STATE.
 * GG_ERR_INVALID_ARG: NULL ctx or csr, objects of another context, stats and out_result both NULL; GG_ERR_STATE: a shard
 * CSR.  The context stays usable. */
typedef struct gg_cc_stats {
  uint64_t vertices;      /* V */
  uint64_t components;    /* number of components (a vertex without kept edges is one) */
  uint64_t largest;       /* members of the largest component (0 if V == 0) */
  uint64_t singletons;    /* components of exactly one vertex */
  uint64_t entries_read;  /* edge entries looked at (= kept edges of the CSR) */
  uint64_t hooks;         /* successful links; equals vertices - components */
  uint32_t jump_launches; /* pointer-doubling launches of the flatten: <= ceil(log2(max(V, 2))) + jumps_per_check */
} gg_cc_stats;
int gg_components(gg_ctx *ctx, const gg_csr *csr, gg_cc_stats *stats /* nullable */,
                  gg_result **out_result /* NULL: stats only */);
/* rows of table 0 (one per vertex) or 1 (one per component); another table is GG_ERR_INVALID_ARG */
int gg_components_rows(const gg_result *res, int table, uint64_t *n_rows);
/* Copy rows [offset, offset+max_rows) of table 0 / of table 1, in row order, into host arrays of >= max_rows entries (any
 * of them may be NULL).  *n_out = rows copied, 0 past the end (gg_result_fetch's conventions, its fetch lanes included). */
int gg_components_fetch(const gg_result *res, uint64_t offset, uint32_t max_rows, int64_t *vertex_id,
                        int64_t *component_id, uint64_t *size /* each nullable */, uint32_t *n_out);
int gg_components_fetch_sizes(const gg_result *res, uint64_t offset, uint32_t max_rows, int64_t *component_id,
                              uint64_t *size /* each nullable */, uint32_t *n_out);

/* ---- 64-lane bitset BFS (shortest path length) --------------------------------------------- */
typedef struct gg_bfs_stats {
  uint32_t levels;               /* levels expanded */
  uint64_t traversed_edges;      /* sum over levels of deg(v) over vertices active in any lane */
  uint64_t active_vertices;      /* sum over levels of |{v : frontier[v] != 0}| */
  uint64_t reached_pairs;        /* (lane, vertex) pairs with dist >= 0 */
} gg_bfs_stats;

/* Lane i starts at src_ids[i] (n_src <= 64).  out_dist[i*n + j] = length of the shortest walk from
 * src_ids[i] to target j, or -1 if none of length <= max_hops (max_hops < 0: run to fixpoint).
 * Targets: dst_ids == NULL -> every vertex in vertex-table order (n = V); else the n_dst given ids
 * (ids absent from the vertex table get -1).  A source absent from the vertex table reaches nothing.
 * out_dist == NULL: run the BFS and fill *stats only (no device-to-host copy of the distances).
 * Distances up to 65 534 are recorded: a search that still has edges to follow at that level and is not bounded there by
 * max_hops fails with GG_ERR_TOO_LARGE ("deeper than 65534 levels"); the context stays usable.
 * Equals, for the reached pairs, the reference relation
 *   SELECT startPerson, friend, min(hopCount) FROM friends GROUP BY startPerson, friend
 * with the recursion bound `f.hopCount < max_hops` (bi-10-shortestpath.sql:8-31). */
int gg_bfs64(gg_ctx *ctx, const gg_csr *csr, const int64_t *src_ids, int n_src, int max_hops, const int64_t *dst_ids,
             uint64_t n_dst, int32_t *out_dist, gg_bfs_stats *stats);
/* gg_bfs64 with the answer compacted on the device: one row (source id, vertex id, distance) per reached
 * pair — the friends_shortest relation of bi-10-shortestpath.sql:26-31 for this batch of sources — instead
 * of the dense n_src x V matrix.  The rows are table 2 of *out_result: gg_result_rows(res, 2, &n),
 * gg_result_fetch(res, 2, offset, n, cols[3], &got); row order is unspecified.  Sources that are not
 * vertices contribute no row. */
int gg_bfs64_pairs(gg_ctx *ctx, const gg_csr *csr, const int64_t *src_ids, int n_src, int max_hops,
                   gg_bfs_stats *stats, gg_result **out_result);
/* The same rows as one 8-byte word each — lane << 58 | distance << 32 | dense vertex index, lane = index
 * into src_ids — in table 0 of *out_result (one column): a third of the bytes over PCIe for hosts that hold
 * the source list and the vertex ids (gg_csr_export) themselves. */
int gg_bfs64_pairs_packed(gg_ctx *ctx, const gg_csr *csr, const int64_t *src_ids, int n_src, int max_hops,
                          gg_bfs_stats *stats, gg_result **out_result);

/* The shortest paths themselves (ANY SHORTEST), read backwards off the distances of one gg_bfs64 batch while they are
 * still on the device.  The batch is gg_bfs64(src_ids, n_src <= 64, max_hops); pair i asks for the path from
 * src_ids[pair_lane[i]] to pair_dst_ids[i].  Which of the shortest paths is pinned: for a source s and a vertex x at
 * distance d >= 1,
 *     pred(s, x) = the in-neighbour of x at distance d - 1 from s with the smallest dense index (vertex-table
 *                  position);
 *     edge(s, x) = the first entry of pred(s, x)'s forward row, in CSR order (gg_csr_export), whose destination is x —
 *                  among parallel edges the one appended first; reported as the rowid the Sink passed with the edge row,
 *                  or its append position if it passed none;
 * and the path of (s, t) is p_d = t, p_{i-1} = pred(s, p_i), p_0 = s.  One row per step i = 0..d:
 *     (pair index, step i, vertex id p_i, rowid of the edge p_{i-1} -> p_i; -1 at step 0),
 * ascending by (pair index, step).  s == t and s a vertex: the one row of step 0.  No path of at most max_hops edges
 * (max_hops < 0: of any length), or s or t not a vertex: no rows.  Duplicate pairs each get their rows.
 * want_edges == 0: the edge column is not computed (gg_bfs64_paths_fetch reports -1).  want_edges != 0 on a CSR built
 * without edge rowids fails with GG_ERR_STATE, as gg_expand_khop_edges does; a shard CSR with GG_ERR_STATE; a
 * pair_lane >= n_src with GG_ERR_INVALID_ARG; 2^32 rows or more in one call with GG_ERR_TOO_LARGE (ask for fewer pairs).
 * Should a reached vertex have no in-neighbour one level closer, the distances and the CSR disagree: GG_ERR_STATE, never
 * a loop.
 * Pairs are traced in parallel, the steps of one pair one after the other — per step a piece of a reverse row, one
 * distance cell per entry looked at and a piece of a forward row: a path of 10^5 steps (a chain) is 10^5 dependent
 * steps of one lane group, slow and correct.  stats: those of the BFS.
 * The first call on a CSR sorts a copy of its reverse rows by source (4 bytes per edge, kept with the CSR).
 * The result answers gg_bfs64_paths_rows / gg_bfs64_paths_fetch only: those two refuse a walk table, a closure or level sets
 * with GG_ERR_INVALID_ARG, as the calls of those kinds refuse this result (the walk closure's included), and an aggregate,
 * pair-count, component or all-paths result with GG_ERR_STATE. */
int gg_bfs64_paths(gg_ctx *ctx, const gg_csr *csr, const int64_t *src_ids, int n_src, int max_hops,
                   const uint32_t *pair_lane, const int64_t *pair_dst_ids, uint64_t n_pairs, int want_edges,
                   gg_bfs_stats *stats, gg_result **out_result);
int gg_bfs64_paths_rows(const gg_result *res, uint64_t *n_rows);
/* Copy rows [offset, offset+max_rows), in row order, into host arrays of >= max_rows entries (edge_rowid may be NULL).
 * *n_out = rows copied, 0 past the end (gg_result_fetch's convention). */
int gg_bfs64_paths_fetch(const gg_result *res, uint64_t offset, uint32_t max_rows, int64_t *pair_index, int32_t *step,
                         int64_t *vertex_id, int64_t *edge_rowid, uint32_t *n_out);

/* How many shortest paths a pair has, and all of them (ALL SHORTEST), off the distances of one gg_bfs64 batch while they
 * are still on the device.  With the reference's operators this is a recursive UNION ALL CTE over friends_shortest joined
 * with knows once per level (src/execution/operator/set/physical_recursive_cte.cpp:60-139 over
 * src/execution/join_hashtable.cpp:304-476) and, for the number, a hash aggregate above it
 * (src/execution/operator/aggregate/physical_hash_aggregate.cpp:152-266): every path row is formed to be folded away.
 * The batch is gg_bfs64(src_ids, n_src <= 64, max_hops); pair i asks about src_ids[pair_lane[i]] -> pair_dst_ids[i].  For
 * lane s and a vertex x at distance d:
 *     sigma(s, s) = 1
 *     sigma(s, x) = SUM over the ENTRIES u -> x of x's reverse row with dist(s, u) == d - 1 of sigma(s, u)     (d >= 1)
 * An entry is a kept edge row, so parallel rows multiply: a path is a sequence of edge rows, with the join's multiplicity
 * as everywhere in this library.  A self-loop is never on a shortest path.  All sums SATURATE at 2^64 - 1 — they do not
 * wrap, unlike walk counts — so that "2^32 rows or more" can be decided from the count; saturating addition of
 * non-negative numbers is associative and commutative, so every route gives the same bits.
 * Rank order of the paths of a pair (s, t) at distance d: path number r (0-based) is found by unranking from the target
 * backwards.  At x = t with rank r go through x's reverse row in ascending order of (source dense index, forward CSR
 * position) — among parallel rows that is append order; an entry u with dist(s, u) == d - 1 is taken if r < sigma(s, u),
 * otherwise r -= sigma(s, u); continue from u with distance d - 1.  So path 0 of every pair is exactly the path
 * gg_bfs64_paths reports, vertices and edge rowids; the order is a function of the tables alone; and the edge of a step is
 * the rowid of the entry taken (the rowid the Sink passed with the row, or its append position).
 * Table 0: one row (pair index, d, sigma, kept = min(sigma, path_limit); path_limit == 0: kept = sigma) per reached pair,
 * ascending by pair index; in both modes.  materialise == 0 stops here (out_result may be NULL if only stats are wanted).
 * Table 1 (materialise != 0): one row (pair, path, step i, vertex id p_i, rowid of the edge into p_i; -1 at step 0) per
 * step of every kept path, ascending by (pair, path, step).
 * As gg_bfs64_paths: s == t and s a vertex is one path of one row; no path of at most max_hops edges, or s or t not a
 * vertex: no rows; duplicate pairs each get their rows; two lanes may carry the same source.  A shard CSR: GG_ERR_STATE;
 * materialising with want_edges on a CSR without rowids: GG_ERR_STATE; a pair_lane >= n_src: GG_ERR_INVALID_ARG; n_pairs >=
 * 2^32: GG_ERR_TOO_LARGE; the unranking running off a row (distances and CSR disagree): GG_ERR_STATE, never a loop.  When
 * materialising, paths_kept >= 2^32 or rows >= 2^32 is GG_ERR_TOO_LARGE, decided from the saturating totals before
 * anything is written (set a path_limit or ask for fewer pairs).  The context stays usable after every error.
 * State: 512 bytes per vertex for the call (GG_ERR_OOM if that does not fit).  The first materialising call on a CSR
 * sorts copies of its reverse rows by source (gg_bfs64_paths' copy, and with want_edges gg_triangles_edges').
 * The result answers gg_bfs64_all_paths_rows / gg_bfs64_all_paths_fetch_pairs / gg_bfs64_all_paths_fetch only, and those
 * three refuse every other result with GG_ERR_STATE. */
typedef struct gg_all_paths_stats {
  gg_bfs_stats bfs;          /* the batch's BFS, as gg_bfs64 reports it */
  uint64_t pairs_reached;    /* pairs with at least one path */
  uint64_t paths;            /* sum over the pairs of sigma, saturating, before path_limit */
  uint64_t paths_kept;       /* sum over the pairs of min(sigma, path_limit), saturating */
  uint64_t rows;             /* sum over the pairs of kept * (d + 1), saturating */
  uint64_t sigma_entries;    /* reverse entries looked at by the count passes: per level L the in-rows of the vertices
                                that some lane reaches at distance L */
  uint64_t sigma_gathered;   /* of those, the ones whose 512-byte sigma row was read: some lane that has the vertex at L
                                has the entry's source at L - 1 */
} gg_all_paths_stats;
int gg_bfs64_all_paths(gg_ctx *ctx, const gg_csr *csr, const int64_t *src_ids, int n_src, int max_hops,
                       const uint32_t *pair_lane, const int64_t *pair_dst_ids, uint64_t n_pairs,
                       uint64_t path_limit /* 0: none */, int want_edges, int materialise,
                       gg_all_paths_stats *stats /* nullable when materialising */, gg_result **out_result);
int gg_bfs64_all_paths_rows(const gg_result *res, int table /* 0 pairs, 1 path rows */, uint64_t *n_rows);
/* Copy rows [offset, offset+max_rows) of table 0 / of table 1, in row order, into host arrays of >= max_rows entries.
 * *n_out = rows copied, 0 past the end (gg_result_fetch's convention). */
int gg_bfs64_all_paths_fetch_pairs(const gg_result *res, uint64_t offset, uint32_t max_rows, int64_t *pair_index,
                                   int32_t *hops, uint64_t *paths, uint64_t *kept /* each nullable */, uint32_t *n_out);
int gg_bfs64_all_paths_fetch(const gg_result *res, uint64_t offset, uint32_t max_rows, int64_t *pair_index,
                             int64_t *path_index, int32_t *step, int64_t *vertex_id,
                             int64_t *edge_rowid /* nullable */, uint32_t *n_out);

/* Distinct endpoints of the walks of 1..k_max edges that start at any of the given sources — the device form of
 *   SELECT dst FROM e WHERE src = C  UNION  SELECT e2.dst FROM e e1, e e2 WHERE e1.src = C AND e1.dst = e2.src
 * (the friends / friends-of-friends table of benchmark/ldbc/queries/interactive-complex-3.sql:3-12), which the
 * reference evaluates as PhysicalUnion under a hash-aggregate dedupe
 * (src/execution/operator/set/physical_union.cpp, src/execution/operator/aggregate/physical_hash_aggregate.cpp:152-266).
 * Table 1 of *out_result has one row (vertex id, mask) per vertex that ends at least one such walk: bit h of mask
 * is set iff the vertex ends a walk of exactly h edges (walks, not shortest paths: a vertex can carry several bits,
 * and a source on a cycle is its own endpoint).  Rows come in vertex-table order; sources that are not vertices
 * contribute nothing.  Fetch with gg_result_rows(res, 1, &n) / gg_result_fetch(res, 1, offset, n, cols[2], &got). */
int gg_walk_endpoints(gg_ctx *ctx, const gg_csr *csr, const int64_t *src_ids, uint64_t n_src, int k_max,
                      gg_result **out_result);

/* Every walk from the seeds, to no fixed depth — the rows a UNION ALL recursive CTE adds to its anchor when its arm joins
 * the CTE's link column with a table's key column and carries a column of the table forward as the next link
 * (benchmark/ldbc/queries/bi-9.sql post_all, interactive-short-6.sql chain), which the reference computes by re-running
 * the arm's pipeline, hash-join build included, once per level (src/execution/operator/set/physical_recursive_cte.cpp:60-139).
 * The table's rows are the CSR's edges key -> next, built with edge rowids kept (gg_ctx_set_edge_rowid(ctx, 1)); seeds
 * are looked up as gg_csr_lookup does, and a seed that is not a vertex has no walks.  One row per walk of L >= 1 edges:
 * (index into seed_ids of its seed, rowid of its last edge as staged, L).  Rows come by level; inside a level in the
 * order of their parent rows (level 1: of the seeds), then in CSR order (the append order of the edge rows) inside the
 * parent's vertex row.
 * max_levels >= 0: walks of at most that many edges; < 0: until a level is empty.  An unbounded run in which a level
 * deeper than the vertex count is not empty has met a cycle — the reference would recurse until memory runs out — and
 * fails with GG_ERR_STATE.  That test costs V + 1 levels, each a few launches and one host round trip: on a graph of many
 * vertices a reachable cycle is a long run before the error (or a level of 2^32 walks, or the pool running out, comes
 * first) — a caller that may meet cycles bounds max_levels.  A level of 2^32 walks or more fails with GG_ERR_TOO_LARGE;
 * a shard CSR with GG_ERR_STATE; a CSR built without edge rowids with GG_ERR_STATE too, whichever build made it (no
 * rows without their rowid column), and the context stays usable.
 * The result answers gg_walk_closure_levels / gg_walk_closure_fetch only (not gg_result_rows / gg_result_fetch): those two
 * refuse a walk table, a reach closure, level sets or paths with GG_ERR_INVALID_ARG and the kinds with a refusal contract
 * of their own with GG_ERR_STATE. */
int gg_walk_closure(gg_ctx *ctx, const gg_csr *csr, const int64_t *seed_ids, uint64_t n_seeds, int max_levels,
                    gg_result **out_result);
/* *n_levels = the deepest level L with walks; rows_per_level[L - 1] = walks of L edges, for the first `capacity`. */
int gg_walk_closure_levels(const gg_result *res, uint64_t *rows_per_level, int capacity, int *n_levels);
/* Copy rows [offset, offset+max_rows) of the closure, in row order, into host arrays of >= max_rows entries (level may
 * be NULL).  *n_out = rows copied, 0 past the end (gg_result_fetch's convention). */
int gg_walk_closure_fetch(const gg_result *res, uint64_t offset, uint32_t max_rows, int64_t *seed_index,
                          int64_t *edge_rowid, int32_t *level, uint32_t *n_out);

/* Every (class, vertex) reachable from the seeds, each once — the rows a UNION recursive CTE adds to its anchor when its
 * arm joins the CTE's link column with a table's key column, carries the table's next column as the new link and keeps
 * every other column as the anchor row had it or sets it to a constant (reachability over a mirrored knows; extended_tags
 * of benchmark/ldbc/queries/interactive-complex-12.sql).  The reference re-runs the arm's pipeline, hash-join build
 * included, once per level, and probes every produced row against a GroupedAggregateHashTable of all rows emitted so
 * far, keeping the new groups only (src/execution/operator/set/physical_recursive_cte.cpp:47-70 ProbeHT / Sink,
 * :75-139 the loop).
 * The table's rows are the CSR's edges key -> next (edge rowids are not needed).  Seed i is (seed_class[i], seed_ids[i]);
 * its id is looked up as gg_csr_lookup does, and a seed that is not a vertex reaches nothing.  seed_seen[i] != 0 marks a
 * seed whose anchor row equals an arm row: its (class, vertex) is visited from the start and is never a row; an unseen
 * seed is expanded too, and is a row of the first level that reaches it again (seed_seen NULL: none is seen).  Duplicate
 * seeds are allowed.  Level L's rows are the (class, w) of the level L - 1 rows' (level 0: the seeds') out-edges that are
 * not visited yet, each once; the first level without a row ends the recursion, cycles included.
 * One row per (class, vertex) pair reached: (class, vertex id, L).  Rows come by level; inside a level ascending by
 * (class, the vertex's dense index in the CSR) — the same on every run and whichever visited set is used.
 * The visited set is a bitmap of n_classes x V bits while that fits a budget, else a hash set of keys
 * class << 32 | vertex (gg_debug_reach_visited forces either).  A level of 2^32 children or more fails with
 * GG_ERR_TOO_LARGE, as do 2^32 seeds or more; a class >= n_classes with GG_ERR_INVALID_ARG (n_classes may be any
 * uint32_t value, on either form); a shard CSR with
 * GG_ERR_STATE.  The result answers gg_reach_closure_levels / gg_reach_closure_fetch (not gg_result_rows /
 * gg_result_fetch, nor the walk closure's calls): those two refuse another of the older kinds with GG_ERR_INVALID_ARG and an
 * aggregate, pair-count, component or all-paths result with GG_ERR_STATE. */
int gg_reach_closure(gg_ctx *ctx, const gg_csr *csr, const int64_t *seed_ids, const uint32_t *seed_class,
                     const uint8_t *seed_seen, uint64_t n_seeds, uint32_t n_classes, gg_result **out_result);
/* *n_levels = the deepest level L with rows; rows_per_level[L - 1] = rows of level L, for the first `capacity`. */
int gg_reach_closure_levels(const gg_result *res, uint64_t *rows_per_level, int capacity, int *n_levels);
/* Copy rows [offset, offset+max_rows) of the closure, in row order, into host arrays of >= max_rows entries (level may
 * be NULL).  *n_out = rows copied, 0 past the end (gg_result_fetch's convention). */
int gg_reach_closure_fetch(const gg_result *res, uint64_t offset, uint32_t max_rows, int64_t *seed_class,
                           int64_t *vertex_id, int32_t *level, uint32_t *n_out);

/* The level sets of the seeds — the rows a UNION recursive CTE adds to its anchor when its arm joins the CTE's link column
 * with a table's key column, carries the table's next column as the new link and adds a positive constant to a depth
 * counter (friends(startPerson, hopCount, friend) of benchmark/ldbc/queries/bi-10-shortestpath.sql:8-25).  A row of level
 * L carries start + step * L and so never equals a row of another level: the reference's hash table of all rows so far
 * (src/execution/operator/set/physical_recursive_cte.cpp:47-70) only ever removes duplicates inside a level.
 * The table's rows are the CSR's edges key -> next (edge rowids are not needed).  Level 0 is the set of
 * (seed_class[i], seed_ids[i]); a seed that is not a vertex contributes nothing and duplicate seeds collapse.  Level
 * L >= 1 is the set of (c, w) with (c, u) in level L - 1 and u -> w an edge.  A vertex without out-edges (a NULL next's
 * sentinel) is a member and is never expanded.
 * One row (class, vertex id, L) per member of every level L >= 1.  Rows come by level; inside a level ascending by
 * (class, the vertex's dense index in the CSR) — gg_reach_closure's order, the same on every run and on every route.
 * max_levels >= 0: levels 1..max_levels; < 0: until a level is empty.  An unbounded run whose level V + 1 is not empty
 * has met a cycle — the reference would never end — and fails with GG_ERR_STATE (after V + 1 levels: a caller that may
 * meet cycles bounds max_levels).  A level of 2^32 children or more fails with GG_ERR_TOO_LARGE, as do 2^32 seeds or
 * more; a class >= n_classes with GG_ERR_INVALID_ARG; a shard CSR with GG_ERR_STATE.
 * The per-level set is a bitmap of n_classes x V bits within gg_reach_closure's budget, else a hash set sized from the
 * level's child count; a level's rows are read off the bitmap in order or claimed and sorted (DESIGN.md 4.9;
 * gg_debug_level_sets forces either).  The result answers gg_level_sets_levels / gg_level_sets_fetch only: those two
 * refuse another of the older kinds with GG_ERR_INVALID_ARG and an aggregate, pair-count, component or all-paths result with
 * GG_ERR_STATE. */
int gg_level_sets(gg_ctx *ctx, const gg_csr *csr, const int64_t *seed_ids, const uint32_t *seed_class, uint64_t n_seeds,
                  uint32_t n_classes, int max_levels, gg_result **out_result);
/* *n_levels = the deepest level L with rows; rows_per_level[L - 1] = members of level L, for the first `capacity`. */
int gg_level_sets_levels(const gg_result *res, uint64_t *rows_per_level, int capacity, int *n_levels);
/* Copy rows [offset, offset+max_rows), in row order, into host arrays of >= max_rows entries (level may be NULL).
 * *n_out = rows copied, 0 past the end (gg_result_fetch's convention). */
int gg_level_sets_fetch(const gg_result *res, uint64_t offset, uint32_t max_rows, int64_t *seed_class,
                        int64_t *vertex_id, int32_t *level, uint32_t *n_out);

/* ---- graph-sharded 64-lane BFS (one shard of the graph per GPU) ------------------------------- */
/* The layout north_star names for graphs that do not fit one GPU: `shard` comes from
 * gg_csr_build_shard; every rank holds the whole frontier (one uint64 of 64 lanes per vertex) and owns the
 * seen words, distances and result rows of its vertices.  Per level, on every rank:
 *     gg_bfs_sharded_expand   the next frontier words of the owned vertices (zero elsewhere): pulled over
 *                             their reverse rows when the frontier is heavy, pushed along the same edges
 *                             grouped by source when it is light (each rank decides from its own edges;
 *                             either way only owned words are written);
 *                             *next_words_dev points at the n_words uint64 words in HBM
 *     (exchange)              combine the ranks' words — disjoint supports, so a SUM all-reduce (RCCL through
 *                             torch.distributed on a view of that memory) is their OR; the library does
 *                             not own a communicator.  gg_bfs_sharded_words copies the words to / from the
 *                             host for hosts without a device-side collective (and for tests)
 *     gg_bfs_sharded_commit   the combined words become the next level's frontier
 * until no rank reports new pairs (or the hop bound is reached).  gg_bfs_sharded_pairs then returns the
 * rank's share of the (source, vertex, distance) rows, in the layout of gg_bfs64_pairs; their union over
 * the ranks is gg_bfs64_pairs on the whole graph.  A whole (unsharded) CSR is accepted as the 1-rank case. */
typedef struct gg_bfs_run gg_bfs_run;
int gg_bfs_sharded_begin(gg_ctx *ctx, const gg_csr *shard, const int64_t *src_ids, int n_src, gg_bfs_run **out);
int gg_bfs_sharded_expand(gg_bfs_run *run, void **next_words_dev, uint64_t *n_words, uint64_t *new_pairs_local);
int gg_bfs_sharded_words(gg_bfs_run *run, uint64_t *host_words, int write_back);
int gg_bfs_sharded_commit(gg_bfs_run *run);
int gg_bfs_sharded_pairs(gg_bfs_run *run, gg_result **out_result);
/* how many levels this rank pushed / pulled so far (diagnostic) */
int gg_bfs_sharded_levels(const gg_bfs_run *run, uint64_t *push_levels, uint64_t *pull_levels);
void gg_bfs_sharded_end(gg_bfs_run *run);

/* ---- in-library kernel timing (HIP events on the library's own stream) ---------------------- */
/* Testing knob: 1 forces gg_expand_khop onto the frontier kernels even where a product kernel applies; 2 and 3 keep
 * the all-sources product kernels out of it (as 1) but take a product form of an explicit frontier's last hops at any
 * size — 2: the last hop (pairs, sort by last vertex, fold; by itself from 65 536 frontier entries on), 3: the last two
 * hops (the frontier sorted by last vertex, k_expand_mid3's tiles over the reverse entries; by itself when the
 * frontier's children are an eighth of the edge table or more); 0 restores normal operation.  All must give identical
 * results. */
int gg_debug_force_frontier(gg_ctx *ctx, int on);
/* Testing knob: force gg_csr_build onto the multi-pass LSD build that graphs of more than 2^22 vertices
 * (and shard builds) take; both builds must export identical arrays. */
int gg_debug_force_legacy_build(gg_ctx *ctx, int on);
/* Testing knob: how the bucketed build ranks entries inside a wavefront.  0 (default): probe once whether one
 * ds_add_rtn serves colliding lanes in lane order and use it if so; 1: use it; 2: match masks by ballots.  Both
 * must export identical arrays. */
int gg_debug_rank_mode(gg_ctx *ctx, int mode);
/* Testing hook: the reverse CSR (in-neighbours) as int64 arrays — roff[V + 1], and rnbr / rrow (source / destination
 * of every reverse entry) with as many entries as the CSR keeps edges (a shard: the edges whose destination it owns);
 * any of the three may be NULL, and no more of the reverse CSR is built than the arrays asked for need (rnbr: all of it;
 * rrow without rnbr: the offsets and the row index; roff alone: the offsets).  Row x lists its sources in edge-rowid order where the bucketed build made the reverse
 * CSR, in ascending (source, rowid) order where the multi-pass build of a whole graph left it to this call.
 * *derived (may be NULL): 1 if the build derived the reverse CSR from the forward rows of a fully mirrored edge table
 * (row i + E/2 = row i with source and destination swapped, for every i), which must give the same arrays as sorting;
 * GG_MIRROR_REVERSE=0 in the environment at gg_ctx_create (or GG_MIRROR_PAIRS=0) switches that off. */
int gg_debug_csr_reverse(gg_csr *csr, int64_t *roff, int64_t *rnbr, int64_t *rrow, int *derived);
/* *ready = 1 if the CSR holds its reverse rows (rnbr), 0 if they are still to be written.  A derived build keeps only
 * the row offsets and one rotation count per vertex, and writes the rows when the first call that reads
 * them arrives (counting 1- and 2-hop walks never does); every other build has them from the start or, for the
 * multi-pass build of a whole graph, from that first call.  This call asks only: it builds and launches nothing, where
 * gg_debug_csr_reverse with an array to fill writes the rows first. */
int gg_debug_csr_reverse_ready(const gg_csr *csr, int *ready);
/* *ready = 1 if the CSR holds the row index of its reverse entries (rrow, the COO column: the row-index expansion of
 * roff), 0 if it is still to be written.  A derived build writes none: the first call that reads the column (2-hop rows
 * through a middle vertex, 3-hop counts, connected components, a sharded BFS, gg_debug_csr_reverse with rnbr or rrow)
 * has it expanded from the offsets by one kernel; counting 1- and 2-hop walks and gg_khop_partition_mid never do.  This
 * call asks only: it builds and launches nothing. */
int gg_debug_csr_reverse_index_ready(const gg_csr *csr, int *ready);
/* Testing knob (fault injection): tile `mute_tile` of every chained prefix scan never publishes its sum and the
 * tiles behind it give up after `spin_limit` polls instead of 2^24; the call that ran the scan must then
 * fail with GG_ERR_HIP instead of returning a wrong result.  spin_limit 0 and mute_tile UINT64_MAX restore
 * normal operation. */
int gg_debug_scan_fault(gg_ctx *ctx, uint32_t spin_limit, uint64_t mute_tile);
/* Testing knob: the expansion kernels split their grids into launches of at most `max_tiles` workgroups (the
 * runtime takes gridDim.x * blockDim.x in 32 bits, so a 3-hop expansion over more than ~1.3e10 2-hop rows runs
 * as several launches); 0 restores the hardware bound.  Results must not depend on it. */
int gg_debug_max_grid_tiles(gg_ctx *ctx, uint64_t max_tiles);
/* Testing knob: the visited set of gg_reach_closure.  mode 0: the budget decides, 1: the bitmap,
 * 2: the hash set, first sized max(hash_initial_slots, 2 x seen seeds) slots when hash_initial_slots != 0 (a tiny size
 * makes it grow by rebuilds).  Both forms must give identical rows in identical order. */
int gg_debug_reach_visited(gg_ctx *ctx, int mode /* 0 auto, 1 bitmap, 2 hash */, uint64_t hash_initial_slots);
/* Testing knob: gg_level_sets' per-level set (0: the budget decides, 1: the bitmap, 2: the hash set) and order route
 * (0: the byte model decides per level, 1: claim and sort, 2: read the rows off the bitmap).  The compact route needs a
 * bitmap: set_mode 2 with order_mode 2 is GG_ERR_INVALID_ARG.  Every combination must give identical rows in identical
 * order. */
int gg_debug_level_sets(gg_ctx *ctx, int set_mode /* 0 auto, 1 bitmap, 2 hash */, int order_mode /* 0 auto, 1 sort, 2 compact */);
/* Testing knob: gg_triangles stages at most `lds_entries` entries of a vertex's sorted in-row in LDS and searches
 * longer in-rows in global memory (the route of hub vertices), so that route runs on small graphs; 0 restores the
 * default, the kernel's own budget is the upper bound.  Results must not depend on it. */
int gg_debug_triangle_tile(gg_ctx *ctx, uint32_t lds_entries /* 0: default */);
/* Testing knob: gg_khop_aggregate gives rows of more than `entries` entries to a whole workgroup each and shorter ones to
 * 16 lanes, so both routes run on small graphs (1: every row of two entries or more is long; UINT32_MAX: none is); 0
 * restores the default.  Results must not depend on it. */
int gg_debug_aggregate_long_row(gg_ctx *ctx, uint32_t entries /* 0: default */);
/* Testing knob: gg_khop_aggregate_top orders its survivors by one workgroup in LDS (1; taken up to GG_CHUNK_ROWS rows,
 * more go through the global passes all the same) or by the global passes (2) whatever their number, and compacts the
 * selection's candidates once they are `candidate_floor` or fewer (1: never, there is nothing left to select by then;
 * UINT32_MAX: after the first pass that at least halves them).  0 restores either default.  Results must not depend on
 * it.  A sort_route outside 0..2 is GG_ERR_INVALID_ARG. */
int gg_debug_aggregate_top(gg_ctx *ctx, int sort_route /* 0 auto, 1 LDS, 2 global */, uint32_t candidate_floor /* 0: default */);
/* Diagnostics: the entries of the candidate list the selection of the LAST successful gg_khop_aggregate_top with
 * 0 < n < rows wrote (0: it never compacted; its passes read every row).  Read-only. */
int gg_debug_aggregate_top_listed(gg_ctx *ctx, uint64_t *list_entries);
/* Testing knob: gg_khop_pair_counts gives in-rows of more than `long_row_entries` entries to a whole workgroup each and
 * shorter ones to one wavefront (1: every row of two entries or more is long; UINT32_MAX: none is; 0: the default, 512), and
 * with gather_mode 1 reads the state row of every entry whatever its mask (0: entries whose mask is 0 are skipped).  Rows
 * and entries_pulled must not depend on either; rows_gathered equals entries_pulled with gather_mode 1.  A gather_mode
 * outside 0..1 is GG_ERR_INVALID_ARG. */
int gg_debug_pair_counts(gg_ctx *ctx, uint32_t long_row_entries /* 0: default */, int gather_mode /* 0 auto, 1 never skip */);
/* Testing knob: what gg_debug_pair_counts is to gg_khop_pair_counts, for gg_cheapest64 (the default threshold is 512 as
 * well).  With gather_mode 1 every entry counts as live and is walked whatever its mask; a lane still takes a value only
 * where the entry's own mask bit is set, which is what keeps the rounds exact.  Rows and every stats field but rows_gathered
 * must not depend on either; rows_gathered equals entries_pulled with gather_mode 1.  A gather_mode outside 0..1 is
 * GG_ERR_INVALID_ARG. */
int gg_debug_cheapest(gg_ctx *ctx, uint32_t long_row_entries /* 0: default */, int gather_mode /* 0 auto, 1 never skip */);
/* Testing knob: gg_components looks at the flatten's changed word once per `jumps_per_check` pointer-doubling launches
 * (0: the default, 4).  init_mode 0 is the default start of the forest and 1 starts every vertex as its own root; the two
 * are the same start since the other candidate (under the first smaller out-neighbour) measured slower and was removed.
 * Rows and every stats field but jump_launches must not depend on either.  An init_mode outside 0..1 is
 * GG_ERR_INVALID_ARG. */
int gg_debug_components(gg_ctx *ctx, int init_mode /* 0 default, 1 every vertex starts as its own root */,
                        uint32_t jumps_per_check /* 0: default */);
/* Testing knob: a workgroup of gg_result_extend_edge's write pass owns `tile_rows` consecutive output rows (0: the default,
 * 1024), so parents that span many tiles and runs of input rows without an edge row that are longer than a tile occur on
 * small graphs.  Results must not depend on it. */
int gg_debug_extend(gg_ctx *ctx, uint32_t tile_rows /* 0: default */);
/* Testing knob: gg_result_group_by accumulates in a workgroup-private LDS table wherever key_csr's vertices fit it (1; where
 * they do not, the global cells run all the same) or in the global cells whatever their number (2); lds_keys shrinks the
 * number of keys that table may hold (0: the default, 6144 for counts and 2048 with weights; larger values change nothing),
 * so the automatic switch and the "does not fit" case occur on small graphs.  stats->route says which route ran.  Results
 * must not depend on it.  A route outside 0..2 is GG_ERR_INVALID_ARG. */
int gg_debug_group(gg_ctx *ctx, int route /* 0 auto, 1 LDS where the table fits, 2 global */, uint32_t lds_keys /* 0: default capacity */);
/* Testing knob: what gg_debug_aggregate_top is to gg_khop_aggregate_top, for gg_result_top_rows — the two calls share their
 * passes (csrc/gg_top.h) but not this setting, so a test of one never moves the other.  sort_route 1 is taken while min(n,
 * rows_in) <= GG_CHUNK_ROWS.  Results must not depend on it.  A sort_route outside 0..2 is GG_ERR_INVALID_ARG. */
int gg_debug_value_top(gg_ctx *ctx, int sort_route /* 0 auto, 1 LDS, 2 global */, uint32_t candidate_floor /* 0: default */);
/* Testing knob: gg_result_distinct uses a table of `slots` slots (0: the default, the next power of two >= 2 rows_in).
 * slots is rounded up to a power of two and raised to the smallest power of two above rows_in where it is lower, so a forced
 * load of almost 1 stays legal and an empty slot always exists.  combine = 1: no lanes of a wavefront are combined, every
 * row probes.  Results must not depend on either.  A combine outside 0..1 is GG_ERR_INVALID_ARG. */
int gg_debug_distinct(gg_ctx *ctx, uint64_t slots /* 0: default */, int combine /* 0 auto, 1 never combine adjacent lanes */);
/* Testing knob: gg_result_group_tuples accumulates in workgroup-private LDS cells wherever the groups fit them (1; where
 * they do not, the global cells run all the same) or in the global cells whatever their number (2); lds_groups shrinks the
 * number of groups those cells may hold (0: the default, 6144 in the count form and 1024 in the valued form; larger values
 * change nothing), so both routes and the boundary occur at small sizes.  The call's tuple table obeys gg_debug_distinct.
 * stats->route says which route ran.  Results must not depend on it.  A route outside 0..2 is GG_ERR_INVALID_ARG. */
int gg_debug_group_tuples(gg_ctx *ctx, int route /* 0 auto, 1 LDS where the groups fit, 2 global */,
                          uint32_t lds_groups /* 0: default capacity */);
/* Testing hook, stateless: the library's shared exclusive prefix scan over a host array.  `in` and `out` are n values of
 * `width` bytes (4: uint32, 8: uint64); out[i] = in[0] + ... + in[i-1] — the width-4 form mod 2^32 — and *total is the
 * exact sum in 64 bits, which must stay below 2^62 (the scan's status words keep two flag bits; a larger sum is not
 * defined).  out == in scans in place on the device, otherwise out of place.  A width other than 4 or 8 is
 * GG_ERR_INVALID_ARG. */
int gg_debug_scan(gg_ctx *ctx, const void *in, uint64_t n, int width /* 4 or 8 */, void *out, uint64_t *total);
/* Testing hook, stateless: the library's shared stable radix sort over host arrays.  n < 2^31 (key, a) pairs — triples with b, which
 * may be NULL together with b_out — are sorted by key < 2^key_bits into (key_out, a_out, b_out).  Key 0xFFFFFFFF means "no
 * element": *n_valid is the number of other keys, the first *n_valid outputs are their stable sort, and the rest hold
 * GG_DEBUG_SORT_PREFILL, which every device output is filled with beforehand.  key_bits >= 32 is GG_ERR_INVALID_ARG (the
 * library's internal refusal of whole-word keys), and nothing is written. */
#define GG_DEBUG_SORT_PREFILL 0xA5A5A5A5u
int gg_debug_sort_pairs(gg_ctx *ctx, const uint32_t *key, const uint32_t *a, const uint32_t *b /* nullable */, uint64_t n,
                        int key_bits, uint32_t *key_out, uint32_t *a_out, uint32_t *b_out /* nullable */,
                        uint64_t *n_valid);
/* Every testing knob above and gg_ctx_set_edge_rowid back to its default (a test suite that shares one context
 * calls this between tests). */
int gg_debug_reset(gg_ctx *ctx);
/* Diagnostics of the pool's placement of large result columns (DESIGN.md 4.2 "Placement"): how many column sets this
 * context has placed by probing, and how many of the three pairs of the LAST set lie in different memory ranks (3 = every
 * column in its own rank class, the 7.2 TB/s case; 2 = two classes, 7.0; 0 = one class or never probed).  Read-only. */
int gg_debug_placement(gg_ctx *ctx, uint64_t *sets_built, uint64_t *fast_pairs_of_last_set);
/* The context's device pool: how many blocks it holds, and how many of them are handed out right now (to a live CSR or
 * result, or inside a running call).  A block that is never given back shows as in_use growing from call to call, one
 * given back twice or lost as the counts of two identical rounds of calls differing.  Read-only; either may be NULL. */
int gg_debug_pool(gg_ctx *ctx, uint64_t *blocks, uint64_t *in_use);
/* The pool's fill mode.  GG_POOL_FILL=<0..255, decimal or 0x..> in the environment of gg_ctx_create makes the context set
 * every device block it hands out, fresh or recycled, to that byte over the block's whole size before its first use (and
 * the staging columns beyond the rows they hold), so that a test decides what scratch memory holds when an operation
 * starts; unset or anything else: off.  gg_debug_reset leaves the mode alone.  *fill = the byte, or -1 when off;
 * *blocks_filled / *bytes_filled = blocks and bytes filled since the context was created.  Read-only; any may be NULL. */
int gg_debug_pool_fill(const gg_ctx *ctx, int *fill, uint64_t *blocks_filled, uint64_t *bytes_filled);
/* Diagnostics of the LAST 64-lane BFS of this context (gg_bfs64 and every call that runs one: pairs, paths, all paths):
 * what its levels recorded about themselves on the device, as the host read it back when the search ended.  *n_levels =
 * stats.levels + 1 entries (entry 0: the seed; entry l: level l), 0 if no BFS ran since gg_ctx_create / gg_debug_reset or
 * the last call ran no level (no sources, no targets, no vertices).  out receives min(*n_levels, cap_levels) entries of
 * four words: n_active (vertices of the frontier the level produced), te (their out-degrees), reached (its new (lane,
 * vertex) cells) and cur, the word buffer (0 / 1) that holds that frontier — a level that pulled flipped it, one that
 * pushed kept it, so cur's flips are the direction each level took.  *cell_bytes = bytes of a distance cell in the run
 * that answered (1, or 2 after the rerun of a search deeper than 254 levels); *pull_factor = the compiled threshold: level l
 * pulls iff te[l - 1] * pull_factor > E.  Read-only; every pointer but ctx may be NULL (out only with cap_levels 0). */
int gg_debug_bfs_steps(gg_ctx *ctx, uint64_t *out, uint64_t cap_levels, uint64_t *n_levels, int *cell_bytes,
                       int *pull_factor);

int gg_profile_enable(gg_ctx *ctx, int on);
/* Time only the kernels named in the comma-separated list (NULL: every kernel).  Two event records per
 * launch are not free — ~35 launches per build + expansion cost 0.3 ms of a 3.9 ms step — so a timed
 * region restricts them to the kernels it reports on. */
int gg_profile_select(gg_ctx *ctx, const char *names);
int gg_profile_reset(gg_ctx *ctx);
/* Number of distinct kernels seen; then per index: name, launches, total milliseconds. */
int gg_profile_count(gg_ctx *ctx, int *n);
int gg_profile_get(gg_ctx *ctx, int index, const char **name, uint64_t *launches, double *total_ms);

#ifdef __cplusplus
}
#endif
#endif /* GG_H */
