// gg_operators.hpp — DuckDB physical operators backed by the MI355X graph kernels (libgg.so).
//
// Host side of the drop-in: these classes implement the reference's own operator interface
// (src/include/duckdb/execution/physical_operator.hpp:24-165 in cwida/duckdb-pgq.old) and call the
// C-ABI of include/gg.h where the reference's operators call their CPU data structures:
//
//   PhysicalGGVertexSink / PhysicalGGEdgeSink   <->  PhysicalHashJoin::Sink/Combine/Finalize
//        (src/execution/operator/join/physical_hash_join.cpp:128-185): the "build side" of the
//        adjacency index; Sink is called concurrently from the pipeline's worker threads with
//        <=1024-row DataChunks, Finalize once.
//   PhysicalGGPathExpand                         <->  the chain of PhysicalHashJoin::Execute probes
//        (physical_hash_join.cpp:217-254) of a k-hop pattern; a source that emits the walks.
//   PhysicalGGShortestPath                       <->  PhysicalRecursiveCTE + min(hop) aggregate
//   PhysicalGGShortestPathRows                   <->  (no counterpart: the paths behind those hop counts, unnested)
//   PhysicalGGAllShortestPaths                   <->  PhysicalRecursiveCTE (UNION ALL) over friends_shortest x knows [+ count]
//        (src/execution/operator/set/physical_recursive_cte.cpp:48-139) for the bi-10 friends CTE.
//
// The sources whose rows stay on the device (here path expansion and the shortest-path ones) hand them to the pipeline's
// threads through one helper, GGResultDrain + GGResultSlab below: claim under a lock, fetch without one.  The sources
// behind the later table functions (triangles, the edge filter, the extension and what follows it, the aggregates, ...)
// are declared in the .cpp that registers their function, over the bases of gg_table_function.hpp.
//
// Compiled against the reference's headers; duckdb symbols are resolved by the hosting libduckdb at
// load time (the library is loaded as an extension: gg_duckdb_extension.cpp).
#pragma once

#include <atomic>
#include <functional>
#include <memory>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "duckdb.hpp"
#include "duckdb/execution/physical_operator.hpp"
#include "gg.h"

namespace duckdb {
class TableCatalogEntry;
struct GGExpandStream;

//! Device graph shared by the sinks that build it and the sources that query it.
struct GGGraph {
	//! keep_edge_rowids: the CSR keeps the rowid the edge sink gets as its third column (walks with their edges)
	//! parts > 1: the graph is ownership-sharded (gg_csr_build_shard, gg.h) — this object is part 0 and `peers`
	//! are parts 1..parts-1, each with a context of its own on device part % gg_device_count.  The sinks hand every
	//! chunk to every part (a part skips the rows it does not own before the id lookups), the parts build side by
	//! side, and the only source that accepts such a graph is the count of all 2-hop walks (k_max = 2, gg.h), whose per-part
	//! counts add (no data-path collective: SURVEY.md section 8e).
	explicit GGGraph(int device, bool keep_edge_rowids = false, int parts = 1);
	~GGGraph();
	//! number of graphs a plan counting the 2-hop walks of all sources is sharded over: GG_DEVICES (default 1)
	static int ConfiguredParts();
	int Parts() const {
		return 1 + (int)peers.size();
	}
	GGGraph &Part(int p) {
		return p == 0 ? *this : *peers[p - 1];
	}
	//! fn(part index, part) on one thread per part; the first exception is rethrown on the caller's
	void ForEachPart(const std::function<void(int, GGGraph &)> &fn);
	//! Turn a non-zero gg status into the exception the reference's operators would throw.
	static void Check(int rc, const char *what);

	int device = 0;
	gg_ctx *ctx = nullptr;        // taken from / returned to a pool of idle contexts
	gg_csr *csr = nullptr;        // path graph
	gg_csr *filter_csr = nullptr; // optional second edge table over the same vertex set (same-neighbour filter)
	std::mutex lock; // gg calls other than the appends are externally serialised (gg.h)
	vector<unique_ptr<GGGraph>> peers;
	//! Host copy of the path CSR's vertex table (dense index -> id), exported once per build and shared by the
	//! statements that unpack dense indices on the host (a pinned graph serves many: 3.6 MB through pageable memory
	//! per SF100 statement otherwise).  Callers hold `lock`; PhysicalGGEdgeSink::Finalize drops it with the CSR.
	shared_ptr<const vector<int64_t>> VertexIds();
	shared_ptr<const vector<int64_t>> vertex_ids;
};

//! Copy one integer key column of a chunk into `out` (BIGINT or INTEGER physical type, any vector
//! type via Orrify); rows whose key is NULL in ANY of the given columns are skipped, as
//! JoinHashTable::PrepareKeys does for join keys (src/execution/join_hashtable.cpp:126-148).
idx_t GGExtractKeys(DataChunk &input, const vector<idx_t> &cols, vector<vector<int64_t>> &out);
//! Same, without the copy where possible: if every requested column is a flat, all-valid BIGINT vector
//! (what DataTable::Scan produces for NOT NULL BIGINT columns) `keys[c]` points into the chunk itself,
//! otherwise into `scratch` filled by GGExtractKeys.  Returns the number of rows behind each pointer.
idx_t GGKeyColumns(DataChunk &input, const vector<idx_t> &cols, vector<vector<int64_t>> &scratch,
                   vector<const int64_t *> &keys);

//! Owner of a device-resident result (gg.h): destroyed with its owner, or when another result takes its place.
struct GGResultDestroy {
	void operator()(gg_result *result) const {
		gg_result_destroy(result);
	}
};
typedef std::unique_ptr<gg_result, GGResultDestroy> GGResultPtr;
//! The `gg_result **out` argument of a C-ABI call that fills `owner`: GGGraph::Check(gg_x(..., GGResultOut(owner)), ..).
//! What the call left in the slot is the owner's when the statement ends, also when Check throws.
class GGResultOut {
public:
	explicit GGResultOut(GGResultPtr &owner_p) : owner(owner_p) {
	}
	~GGResultOut() {
		owner.reset(slot);
	}
	operator gg_result **() {
		return &slot;
	}

private:
	GGResultPtr &owner;
	gg_result *slot = nullptr;
};

//! A thread's window onto a device-resident result table: up to SLAB_ROWS rows of up to GG_MAX_HOPS+1
//! int64 columns in page-locked host memory (gg_host_alloc), refilled with one copy per column and served
//! to the pipeline in <=1024-row DataChunks.  This is the LocalSourceState of the GG sources, so several
//! pipeline threads drain one result concurrently, each through its own slab (GGResultDrain::Refill).
class GGResultSlab : public LocalSourceState {
public:
	//! 2 MB per column and fetch: a result drains at 44 GB/s in copies of that size over the library's fetch lanes
	//! (36 at 1 MB, 48 at 4 MB, 51 at 8 MB — scripts/bench_fetch.py, profiles/r04_bench_fetch.txt; 22-29 GB/s before
	//! the lanes) against twice / four times the page-locked memory per thread
	static constexpr idx_t SLAB_ROWS = 1u << 18;
	//! pipeline threads worth starting on a result of `rows` rows: one per slab of it
	static idx_t ThreadsFor(idx_t rows) {
		return MaxValue<idx_t>(1, rows / SLAB_ROWS);
	}

	explicit GGResultSlab(shared_ptr<GGGraph> graph);
	~GGResultSlab() override;

	//! make room for `columns` columns; returns the column base pointers
	int64_t **Columns(idx_t columns);
	//! serve the next <=1024 rows: the first `columns` columns as they are, into chunk.data[first ..]; sets the cardinality
	idx_t Emit(DataChunk &chunk, idx_t first, idx_t columns);

	shared_ptr<GGGraph> graph;
	int64_t *memory = nullptr;
	idx_t capacity_columns = 0;
	int64_t *column[2 * GG_MAX_HOPS + 1]; // (GG_EXTEND: hops + 2 id columns and hops + 1 edge columns, hops < GG_MAX_HOPS)
	idx_t rows = 0, pos = 0; // filled rows, next row to serve
	int table = 0;           // which table of the result the slab holds (hop length / batch)
};

//! The scan position the pipeline threads of a source share, and the one place where the protocol between them is
//! written down: the result that stands in HBM right now, the table of it that is being handed out (hop length /
//! batch), and the next row of that table nobody has claimed.
//!   - A thread claims up to SLAB_ROWS rows under `lock` and fetches them into its own slab with NO lock held (the
//!     library's fetch lanes rely on that); `fetching` counts the claims whose fetch has not ended.  It is raised under
//!     the lock at claim time and lowered on every exit from the fetch, an exception included.
//!   - The result is replaced only under `lock` and only once `fetching` is 0: never under a fetch that reads it.
//!   - Lock order: `lock`, then GGGraph::lock.  `lock` stays held through the device call that makes the next part or
//!     batch — the other threads have nothing to claim until its rows exist.
//!   - The slab carries the table it was claimed from (GGResultSlab::table): rows are emitted by that tag, never by
//!     the table the drain has moved on to.
class GGResultDrain {
public:
	//! the device call that makes the next result (taking the GGGraph::lock it needs) and says how many rows its first
	//! table has
	typedef std::function<GGResultPtr(idx_t &rows)> produce_t;
	//! called under `lock` when the current table is claimed completely: move to the next table (Open), part or batch
	//! (Replace); false: nothing is left
	typedef std::function<bool()> advance_t;
	//! copies rows [offset, offset + want) of `table` into the slab (slab.Columns(n) in here: a pinned allocation that
	//! throws must not leave `fetching` raised); returns the rows copied
	typedef std::function<uint32_t(gg_result *result, int table, idx_t offset, uint32_t want, GGResultSlab &slab)> fetch_t;

	//! Caller holds `lock` (or is single-threaded).  Waits for the fetches in flight (polling the interrupt flag),
	//! destroys the current result — one is resident at a time — and installs the one `produce` makes, open at `table`.
	void Replace(ClientContext &context, int table, const produce_t &produce);
	//! Caller holds `lock`.  Another table of the same result: hand out its `rows` rows from the first.
	void Open(int table_p, idx_t rows_p) {
		table = table_p;
		rows = rows_p;
		offset = 0;
	}
	//! Claim the next rows and fetch them into the slab; false: the slab has no rows (nothing is left to claim).
	bool Refill(GGResultSlab &slab, const advance_t &advance, const fetch_t &fetch);

	int Table() const {
		return table;
	}
	idx_t Rows() const {
		return rows;
	}

	std::mutex lock;

private:
	GGResultPtr result;              // in HBM
	int table = 0;                   // the table of it being handed out
	idx_t rows = 0, offset = 0;      // rows of that table, next unclaimed one
	std::atomic<idx_t> fetching {0}; // slab fetches still reading `result` (it may not be freed under them)
};

//! A source list for the C-ABI: an EMPTY list must not arrive as a null pointer (gg.h: null means every vertex).
const int64_t *GGSourceIds(const vector<int64_t> &sources);
//! The `hops`-hop walk table from `sources` (all_sources: from every vertex), left on the device (gg_expand_khop_result,
//! include/gg.h).  Caller holds graph.lock.
void GGExpandWalks(GGGraph &graph, const vector<int64_t> &sources, bool all_sources, int hops, GGResultPtr &out);

//! The global source state of the operators that answer (src, dst) pairs from 64-source device batches (gg_shortest_paths.cpp,
//! gg_cheapest.cpp): the pairs grouped by source, and the drain of the batch that is resident.
class ShortestPathRowsState : public GlobalSourceState {
public:
	idx_t MaxThreads() override {
		return max_threads;
	}
	vector<int64_t> uniq;            // distinct sources, in first-occurrence order; batch b holds uniq[64 b ..]
	vector<vector<idx_t>> members;   // per batch: the pairs (indices into src / dst) of its sources, ascending
	vector<vector<uint32_t>> lanes;  // per batch and member: the source's lane
	GGResultDrain drain;             // the path rows of the current batch; its table is the batch
	idx_t max_threads = 1;

	//! group the pairs by source, 64 distinct sources to a batch, in the order the sources first occur
	void Group(const vector<int64_t> &src) {
		std::unordered_map<int64_t, idx_t> position; // source id -> index into uniq
		for (idx_t p = 0; p < src.size(); p++) {
			auto found = position.find(src[p]);
			idx_t at;
			if (found == position.end()) {
				at = uniq.size();
				position.emplace(src[p], at);
				uniq.push_back(src[p]);
				if (at % GG_BFS_LANES == 0) {
					members.emplace_back();
					lanes.emplace_back();
				}
			} else {
				at = found->second;
			}
			members[at / GG_BFS_LANES].push_back(p);
			lanes[at / GG_BFS_LANES].push_back((uint32_t)(at % GG_BFS_LANES));
		}
	}
};

class PhysicalGGVertexSink : public PhysicalOperator {
public:
	PhysicalGGVertexSink(shared_ptr<GGGraph> graph, vector<LogicalType> types, idx_t estimated_cardinality);

	shared_ptr<GGGraph> graph;

public:
	unique_ptr<GlobalSinkState> GetGlobalSinkState(ClientContext &context) const override;
	unique_ptr<LocalSinkState> GetLocalSinkState(ExecutionContext &context) const override;
	SinkResultType Sink(ExecutionContext &context, GlobalSinkState &gstate, LocalSinkState &lstate,
	                    DataChunk &input) const override;
	void Combine(ExecutionContext &context, GlobalSinkState &gstate, LocalSinkState &lstate) const override;
	SinkFinalizeType Finalize(Pipeline &pipeline, Event &event, ClientContext &context,
	                          GlobalSinkState &gstate) const override;
	bool IsSink() const override {
		return true;
	}
	bool ParallelSink() const override {
		return true;
	}
	string GetName() const override {
		return "GG_VERTEX_SINK";
	}
};

//! Input columns: (source key, destination key[, edge rowid]).  Finalize builds the CSR.
class PhysicalGGEdgeSink : public PhysicalOperator {
public:
	//! as_filter: the rows are a SECOND edge table over the already staged vertex set; Finalize builds
	//! GGGraph::filter_csr instead of GGGraph::csr.
	//! derive_vertices: there is no vertex sink — the pattern is a join chain over the edge table alone
	//! (k1.dst = k2.src), so the vertex set is the distinct endpoint ids (gg_vertices_from_edges).
	//! keep_vertices (with derive_vertices): unite the endpoint ids with the vertex ids already staged (a
	//! second edge table over the same id space).  build = false: Finalize stops after the vertex set —
	//! the edge rows only contribute their endpoints (the table is ingested again for its own CSR).
	PhysicalGGEdgeSink(shared_ptr<GGGraph> graph, vector<LogicalType> types, idx_t estimated_cardinality,
	                   bool as_filter = false, bool derive_vertices = false, bool keep_vertices = false,
	                   bool build = true);

	shared_ptr<GGGraph> graph;
	bool as_filter;
	bool derive_vertices;
	bool keep_vertices;
	bool build;
	//! Clears what this sink's options say must leave the staging area before its rows go in; runs once, when the
	//! sink runs (first Sink call or Finalize), never at schedule time.
	void PrepareStaging(GlobalSinkState &gstate) const;

public:
	unique_ptr<GlobalSinkState> GetGlobalSinkState(ClientContext &context) const override;
	unique_ptr<LocalSinkState> GetLocalSinkState(ExecutionContext &context) const override;
	SinkResultType Sink(ExecutionContext &context, GlobalSinkState &gstate, LocalSinkState &lstate,
	                    DataChunk &input) const override;
	void Combine(ExecutionContext &context, GlobalSinkState &gstate, LocalSinkState &lstate) const override;
	SinkFinalizeType Finalize(Pipeline &pipeline, Event &event, ClientContext &context,
	                          GlobalSinkState &gstate) const override;
	bool IsSink() const override {
		return true;
	}
	bool ParallelSink() const override {
		return true;
	}
	string GetName() const override {
		return "GG_EDGE_SINK";
	}
};

//! Source: walks of length k_min..k_max.  Output: (hops INTEGER, v0 BIGINT, ..., v{k_max} BIGINT),
//! trailing vertices NULL for shorter walks.  count_only: (hops INTEGER, rows BIGINT, digest BIGINT,
//! traversed_edges BIGINT), one row per length.
class PhysicalGGPathExpand : public PhysicalOperator {
public:
	//! rows_only (with count_only): the row counts come from degrees (gg_khop_count) — what `count(*)` over the join
	//! chain needs; the digest column is 0 and no walk is formed.  Without it the counting expansion runs and the
	//! digest of every walk comes with the count (the gg_path_count table function, parity tests, the benchmark).
	PhysicalGGPathExpand(shared_ptr<GGGraph> graph, int k_min, int k_max, bool count_only, vector<int64_t> sources,
	                     bool all_sources, idx_t estimated_cardinality, bool rows_only = false);

	static vector<LogicalType> OutputTypes(int k_max, bool count_only);
	//! expand the current part of a stream of a result that is produced part by part (see GetGlobalSourceState)
	GGResultPtr MaterialisePart(GGExpandStream &stream, idx_t &rows) const;
	void PlanMiddleParts(GGExpandStream &stream, GGGraph &part, const gg_khop_stats &stats) const;

	shared_ptr<GGGraph> graph;
	int k_min, k_max;
	bool count_only;
	vector<int64_t> sources;
	bool all_sources;
	bool rows_only;

public:
	unique_ptr<GlobalSourceState> GetGlobalSourceState(ClientContext &context) const override;
	unique_ptr<LocalSourceState> GetLocalSourceState(ExecutionContext &context,
	                                                 GlobalSourceState &gstate) const override;
	void GetData(ExecutionContext &context, DataChunk &chunk, GlobalSourceState &gstate,
	             LocalSourceState &lstate) const override;
	bool IsSource() const override {
		return true;
	}
	bool ParallelSource() const override {
		return true;
	}
	string GetName() const override {
		return "GG_PATH_EXPAND";
	}
};

//! Streaming operator + sink: a generic INNER hash join on ONE integer key whose build side is a base-table scan —
//! the reference's PhysicalHashJoin in both of its roles (src/execution/operator/join/physical_hash_join.cpp:128-254):
//!   children[1] (a scan of the build table's key column and rowid) is SUNK into a device index keyed on the key
//!               (Sink / Combine / Finalize = the hash-join build, concurrent Sink calls; gg_edges_append, gg_csr_build);
//!   children[0] (any plan) is PROBED chunk by chunk: Execute sends the chunk's keys to the device (gg_join_probe: for
//!               every probe position the rowids of the build rows under its key), slices the probe chunk by position
//!               and fetches the build table's columns by rowid (DataTable::Fetch, as the index join does) —
//!               HAVE_MORE_OUTPUT while one probe chunk's matches exceed a DataChunk, like ScanStructure::Next.
//! Its PhysicalOperatorType is HASH_JOIN, so the reference's executor schedules it with the code it has for joins
//! (Executor::BuildPipelines, src/parallel/executor.cpp:424-442: the operator is all it looks at), also inside the
//! arms of a recursive CTE.  Output columns: `probe_columns` of the probe child's, then `build_columns` of the build table.
class PhysicalGGKeyJoin : public PhysicalOperator {
public:
	PhysicalGGKeyJoin(vector<LogicalType> types, unique_ptr<PhysicalOperator> probe, unique_ptr<PhysicalOperator> build_scan,
	                  idx_t probe_key, vector<idx_t> probe_columns, TableCatalogEntry *build_table, column_t build_key,
	                  vector<column_t> build_columns, idx_t estimated_cardinality);

	idx_t probe_key;                 // column of the probe child's chunks that holds the key
	vector<idx_t> probe_columns;     // columns of the probe child's chunks that go out, in output order
	TableCatalogEntry *build_table;
	column_t build_key;
	vector<column_t> build_columns;  // of the build table, in output order (COLUMN_IDENTIFIER_ROW_ID allowed)

public:
	// sink (build side)
	unique_ptr<GlobalSinkState> GetGlobalSinkState(ClientContext &context) const override;
	unique_ptr<LocalSinkState> GetLocalSinkState(ExecutionContext &context) const override;
	SinkResultType Sink(ExecutionContext &context, GlobalSinkState &gstate, LocalSinkState &lstate,
	                    DataChunk &input) const override;
	void Combine(ExecutionContext &context, GlobalSinkState &gstate, LocalSinkState &lstate) const override;
	SinkFinalizeType Finalize(Pipeline &pipeline, Event &event, ClientContext &context,
	                          GlobalSinkState &gstate) const override;
	bool IsSink() const override {
		return true;
	}
	bool ParallelSink() const override {
		return true;
	}
	// operator (probe side)
	unique_ptr<OperatorState> GetOperatorState(ClientContext &context) const override;
	OperatorResultType Execute(ExecutionContext &context, DataChunk &input, DataChunk &chunk,
	                           OperatorState &state) const override;
	bool ParallelOperator() const override {
		return true;
	}
	bool RequiresCache() const override {
		return true;
	}
	string GetName() const override {
		return "GG_KEY_JOIN";
	}
	string ParamsToString() const override;
};

//! Source: `hops`-hop walks WITH payload columns of the edge table (a join chain that projects columns of its edge
//! instances other than the two keys).  The device returns every walk with the rowid of each edge taken
//! (gg_expand_khop_edges); the payload columns are then fetched from the base table by rowid, in the statement's
//! transaction — the late-materialising counterpart of the gather the reference's hash join does per match from its
//! build side (src/execution/join_hashtable.cpp:466-473), through the call its index join uses
//! (DataTable::Fetch, src/execution/operator/join/physical_index_join.cpp).
//! Output: (hops INTEGER, v0 BIGINT, ..., v{hops} BIGINT, payload columns in the order given).
class PhysicalGGPathEdges : public PhysicalOperator {
public:
	//! payload: (1-based edge number of the walk, column of the edge table)
	PhysicalGGPathEdges(shared_ptr<GGGraph> graph, int hops, vector<int64_t> sources, bool all_sources,
	                    TableCatalogEntry *edge_table, vector<std::pair<idx_t, column_t>> payload,
	                    idx_t estimated_cardinality);
	static vector<LogicalType> OutputTypes(int hops, TableCatalogEntry &edge_table,
	                                       const vector<std::pair<idx_t, column_t>> &payload);

	shared_ptr<GGGraph> graph;
	int hops;
	vector<int64_t> sources;
	bool all_sources;
	TableCatalogEntry *edge_table;
	vector<std::pair<idx_t, column_t>> payload;

	//! expand the current part (slices of the sources under GG_RESULT_BUDGET_MB; caller holds graph->lock)
	void MaterialisePart(GlobalSourceState &gstate) const;

public:
	unique_ptr<GlobalSourceState> GetGlobalSourceState(ClientContext &context) const override;
	void GetData(ExecutionContext &context, DataChunk &chunk, GlobalSourceState &gstate,
	             LocalSourceState &lstate) const override;
	bool IsSource() const override {
		return true;
	}
	string GetName() const override {
		return "GG_PATH_EDGES";
	}
};

//! Source: fixed-length walks whose vertices all share a neighbour in the filter graph — Train Benchmark
//! ConnectedSegments (benchmark/trainbenchmark/queries/connectedsegments.sql:1-25): `hops` connectsTo
//! edges from the source segments, all hops+1 segments monitored by one sensor.
//! Output: (w BIGINT, v0 BIGINT, ..., v{hops} BIGINT).
class PhysicalGGFilteredPaths : public PhysicalOperator {
public:
	PhysicalGGFilteredPaths(shared_ptr<GGGraph> graph, int hops, vector<int64_t> sources,
	                        idx_t estimated_cardinality, bool all_sources = false);

	shared_ptr<GGGraph> graph;
	int hops;
	vector<int64_t> sources;
	bool all_sources; // walks may start at any vertex (no source table in the pattern)

public:
	unique_ptr<GlobalSourceState> GetGlobalSourceState(ClientContext &context) const override;
	void GetData(ExecutionContext &context, DataChunk &chunk, GlobalSourceState &gstate,
	             LocalSourceState &lstate) const override;
	bool IsSource() const override {
		return true;
	}
	string GetName() const override {
		return "GG_FILTERED_PATHS";
	}
};

//! Source: (vertex id BIGINT, h1 BIGINT, ..., hk BIGINT) — one row per vertex that ends a walk of 1..k_max edges from
//! one of the sources; h = 1 iff a walk of exactly h edges ends there (gg_walk_endpoints).  The device form of the
//! reference's hash-aggregate dedupe above a UNION of endpoint sets (interactive-complex-3.sql:3-12).
class PhysicalGGWalkEndpoints : public PhysicalOperator {
public:
	PhysicalGGWalkEndpoints(shared_ptr<GGGraph> graph, vector<int64_t> sources, int k_max, idx_t estimated_cardinality);

	static vector<LogicalType> OutputTypes(int k_max);

	shared_ptr<GGGraph> graph;
	vector<int64_t> sources;
	int k_max;

public:
	unique_ptr<GlobalSourceState> GetGlobalSourceState(ClientContext &context) const override;
	void GetData(ExecutionContext &context, DataChunk &chunk, GlobalSourceState &gstate,
	             LocalSourceState &lstate) const override;
	bool IsSource() const override {
		return true;
	}
	string GetName() const override {
		return "GG_WALK_ENDPOINTS";
	}
};

//! Source: (startPerson BIGINT, friend BIGINT, hopCount INTEGER) for every pair reached within
//! max_hops — the friends_shortest relation of benchmark/ldbc/queries/bi-10-shortestpath.sql:8-31.
//! Sources are processed in batches of 64 bit lanes.
class PhysicalGGShortestPath : public PhysicalOperator {
public:
	//! lone_sources: a source that is not a vertex of the graph (it has no edge in an edge-only vertex
	//! set) still reaches itself at hop 0 — the seed row of the recursive CTE does not depend on the edges
	PhysicalGGShortestPath(shared_ptr<GGGraph> graph, vector<int64_t> sources, int max_hops,
	                       idx_t estimated_cardinality, bool lone_sources = false);

	//! BFS of the 64-source batch starting at source `batch_base` (batches run one at a time, when the previous one
	//! is drained); caller holds graph->lock
	GGResultPtr RunBatch(GlobalSourceState &gstate, idx_t batch_base, idx_t &rows) const;

	shared_ptr<GGGraph> graph;
	vector<int64_t> sources;
	int max_hops;
	bool lone_sources;

public:
	unique_ptr<GlobalSourceState> GetGlobalSourceState(ClientContext &context) const override;
	unique_ptr<LocalSourceState> GetLocalSourceState(ExecutionContext &context,
	                                                 GlobalSourceState &gstate) const override;
	void GetData(ExecutionContext &context, DataChunk &chunk, GlobalSourceState &gstate,
	             LocalSourceState &lstate) const override;
	bool IsSource() const override {
		return true;
	}
	bool ParallelSource() const override {
		return true;
	}
	string GetName() const override {
		return "GG_SHORTEST_PATH";
	}
};

//! Source: (src BIGINT, dst BIGINT, step INTEGER, vertex BIGINT, edge_rowid BIGINT) — the pinned shortest path of every
//! (src[i], dst[i]) unnested, one row per step 0..d, edge_rowid NULL at step 0 (include/gg.h, gg_bfs64_paths).  The graph
//! must have been built with the edge table's rowids.  Pairs are grouped by source into batches of 64 bit lanes; pairs
//! without a path of at most max_hops edges (max_hops < 0: of any length) yield no row.
class PhysicalGGShortestPathRows : public PhysicalOperator {
public:
	PhysicalGGShortestPathRows(shared_ptr<GGGraph> graph, vector<int64_t> src, vector<int64_t> dst, int max_hops,
	                           idx_t estimated_cardinality);
	static vector<LogicalType> OutputTypes();

	//! BFS + trace of batch `batch` (batches run one at a time, when the previous one is drained); caller holds
	//! graph->lock
	GGResultPtr RunBatch(GlobalSourceState &gstate, idx_t batch, idx_t &rows) const;

	shared_ptr<GGGraph> graph;
	vector<int64_t> src, dst;
	int max_hops;

public:
	unique_ptr<GlobalSourceState> GetGlobalSourceState(ClientContext &context) const override;
	unique_ptr<LocalSourceState> GetLocalSourceState(ExecutionContext &context,
	                                                 GlobalSourceState &gstate) const override;
	void GetData(ExecutionContext &context, DataChunk &chunk, GlobalSourceState &gstate,
	             LocalSourceState &lstate) const override;
	bool IsSource() const override {
		return true;
	}
	bool ParallelSource() const override {
		return true;
	}
	string GetName() const override {
		return "GG_SHORTEST_PATH_ROWS";
	}
};

//! Source: every shortest path of every (src[i], dst[i]), unnested — (src BIGINT, dst BIGINT, path BIGINT, step INTEGER,
//! vertex BIGINT, edge_rowid BIGINT), at most path_limit paths of a pair (0: all), path numbers in the pinned rank order of
//! include/gg.h (gg_bfs64_all_paths), edge_rowid NULL at step 0 — or, count_only, their number: (src BIGINT, dst BIGINT,
//! hops INTEGER, paths HUGEINT), 2^64 - 1 standing for that many or more.  The graph must have been built with the edge
//! table's rowids.  Batching and draining as PhysicalGGShortestPathRows.
class PhysicalGGAllShortestPaths : public PhysicalOperator {
public:
	PhysicalGGAllShortestPaths(shared_ptr<GGGraph> graph, vector<int64_t> src, vector<int64_t> dst, int max_hops,
	                           uint64_t path_limit, bool count_only, idx_t estimated_cardinality);
	static vector<LogicalType> OutputTypes(bool count_only);

	//! BFS, count and (unless count_only) unranking of batch `batch`; caller holds graph->lock
	GGResultPtr RunBatch(GlobalSourceState &gstate, idx_t batch, idx_t &rows) const;

	shared_ptr<GGGraph> graph;
	vector<int64_t> src, dst;
	int max_hops;
	uint64_t path_limit;
	bool count_only;

public:
	unique_ptr<GlobalSourceState> GetGlobalSourceState(ClientContext &context) const override;
	unique_ptr<LocalSourceState> GetLocalSourceState(ExecutionContext &context,
	                                                 GlobalSourceState &gstate) const override;
	void GetData(ExecutionContext &context, DataChunk &chunk, GlobalSourceState &gstate,
	             LocalSourceState &lstate) const override;
	bool IsSource() const override {
		return true;
	}
	bool ParallelSource() const override {
		return true;
	}
	string GetName() const override {
		return count_only ? "GG_SHORTEST_PATH_COUNTS" : "GG_ALL_SHORTEST_PATH_ROWS";
	}
};

} // namespace duckdb
