// gg_pipeline.hpp — the device graph's build side as pipeline sinks of the reference's executor (gg_pipeline.cpp)
#pragma once

#include <functional>

#include "duckdb/common/types/chunk_collection.hpp"

#include "gg_extension.hpp"
#include "gg_operators.hpp"

namespace duckdb {

//! Where the sinks of one plan leave the graph they build and its scan picks it up; one graph per execution.
struct GGGraphSlot {
	mutex lock;
	shared_ptr<GGGraph> graph;
	int shards = 1; // GGGraphSpec::shards of the plan
};

//! PhysicalGGVertexSink / PhysicalGGEdgeSink created when the pipeline starts (the device context with them), so a
//! plan that is only explained or prepared never touches the GPU.
class PhysicalGGLazySink : public PhysicalOperator {
public:
	enum Kind { VERTICES, EDGES, EDGES_DERIVE_VERTICES, EDGES_CUSTOM };
	PhysicalGGLazySink(shared_ptr<GGGraphSlot> slot, Kind kind, vector<LogicalType> types, idx_t estimated_cardinality);
	//! an edge sink with PhysicalGGEdgeSink's own switches (plans over two edge tables: ConnectedSegments).  `first`: the
	//! sink that opens the execution's graph; `clear_edges_after`: its Finalize drops the staged edge rows once its own
	//! CSR is built (gg_staging_clear_edges: the vertex numbering stays) — every sink's global state is created when
	//! the pipelines are scheduled, before any of them runs, so nothing of that kind can happen there
	struct EdgeOptions {
		bool first = false, clear_edges_after = false;
		bool as_filter = false, derive_vertices = false, keep_vertices = false, build = true;
	};
	PhysicalGGLazySink(shared_ptr<GGGraphSlot> slot, EdgeOptions options, vector<LogicalType> types,
	                   idx_t estimated_cardinality);

	shared_ptr<GGGraphSlot> slot;
	Kind kind;
	EdgeOptions options;
	mutable unique_ptr<PhysicalOperator> inner;

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
	string GetName() const override;
};

//! A GG source over the graph its sink children build.  `factory` makes the actual source operator
//! (PhysicalGGPathExpand, PhysicalGGWalkEndpoints, ...) once the graph exists.
class PhysicalGGGraphScan : public PhysicalOperator {
public:
	//! (the context is the executing statement's: a factory may read more rows in its transaction, e.g. BFS seeds)
	using Factory = std::function<unique_ptr<PhysicalOperator>(ClientContext &, shared_ptr<GGGraph>)>;
	PhysicalGGGraphScan(vector<LogicalType> types, string name, string description, shared_ptr<GGGraphSlot> slot,
	                    Factory factory, bool parallel_result, idx_t estimated_cardinality);

	string name, description;
	shared_ptr<GGGraphSlot> slot;
	Factory factory;
	bool parallel_result;
	//! set while the plan's pipelines are built: the scan sits in a plan with a recursive CTE, whose pipelines are
	//! reset and re-run per iteration — the graph then lives as long as the plan
	mutable bool keep_graph = false;

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
		return parallel_result;
	}
	string GetName() const override;
	string ParamsToString() const override;
};

//===--------------------------------------------------------------------===//
// UNION ALL recursion over one keyed table (gg_recursive_walks.cpp, rule: PlanRecursiveWalks in gg_plan_rule.cpp)
//===--------------------------------------------------------------------===//
//! What one output column of the recursive arm is
struct GGWalkColumn {
	enum Kind { CARRIED, TABLE, CONSTANT, COUNTER } kind = CARRIED;
	idx_t index = 0;     // TABLE: column of the arm table's rows
	Value constant;      // CONSTANT
	int64_t step = 0;    // COUNTER: anchor value + step x level
};

//! The rows both sinks collect and the source reads
struct GGWalkInput {
	mutex lock;
	ChunkCollection anchor; // the anchor's rows, in the CTE's column layout
	ChunkCollection table;  // the arm table's rows (row number = edge rowid)
	idx_t link_column = 0;  // of the anchor (and of the CTE)
	idx_t key_column = 0;   // of the table: joined with the link
	idx_t next_column = 0;  // of the table: the next level's link
	int max_levels = -1;    // from `counter < K` on the CTE side; -1: until a level is empty
	vector<GGWalkColumn> columns;
	string description;
	// set by the table sink's Finalize: the id a NULL next (or anchor link) is staged as — no key, link or next — and
	// whether any table row has a non-NULL key (without one the CSR holds only a dummy sentinel -> sentinel edge)
	int64_t sentinel = 0;
	bool has_edges = false;
};

//! Keeps the rows of the anchor (table_side false) or of the arm table on the host; the table side's Finalize stages
//! its rows as edges key -> next and builds the CSR into the slot
class PhysicalGGWalkRowSink : public PhysicalOperator {
public:
	PhysicalGGWalkRowSink(shared_ptr<GGWalkInput> input, shared_ptr<GGGraphSlot> slot, bool table_side,
	                      vector<LogicalType> types, idx_t estimated_cardinality);
	shared_ptr<GGWalkInput> input;
	shared_ptr<GGGraphSlot> slot;
	bool table_side;

public:
	unique_ptr<GlobalSinkState> GetGlobalSinkState(ClientContext &context) const override;
	SinkResultType Sink(ExecutionContext &context, GlobalSinkState &gstate, LocalSinkState &lstate,
	                    DataChunk &input) const override;
	SinkFinalizeType Finalize(Pipeline &pipeline, Event &event, ClientContext &context,
	                          GlobalSinkState &gstate) const override;
	bool IsSink() const override {
		return true;
	}
	bool ParallelSink() const override {
		return true;
	}
	string GetName() const override;
};

//! Source: the anchor's rows, then every walk of the closure (gg_walk_closure) level by level, its columns gathered
//! from its seed's anchor row and its last edge's table row
class PhysicalGGRecursiveWalks : public PhysicalOperator {
public:
	PhysicalGGRecursiveWalks(vector<LogicalType> types, shared_ptr<GGGraph> graph, shared_ptr<GGWalkInput> input,
	                         idx_t estimated_cardinality);
	shared_ptr<GGGraph> graph;
	shared_ptr<GGWalkInput> input;

public:
	unique_ptr<GlobalSourceState> GetGlobalSourceState(ClientContext &context) const override;
	void GetData(ExecutionContext &context, DataChunk &chunk, GlobalSourceState &gstate,
	             LocalSourceState &lstate) const override;
	bool IsSource() const override {
		return true;
	}
	string GetName() const override {
		return "GG_RECURSIVE_WALKS";
	}
	string ParamsToString() const override;
};

//===--------------------------------------------------------------------===//
// UNION recursion over one keyed table (gg_recursive_reach.cpp, rule: PlanRecursiveWalks in gg_plan_rule.cpp under
// PRAGMA enable_gpu_recursive_union).  The same sinks and GGWalkInput; every column is CARRIED, CONSTANT or, at the
// link's position, the TABLE's next column.
//===--------------------------------------------------------------------===//
//! Source: the distinct anchor rows, then every new (carried columns, next, constants) row of the reachability closure
//! (gg_reach_closure) level by level
class PhysicalGGRecursiveReach : public PhysicalOperator {
public:
	PhysicalGGRecursiveReach(vector<LogicalType> types, shared_ptr<GGGraph> graph, shared_ptr<GGWalkInput> input,
	                         idx_t estimated_cardinality);
	shared_ptr<GGGraph> graph;
	shared_ptr<GGWalkInput> input;

public:
	unique_ptr<GlobalSourceState> GetGlobalSourceState(ClientContext &context) const override;
	void GetData(ExecutionContext &context, DataChunk &chunk, GlobalSourceState &gstate,
	             LocalSourceState &lstate) const override;
	bool IsSource() const override {
		return true;
	}
	string GetName() const override {
		return "GG_RECURSIVE_REACH";
	}
	string ParamsToString() const override;
};

//===--------------------------------------------------------------------===//
// UNION recursion with a depth counter over one keyed table (gg_recursive_levels.cpp, rule: PlanRecursiveWalks in
// gg_plan_rule.cpp under PRAGMA enable_gpu_recursive_levels).  The same sinks and GGWalkInput; every column is CARRIED,
// CONSTANT, a COUNTER or, at the link's position, the TABLE's next column.
//===--------------------------------------------------------------------===//
//! Source: the distinct anchor rows, then level by level the members of the level sets (gg_level_sets) as (carried
//! columns, next, constants, start + step x level)
class PhysicalGGRecursiveLevels : public PhysicalOperator {
public:
	PhysicalGGRecursiveLevels(vector<LogicalType> types, shared_ptr<GGGraph> graph, shared_ptr<GGWalkInput> input,
	                          idx_t estimated_cardinality);
	shared_ptr<GGGraph> graph;
	shared_ptr<GGWalkInput> input;

public:
	unique_ptr<GlobalSourceState> GetGlobalSourceState(ClientContext &context) const override;
	void GetData(ExecutionContext &context, DataChunk &chunk, GlobalSourceState &gstate,
	             LocalSourceState &lstate) const override;
	bool IsSource() const override {
		return true;
	}
	string GetName() const override {
		return "GG_RECURSIVE_LEVELS";
	}
	string ParamsToString() const override;
};

//! what GG_RECURSIVE_REACH and GG_RECURSIVE_LEVELS share (gg_recursive_reach.cpp), rows compared as the reference's
//! hash table compares them (NULL equal to NULL):
//! the distinct rows of `rows`, in their first occurrence's order
void GGDistinctRows(ClientContext &context, ChunkCollection &rows, const vector<LogicalType> &types,
                    ChunkCollection &distinct);
//! row_class[r]: the class of row r, classes being the distinct values of the columns `carried` numbered in order of
//! appearance (none carried: one class); class_row[c]: the first row of class c
void GGRowClasses(ClientContext &context, ChunkCollection &rows, const vector<idx_t> &carried,
                  const vector<LogicalType> &carried_types, vector<uint32_t> &row_class, vector<idx_t> &class_row);
//! every (class, vertex id) row of a device result and its rows per level, through its levels / fetch calls
typedef int (*GGPairLevelsFn)(const gg_result *, uint64_t *, int, int *);
typedef int (*GGPairFetchFn)(const gg_result *, uint64_t, uint32_t, int64_t *, int64_t *, int32_t *, uint32_t *);
void GGFetchPairRows(gg_result *res, GGPairLevelsFn levels_fn, GGPairFetchFn fetch_fn, const char *what,
                     vector<int64_t> &row_class, vector<int64_t> &vertex, vector<uint64_t> &per_level);
//! target[i] = vertex[i] cast to the target's type, the sentinel as NULL, i < n
void GGLinkColumn(const int64_t *vertex, idx_t n, int64_t sentinel, Vector &target);

//! column `col` of every row of `rows` as int64 (NULL: valid[r] = false) (gg_recursive_walks.cpp)
void GGIntegerColumn(ChunkCollection &rows, idx_t col, vector<int64_t> &out, vector<bool> &valid);
//! target[i] = column `col` of row row[i] of `rows`, i < n (gg_recursive_walks.cpp)
void GGGatherRows(ChunkCollection &rows, idx_t col, const idx_t *row, idx_t n, Vector &target);

//! true if a plan over `spec` can read its tables through pipeline sinks: the BuildPipelines rule is registered with
//! the shim, every source is a plain table, and the connection did not ask for pinned graphs
bool GGPipelineSinksAvailable(ClientContext &context, const GGGraphSpec &spec);
//! GG_<name> scan with the sinks (and the reference's own table scans) of `spec` as children
unique_ptr<PhysicalOperator> GGMakeGraphScan(const GGGraphSpec &spec, vector<LogicalType> types, string name,
                                             string description, bool parallel_result,
                                             PhysicalGGGraphScan::Factory factory, idx_t estimated_cardinality);
//! the same for a plan whose graph takes several edge-table passes: one sink child per entry, in build order
struct GGSinkSpec {
	GGScanSource rows;
	PhysicalGGLazySink::EdgeOptions options;
};
unique_ptr<PhysicalOperator> GGMakeGraphScan(const vector<GGSinkSpec> &sinks, vector<LogicalType> types, string name,
                                             string description, bool parallel_result,
                                             PhysicalGGGraphScan::Factory factory, idx_t estimated_cardinality);
//! PhysicalTableScan of the given columns of a base table (what plan_get.cpp:47-60 builds for a seq_scan)
unique_ptr<PhysicalOperator> GGBaseTableScan(const GGScanSource &source);
void GGRegisterPipelineRule();
//! the hosting reference has the BuildPipelines case itself (oracle/callout.patch): pipeline sinks without a rule
void GGPipelineSinksNative();
//! every graph scan below `plan` keeps its graph for as long as the plan lives (plans with a recursive CTE)
void GGKeepGraphs(PhysicalOperator &plan);

} // namespace duckdb

extern "C" int gg_pipeline_rule_registered();
