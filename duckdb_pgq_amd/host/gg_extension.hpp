// gg_extension.hpp — shared between the table functions (gg_duckdb_extension.cpp) and the planner rules
// (gg_plan_rule.cpp) of the loadable extension.
#pragma once

#include <functional>

#include "duckdb/function/table_function.hpp"
#include "gg_operators.hpp"

namespace duckdb {

//! What a gg scan holds while it runs: the device graph, the GG source operator and its state.
struct GGOpened {
	shared_ptr<GGGraph> graph;
	unique_ptr<PhysicalOperator> source;
	unique_ptr<GlobalSourceState> gstate;
};

//! Bind data of every gg table function: a recipe that scans the base tables, builds the graph and
//! creates the source operator.  It runs when the scan is initialised (once per execution, never during
//! EXPLAIN or PREPARE), the point where the reference's hash-join build pipelines would run.
struct GGFunctionData : public TableFunctionData {
	std::function<void(ClientContext &, GGOpened &)> open;
	string description;           // what EXPLAIN prints under the operator name
	bool parallel_result = false; // the result is large: let several pipeline threads drain it
};

//! The table function whose init runs GGFunctionData::open and whose function is the source's GetData.
//! `name` is what EXPLAIN shows for the PhysicalTableScan wrapped around it.
TableFunction GGScanFunction(const string &name, vector<LogicalType> arguments = {},
                             table_function_bind_t bind = nullptr);

class TableCatalogEntry;

//! One base-table scan feeding a sink: either the table's storage read directly — row-group morsels on the
//! reference's worker threads, in the query's own transaction (gg_ingest.cpp) — or, for anything that is
//! not a plain table (views, arbitrary SQL), a statement run on a side connection.
struct GGScanSource {
	TableCatalogEntry *table = nullptr;
	vector<column_t> columns; // table column ids (COLUMN_IDENTIFIER_ROW_ID allowed)
	string sql;               // used when table is null
	bool Empty() const {
		return !table && sql.empty();
	}
};

//! The scans a graph is built from.
struct GGGraphSpec {
	GGScanSource vertices; // key column; empty: vertex set = distinct endpoint ids of the edges
	GGScanSource edges;    // (src, dst[, rowid])
	bool edges_with_rowid = false; // (SQL sources: the statement's third column is the edge's rowid)
	int shards = 1; // > 1: ownership-sharded over that many device contexts (GGGraph::peers)
};

//! Push every row of `source` through `sink` the way a pipeline would: GetGlobalSinkState, Sink per
//! <=1024-row chunk (concurrently for table sources), Combine, Finalize.
void GGRunSinkPipeline(ClientContext &context, const GGScanSource &source, PhysicalOperator &sink);

//! every non-NULL value of a one-column source, through the same ingest path (order unspecified)
vector<int64_t> GGScanInt64Column(ClientContext &context, const GGScanSource &source);

//! (schema.)table resolved in the catalog, or a SQL fallback `SELECT columns FROM name` for views
GGScanSource GGTableSource(ClientContext &context, const string &table_name, const vector<string> &columns,
                           bool with_rowid);
//! Builds the graph — or hands back the pinned one for exactly these tables and columns (gg_graph_pin), if this
//! connection asked for pinned graphs (PRAGMA gg_use_pinned_graphs) and its transaction has changed nothing.
shared_ptr<GGGraph> GGBuildGraph(ClientContext &context, const GGGraphSpec &spec);
//! The graph of `spec` (whose edge source ends in the rowid) built with edge rowids.  A pinned graph carries none and is
//! not used as it is: where this connection would get one for the same tables, its rowid-carrying companion is — built
//! on first use, kept and dropped with the pin.
shared_ptr<GGGraph> GGBuildGraphWithRowids(ClientContext &context, const GGGraphSpec &spec);

//! Per-connection switches (the reference's pragmas act on one ClientContext, client_context.hpp:61-95; so do
//! ours).  Entries die with their connection: they are held by weak_ptr.
struct GGConnectionFlags {
	bool rules = false;        // PRAGMA enable_gpu_graph / disable_gpu_graph
	bool pinned_graphs = false; // PRAGMA gg_use_pinned_graphs / gg_ignore_pinned_graphs
	bool joins = false;         // PRAGMA enable_gpu_joins / disable_gpu_joins: ANY single-key inner join over a table scan
	bool recursive_union = false; // PRAGMA enable_gpu_recursive_union / disable_gpu_recursive_union: UNION recursive CTEs
	                              // over one keyed table (GG_RECURSIVE_REACH; needs enable_gpu_graph too)
	bool recursive_levels = false; // PRAGMA enable_gpu_recursive_levels / disable_gpu_recursive_levels: UNION recursive
	                               // CTEs with a depth counter (GG_RECURSIVE_LEVELS; needs enable_gpu_graph too)
};
GGConnectionFlags GGGetConnectionFlags(ClientContext &context);
void GGSetConnectionFlags(ClientContext &context, const GGConnectionFlags &flags);
//! a statement is about to change `table_oid`: graphs pinned on it are dropped
void GGDropPinsOfTable(idx_t table_oid);

//! first column of `sql` (run on a side connection) as int64, NULLs skipped
vector<int64_t> GGQueryInt64Column(ClientContext &context, const string &sql, const char *what);
//! the two integer columns of `sql` (run on a side connection) as (src, dst) pairs; a row with a NULL is no pair
void GGQueryInt64Pairs(ClientContext &context, const string &sql, const char *what, vector<int64_t> &src,
                       vector<int64_t> &dst);

//! The (key, value) rows of a two-column integer source (TINYINT .. BIGINT; anything else raises, naming `fn` and
//! `value_name`), read through the ingest path in the statement's own transaction, order unspecified.  Rows with a NULL key
//! are skipped; a NULL value is kept as values[i] = 0 with has[i] = 0.  (gg_aggregate.cpp)
struct GGKeyedValues {
	vector<int64_t> keys, values;
	vector<uint8_t> has;
};
GGKeyedValues GGCollectKeyedValues(ClientContext &context, const GGScanSource &source, const string &fn,
                                   const string &value_name);

//! "identifier" with embedded quotes doubled
string GGQuote(const string &ident);

//! gg_triangles.cpp: registers gg_triangles / gg_triangle_count (inside the caller's transaction)
void GGRegisterTriangleFunctions(ClientContext &context);

//! gg_edge_filter.cpp: registers gg_khop_edge_filter / gg_khop_edge_filter_count (inside the caller's transaction)
void GGRegisterEdgeFilterFunctions(ClientContext &context);

//! gg_extend.cpp: registers gg_khop_extend / gg_khop_extend_count (inside the caller's transaction)
void GGRegisterExtendFunctions(ClientContext &context);
//! gg_extend.cpp: the graph of such a statement — the walk CSR over (vertices, edges), then the CSR of the joined table with
//! its rowids over the union of the vertex ids and its endpoints, in GGGraph::filter_csr.  Never a pinned graph.
shared_ptr<GGGraph> GGBuildExtendGraph(ClientContext &context, const GGScanSource &vertices, const GGScanSource &edges,
                                       const GGScanSource &ext);

//! gg_group.cpp: registers gg_khop_extend_group (inside the caller's transaction)
void GGRegisterGroupFunctions(ClientContext &context);

//! gg_value_rows.cpp: registers gg_khop_extend_filter / gg_khop_extend_filter_count / gg_khop_extend_top (inside the caller's
//! transaction)
void GGRegisterValueRowsFunctions(ClientContext &context);

//! gg_distinct.cpp: registers gg_khop_extend_distinct / gg_khop_extend_distinct_count (inside the caller's transaction)
void GGRegisterDistinctFunctions(ClientContext &context);

//! gg_group_tuples.cpp: registers gg_khop_extend_group_columns (inside the caller's transaction)
void GGRegisterGroupTuplesFunctions(ClientContext &context);

//! gg_aggregate.cpp: registers gg_khop_aggregate (inside the caller's transaction)
void GGRegisterAggregateFunctions(ClientContext &context);

//! gg_pair_counts.cpp: registers gg_khop_pair_counts (inside the caller's transaction)
void GGRegisterPairCountFunctions(ClientContext &context);

//! gg_cheapest.cpp: registers gg_cheapest_path and gg_cheapest_path_rows (inside the caller's transaction)
void GGRegisterCheapestFunctions(ClientContext &context);

//! gg_components.cpp: registers gg_components and gg_component_sizes (inside the caller's transaction)
void GGRegisterComponentFunctions(ClientContext &context);

//! gg_plan_rule.cpp: hand the planner rules to the interposition shim if it is loaded; registers
//! `PRAGMA enable_gpu_graph` / `PRAGMA disable_gpu_graph`.
void GGRegisterPlanRules(ClientContext &context);

} // namespace duckdb
