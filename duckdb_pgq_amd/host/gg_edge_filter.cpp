// gg_edge_filter.cpp — walk rows filtered by an edge between two of their columns, as two table functions:
//
//   gg_khop_edge_filter(vertex_table, vertex_key, edge_table, src_col, dst_col,
//                       sources_sql VARCHAR, hops BIGINT, from_col BIGINT, to_col BIGINT, mode VARCHAR)
//        -> (v0 BIGINT, ..., v{hops} BIGINT)                              the surviving walk rows
//   gg_khop_edge_filter_count(same arguments)
//        -> (rows BIGINT, walks BIGINT, matches BIGINT)                   one row: rows out, walks looked at, edge rows matched
//
// The `hops`-hop walks from the ids `sources_sql` yields (one integer column; NULL or '': from every vertex) are kept by
// the number m of rows of edge_table that lead from column from_col to column to_col of the walk: mode 'inner' gives m
// copies of the row, 'semi' the row if m > 0, 'anti' the row if m = 0.  What that stands for in the reference:
//   'inner'  the last hash join of a chain when it carries two conditions — `k4.dst = k1.src` closes a 4-walk —
//            PhysicalHashJoin::Execute -> JoinHashTable::Probe + ScanStructure::NextInnerJoin
//            (src/execution/join_hashtable.cpp:304-476).  Closed walks of k edges through a set of persons:
//            hops = k - 1, from_col = k - 1, to_col = 0.
//   'anti'   NOT EXISTS (SELECT * FROM knows WHERE k_person1id = C AND k_person2id = k2.k_person2id), "friends of friends
//            who are not friends" (benchmark/ldbc/queries/interactive-complex-10.sql:19-24): ScanKeyMatches + NextAntiJoin
//            (join_hashtable.cpp:478-540) — hops = 2, from_col = 0, to_col = 2; `k2.dst <> C` stays a predicate on v2
//            above the function.
//   'semi'   EXISTS (...) (interactive-complex-7.sql:5, interactive-short-7.sql:3): NextSemiJoin (join_hashtable.cpp:522).
// The condition is asked of the same edge table the walks are formed over (one graph; the two-graph form is the C-ABI's,
// gg_result_filter_edge in include/gg.h).  No planner rule recognises these shapes.
//
// The graph comes from GGBuildGraph — or is the pinned graph of these tables if the connection asked for pinned graphs.
// The walk table is expanded on the device, filtered there and dropped before the first row leaves; the surviving rows
// stay on the device and the pipeline's threads drain them together (GGResultDrain, gg_operators.hpp).
#include "duckdb.hpp"
#include "duckdb/catalog/catalog.hpp"
#include "duckdb/common/exception.hpp"
#include "duckdb/main/client_context.hpp"
#include "duckdb/parser/parsed_data/create_table_function_info.hpp"

#include "gg_extension.hpp"
#include "gg_operators.hpp"

namespace duckdb {

namespace {

class EdgeFilterState : public GlobalSourceState {
public:
	idx_t MaxThreads() override {
		return max_threads;
	}
	gg_edge_filter_stats stats {};
	GGResultDrain drain;  // the rows (count_only: none)
	bool counted = false; // count_only: the one row went out (under drain.lock)
	idx_t max_threads = 1;
};

} // namespace

PhysicalGGEdgeFilter::PhysicalGGEdgeFilter(shared_ptr<GGGraph> graph_p, int hops_p, vector<int64_t> sources_p,
                                           bool all_sources_p, int from_col_p, int to_col_p, int mode_p, bool count_only_p,
                                           idx_t estimated_cardinality)
    : PhysicalOperator(PhysicalOperatorType::INVALID, OutputTypes(hops_p, count_only_p), estimated_cardinality),
      graph(move(graph_p)), hops(hops_p), sources(move(sources_p)), all_sources(all_sources_p), from_col(from_col_p),
      to_col(to_col_p), mode(mode_p), count_only(count_only_p) {
}

vector<LogicalType> PhysicalGGEdgeFilter::OutputTypes(int hops, bool count_only) {
	return vector<LogicalType>(count_only ? 3 : hops + 1, LogicalType::BIGINT);
}

unique_ptr<GlobalSourceState> PhysicalGGEdgeFilter::GetGlobalSourceState(ClientContext &context) const {
	auto state = make_unique<EdgeFilterState>();
	lock_guard<mutex> guard(graph->lock);
	if (!graph->csr) {
		throw InternalException("GG_EDGE_FILTER scheduled before the CSR was built");
	}
	static const int64_t none = 0; // an EMPTY list must not arrive as a null pointer (gg.h: null means every vertex)
	const int64_t *ids = all_sources ? nullptr : sources.empty() ? &none : sources.data();
	state->drain.Replace(context, hops, [&](idx_t &rows) {
		GGResultPtr owner;
		gg_khop_stats walk_stats;
		GGResultPtr walks; // (gone once filtered: dropped before the rows drain)
		GGGraph::Check(gg_expand_khop_result(graph->ctx, graph->csr, ids, all_sources ? 0 : sources.size(), hops, hops,
		                                     &walk_stats, GGResultOut(walks)),
		               "gg_expand_khop_result");
		GGGraph::Check(gg_result_filter_edge(graph->ctx, walks.get(), hops, graph->csr, from_col, to_col, mode,
		                                     count_only ? 0 : 1, &state->stats,
		                                     count_only ? nullptr : static_cast<gg_result **>(GGResultOut(owner))),
		               "gg_result_filter_edge");
		rows = count_only ? 0 : state->stats.rows_out;
		return owner;
	});
	state->max_threads = GGResultSlab::ThreadsFor(count_only ? 0 : state->stats.rows_out);
	return move(state);
}

unique_ptr<LocalSourceState> PhysicalGGEdgeFilter::GetLocalSourceState(ExecutionContext &context,
                                                                       GlobalSourceState &gstate) const {
	return make_unique<GGResultSlab>(graph);
}

void PhysicalGGEdgeFilter::GetData(ExecutionContext &context, DataChunk &chunk, GlobalSourceState &gstate_p,
                                   LocalSourceState &lstate) const {
	auto &gstate = (EdgeFilterState &)gstate_p;
	if (context.client.interrupted) {
		throw InterruptException();
	}
	if (count_only) {
		lock_guard<mutex> guard(gstate.drain.lock);
		if (gstate.counted) {
			return;
		}
		gstate.counted = true;
		FlatVector::GetData<int64_t>(chunk.data[0])[0] = (int64_t)gstate.stats.rows_out;
		FlatVector::GetData<int64_t>(chunk.data[1])[0] = (int64_t)gstate.stats.rows_in;
		FlatVector::GetData<int64_t>(chunk.data[2])[0] = (int64_t)gstate.stats.matches;
		chunk.SetCardinality(1);
		return;
	}
	auto &slab = (GGResultSlab &)lstate;
	const idx_t columns = (idx_t)hops + 1;
	if (slab.pos >= slab.rows) {
		auto fetch = [columns](gg_result *result, int table, idx_t offset, uint32_t want, GGResultSlab &slab) {
			uint32_t got = 0;
			GGGraph::Check(gg_result_fetch(result, table, offset, want, slab.Columns(columns), &got), "gg_result_fetch");
			return got;
		};
		if (!gstate.drain.Refill(slab, [] { return false; }, fetch)) { // (one table: nothing to advance to)
			return;
		}
	}
	slab.Emit(chunk, 0, columns);
}

static unique_ptr<FunctionData> EdgeFilterBindInternal(vector<Value> &inputs, vector<LogicalType> &return_types,
                                                       vector<string> &names, bool count_only) {
	const char *fn = count_only ? "gg_khop_edge_filter_count" : "gg_khop_edge_filter";
	const string vertex_table = inputs[0].ToString(), vertex_key = inputs[1].ToString();
	const string edge_table = inputs[2].ToString(), edge_src = inputs[3].ToString(), edge_dst = inputs[4].ToString();
	const string sources_sql = inputs[5].is_null ? string() : inputs[5].ToString();
	for (idx_t i = 6; i <= 9; i++) {
		if (inputs[i].is_null) {
			throw BinderException(string(fn) + ": hops, from_col, to_col and mode must not be NULL");
		}
	}
	const auto hops = inputs[6].GetValue<int64_t>(), from_col = inputs[7].GetValue<int64_t>(),
	           to_col = inputs[8].GetValue<int64_t>();
	const string mode_name = inputs[9].ToString();
	if (hops < 1 || hops > GG_MAX_HOPS) {
		throw BinderException(string(fn) + ": need 1 <= hops <= " + to_string(GG_MAX_HOPS));
	}
	if (from_col < 0 || from_col > hops || to_col < 0 || to_col > hops) {
		throw BinderException(string(fn) + ": from_col and to_col must lie in 0.." + to_string(hops));
	}
	int mode;
	if (mode_name == "inner") {
		mode = GG_EDGE_INNER;
	} else if (mode_name == "semi") {
		mode = GG_EDGE_SEMI;
	} else if (mode_name == "anti") {
		mode = GG_EDGE_ANTI;
	} else {
		throw BinderException(string(fn) + ": mode '" + mode_name + "' (one of 'inner', 'semi', 'anti')");
	}
	auto data = make_unique<GGFunctionData>();
	data->open = [=](ClientContext &ctx, GGOpened &opened) {
		GGGraphSpec spec; // (tables and columns are resolved at execution time: a missing one raises here)
		spec.vertices = GGTableSource(ctx, vertex_table, {vertex_key}, false);
		spec.edges = GGTableSource(ctx, edge_table, {edge_src, edge_dst}, false);
		opened.graph = GGBuildGraph(ctx, spec);
		vector<int64_t> sources;
		if (!sources_sql.empty()) {
			sources = GGQueryInt64Column(ctx, sources_sql, count_only ? "gg_khop_edge_filter_count: sources"
			                                                          : "gg_khop_edge_filter: sources");
		}
		opened.source = make_unique<PhysicalGGEdgeFilter>(opened.graph, (int)hops, move(sources), sources_sql.empty(),
		                                                  (int)from_col, (int)to_col, mode, count_only, 0);
	};
	data->parallel_result = !count_only;
	data->description = mode_name + " edge v" + to_string(from_col) + " -> v" + to_string(to_col) + " over " +
	                    to_string(hops) + "-hop walks of " + edge_table;
	return_types = PhysicalGGEdgeFilter::OutputTypes((int)hops, count_only);
	if (count_only) {
		names = {"rows", "walks", "matches"};
	} else {
		for (int64_t c = 0; c <= hops; c++) {
			names.push_back("v" + to_string(c));
		}
	}
	return move(data);
}

static unique_ptr<FunctionData> EdgeFilterBind(ClientContext &context, vector<Value> &inputs,
                                               unordered_map<string, Value> &named_parameters,
                                               vector<LogicalType> &input_table_types, vector<string> &input_table_names,
                                               vector<LogicalType> &return_types, vector<string> &names) {
	return EdgeFilterBindInternal(inputs, return_types, names, false);
}

static unique_ptr<FunctionData> EdgeFilterCountBind(ClientContext &context, vector<Value> &inputs,
                                                    unordered_map<string, Value> &named_parameters,
                                                    vector<LogicalType> &input_table_types,
                                                    vector<string> &input_table_names, vector<LogicalType> &return_types,
                                                    vector<string> &names) {
	return EdgeFilterBindInternal(inputs, return_types, names, true);
}

void GGRegisterEdgeFilterFunctions(ClientContext &context) {
	const vector<LogicalType> args = {LogicalType::VARCHAR, LogicalType::VARCHAR, LogicalType::VARCHAR,
	                                  LogicalType::VARCHAR, LogicalType::VARCHAR, LogicalType::VARCHAR,
	                                  LogicalType::BIGINT,  LogicalType::BIGINT,  LogicalType::BIGINT,
	                                  LogicalType::VARCHAR};
	auto rows = GGScanFunction("gg_khop_edge_filter", args, EdgeFilterBind);
	auto count = GGScanFunction("gg_khop_edge_filter_count", args, EdgeFilterCountBind);
	CreateTableFunctionInfo rows_info(rows), count_info(count);
	auto &catalog = Catalog::GetCatalog(context);
	catalog.CreateTableFunction(context, &rows_info);
	catalog.CreateTableFunction(context, &count_info);
}

} // namespace duckdb
