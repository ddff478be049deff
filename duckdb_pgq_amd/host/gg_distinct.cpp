// gg_distinct.cpp — SELECT DISTINCT over chosen columns of walk rows, joined with a second keyed table or not, as two table
// functions over gg_khop_extend's eleven arguments (gg_extend.cpp) and graph (GGBuildExtendGraph) plus `columns VARCHAR`:
//
//   gg_khop_extend_distinct(<gg_khop_extend's 11 arguments>, columns VARCHAR)
//        -> (c0 BIGINT, ..., c{n-1} BIGINT)      the distinct tuples over the listed columns, in the list's order
//   gg_khop_extend_distinct_count(same arguments)
//        -> (rows BIGINT, walks BIGINT)          one row: the distinct tuples, the joined rows looked at
//
// columns is a comma-separated list of column numbers of the joined row (v0, ..., v{hops}, w): 0..hops + 1, pairwise
// different, in the output's order.  A NULL or empty ext_table means no extension: the walk table itself is deduplicated,
// columns ranges over 0..hops, and ext_key_col, ext_next_col and from_col are not looked at — `SELECT DISTINCT
// k2.k_person2id` of benchmark/ldbc/queries/interactive-complex-10.sql:19-24 is hops = 2, columns = '2'.  With an extension,
// columns = '3' over hops = 2 is the set of messages of friends of friends however many walks reach their creator, and
// '0, 3' the (person, message) pairs under the count(DISTINCT m_messageid) of interactive-complex-10.sql:2-9.
// What that stands for in the reference: the hash aggregate without aggregates that SELECT DISTINCT and UNION plan
// (src/execution/physical_plan/plan_distinct.cpp:12-78, physical_hash_aggregate.cpp:152-266) above the join chain.  No
// planner rule recognises these shapes.
// The walk table and the extended table are dropped before the first row leaves; the distinct rows stay on the device and
// the pipeline's threads drain them together (GGResultDrain, gg_operators.hpp).  SQL gives DISTINCT no order; the rows
// happen to leave in the order of the first walk that holds each.
#include "duckdb.hpp"
#include "duckdb/catalog/catalog.hpp"
#include "duckdb/common/exception.hpp"
#include "duckdb/main/client_context.hpp"
#include "duckdb/parser/parsed_data/create_table_function_info.hpp"

#include "gg_column_list.hpp"
#include "gg_extension.hpp"
#include "gg_operators.hpp"

namespace duckdb {

namespace {

class DistinctState : public GlobalSourceState {
public:
	idx_t MaxThreads() override {
		return max_threads;
	}
	gg_distinct_stats stats {};
	GGResultDrain drain;  // the rows (count_only: none)
	bool counted = false; // count_only: the one row went out (under drain.lock)
	idx_t max_threads = 1;
};

class PhysicalGGDistinct : public PhysicalOperator {
public:
	PhysicalGGDistinct(shared_ptr<GGGraph> graph_p, int hops_p, vector<int64_t> sources_p, bool all_sources_p,
	                   bool extended_p, int from_col_p, vector<int> columns_p, bool count_only_p)
	    : PhysicalOperator(PhysicalOperatorType::INVALID, OutputTypes(columns_p.size(), count_only_p), 0),
	      graph(move(graph_p)), hops(hops_p), sources(move(sources_p)), all_sources(all_sources_p), extended(extended_p),
	      from_col(from_col_p), columns(move(columns_p)), count_only(count_only_p) {
	}
	static vector<LogicalType> OutputTypes(idx_t n_columns, bool count_only) {
		return vector<LogicalType>(count_only ? 2 : n_columns, LogicalType::BIGINT);
	}

	shared_ptr<GGGraph> graph;
	int hops;
	vector<int64_t> sources;
	bool all_sources;
	bool extended; // the walks are joined with GGGraph::filter_csr first
	int from_col;
	vector<int> columns;
	bool count_only;

	unique_ptr<GlobalSourceState> GetGlobalSourceState(ClientContext &context) const override {
		auto state = make_unique<DistinctState>();
		lock_guard<mutex> guard(graph->lock);
		if (!graph->csr || (extended && !graph->filter_csr)) {
			throw InternalException("GG_DISTINCT scheduled before its CSRs were built");
		}
		static const int64_t none = 0; // an EMPTY list must not arrive as a null pointer (gg.h: null means every vertex)
		const int64_t *ids = all_sources ? nullptr : sources.empty() ? &none : sources.data();
		const int out_table = (int)columns.size() - 1;
		state->drain.Replace(context, out_table, [&](idx_t &rows) {
			GGResultPtr owner;
			{
				GGResultPtr table; // the walk table, then the extended one (gone before the rows drain)
				int table_hops = hops;
				gg_khop_stats walk_stats;
				GGGraph::Check(gg_expand_khop_result(graph->ctx, graph->csr, ids, all_sources ? 0 : sources.size(), hops, hops,
				                                     &walk_stats, GGResultOut(table)),
				               "gg_expand_khop_result");
				if (extended) {
					GGResultPtr longer;
					gg_extend_stats extend_stats {};
					GGGraph::Check(gg_result_extend_edge(graph->ctx, table.get(), hops, graph->filter_csr, from_col, 0, 1,
					                                     &extend_stats, GGResultOut(longer)),
					               "gg_result_extend_edge");
					table = move(longer);
					table_hops = hops + 1;
				}
				GGGraph::Check(gg_result_distinct(graph->ctx, table.get(), table_hops, columns.data(), (int)columns.size(),
				                                  count_only ? 0 : 1, &state->stats,
				                                  count_only ? nullptr : static_cast<gg_result **>(GGResultOut(owner))),
				               "gg_result_distinct");
			}
			rows = count_only ? 0 : state->stats.rows_out;
			return owner;
		});
		state->max_threads = GGResultSlab::ThreadsFor(count_only ? 0 : state->stats.rows_out);
		return move(state);
	}

	unique_ptr<LocalSourceState> GetLocalSourceState(ExecutionContext &context, GlobalSourceState &gstate) const override {
		return make_unique<GGResultSlab>(graph);
	}

	void GetData(ExecutionContext &context, DataChunk &chunk, GlobalSourceState &gstate_p,
	             LocalSourceState &lstate) const override {
		auto &gstate = (DistinctState &)gstate_p;
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
			chunk.SetCardinality(1);
			return;
		}
		auto &slab = (GGResultSlab &)lstate;
		const idx_t n = columns.size();
		if (slab.pos >= slab.rows) {
			auto fetch = [n](gg_result *result, int table, idx_t offset, uint32_t want, GGResultSlab &slab) {
				uint32_t got = 0;
				GGGraph::Check(gg_result_fetch(result, table, offset, want, slab.Columns(n), &got), "gg_result_fetch");
				return got;
			};
			if (!gstate.drain.Refill(slab, [] { return false; }, fetch)) { // (one table: nothing to advance to)
				return;
			}
		}
		slab.Emit(chunk, 0, n);
	}

	string GetName() const override {
		return "GG_DISTINCT";
	}
};

unique_ptr<FunctionData> DistinctBindInternal(vector<Value> &inputs, vector<LogicalType> &return_types, vector<string> &names,
                                              bool count_only) {
	const string fn = count_only ? "gg_khop_extend_distinct_count" : "gg_khop_extend_distinct";
	const string vertex_table = inputs[0].ToString(), vertex_key = inputs[1].ToString();
	const string edge_table = inputs[2].ToString(), edge_src = inputs[3].ToString(), edge_dst = inputs[4].ToString();
	const string sources_sql = inputs[5].is_null ? string() : inputs[5].ToString();
	if (inputs[6].is_null) {
		throw BinderException(fn + ": hops must not be NULL");
	}
	const auto hops = inputs[6].GetValue<int64_t>();
	const string ext_table = inputs[7].is_null ? string() : inputs[7].ToString();
	const bool extended = !ext_table.empty();
	string ext_key, ext_next;
	int64_t from_col = 0;
	if (extended) {
		for (idx_t i = 8; i <= 10; i++) {
			if (inputs[i].is_null) {
				throw BinderException(fn + ": ext_key_col, ext_next_col and from_col must not be NULL where ext_table is given");
			}
		}
		ext_key = inputs[8].ToString(), ext_next = inputs[9].ToString();
		from_col = inputs[10].GetValue<int64_t>();
	}
	if (hops < 1 || hops + (extended ? 1 : 0) > GG_MAX_HOPS) {
		throw BinderException(fn + ": need 1 <= hops <= " + to_string(GG_MAX_HOPS - (extended ? 1 : 0)));
	}
	if (extended && (from_col < 0 || from_col > hops)) {
		throw BinderException(fn + ": from_col must lie in 0.." + to_string(hops));
	}
	if (inputs[11].is_null) {
		throw InvalidInputException(fn + ": columns must not be NULL");
	}
	vector<int> columns;
	string problem;
	if (!GGParseColumnList(inputs[11].ToString(), (int)hops + (extended ? 1 : 0), columns, problem)) {
		throw InvalidInputException(fn + ": columns: " + problem);
	}
	auto data = make_unique<GGFunctionData>();
	data->open = [=](ClientContext &ctx, GGOpened &opened) {
		// (tables and columns are resolved at execution time: a missing one raises here)
		if (extended) {
			opened.graph = GGBuildExtendGraph(ctx, GGTableSource(ctx, vertex_table, {vertex_key}, false),
			                                  GGTableSource(ctx, edge_table, {edge_src, edge_dst}, false),
			                                  GGTableSource(ctx, ext_table, {ext_key, ext_next}, true));
		} else {
			GGGraphSpec spec;
			spec.vertices = GGTableSource(ctx, vertex_table, {vertex_key}, false);
			spec.edges = GGTableSource(ctx, edge_table, {edge_src, edge_dst}, false);
			opened.graph = GGBuildGraph(ctx, spec);
		}
		vector<int64_t> sources;
		if (!sources_sql.empty()) {
			sources = GGQueryInt64Column(ctx, sources_sql, (fn + ": sources").c_str());
		}
		opened.source = make_unique<PhysicalGGDistinct>(opened.graph, (int)hops, move(sources), sources_sql.empty(), extended,
		                                                (int)from_col, columns, count_only);
	};
	data->parallel_result = !count_only;
	data->description = "distinct columns " + inputs[11].ToString() + " of " + to_string(hops) + "-hop walks of " + edge_table +
	                    (extended ? " joined with " + ext_table + " on v" + to_string(from_col) + " = " + ext_key : string());
	return_types = PhysicalGGDistinct::OutputTypes(columns.size(), count_only);
	if (count_only) {
		names = {"rows", "walks"};
	} else {
		for (idx_t c = 0; c < columns.size(); c++) {
			names.push_back("c" + to_string(c));
		}
	}
	return move(data);
}

template <bool COUNT_ONLY>
unique_ptr<FunctionData> DistinctBind(ClientContext &context, vector<Value> &inputs,
                                      unordered_map<string, Value> &named_parameters, vector<LogicalType> &input_table_types,
                                      vector<string> &input_table_names, vector<LogicalType> &return_types,
                                      vector<string> &names) {
	return DistinctBindInternal(inputs, return_types, names, COUNT_ONLY);
}

} // namespace

void GGRegisterDistinctFunctions(ClientContext &context) {
	const vector<LogicalType> args = {LogicalType::VARCHAR, LogicalType::VARCHAR, LogicalType::VARCHAR, LogicalType::VARCHAR,
	                                  LogicalType::VARCHAR, LogicalType::VARCHAR, LogicalType::BIGINT,  LogicalType::VARCHAR,
	                                  LogicalType::VARCHAR, LogicalType::VARCHAR, LogicalType::BIGINT,  LogicalType::VARCHAR};
	auto rows = GGScanFunction("gg_khop_extend_distinct", args, DistinctBind<false>);
	auto count = GGScanFunction("gg_khop_extend_distinct_count", args, DistinctBind<true>);
	CreateTableFunctionInfo rows_info(rows), count_info(count);
	auto &catalog = Catalog::GetCatalog(context);
	catalog.CreateTableFunction(context, &rows_info);
	catalog.CreateTableFunction(context, &count_info);
}

} // namespace duckdb
