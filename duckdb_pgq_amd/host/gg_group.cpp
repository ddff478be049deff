// gg_group.cpp — walk rows joined with a second keyed table, counted per value of one column, as a table function:
//
//   gg_khop_extend_group(vertex_table, vertex_key, edge_table, src_col, dst_col, sources_sql VARCHAR, hops BIGINT,
//                        ext_table VARCHAR, ext_key_col VARCHAR, ext_next_col VARCHAR, from_col BIGINT,
//                        key_col BIGINT, n BIGINT)
//        -> (rank BIGINT, key BIGINT, rows BIGINT)
//
// The rows gg_khop_extend would return (gg_extend.cpp: the `hops`-hop walks from the ids `sources_sql` yields joined with
// ext_table on v{from_col} = ext_key_col) grouped by column key_col in 0..hops + 1 (hops + 1 is w, the row's
// ext_next_col): the first n groups under ORDER BY rows DESC, key — n NULL: every group, ordered.  What that stands for in
// the reference is the end of benchmark/ldbc/queries/interactive-complex-4.sql:1-22 and interactive-complex-6.sql:1-22,
//     SELECT t_name, count(*) FROM knows [, knows], message, message_tag, tag ... GROUP BY t_name ORDER BY 2 DESC, t_name LIMIT 10
// and of interactive-complex-5.sql (by forum): PhysicalTopN (src/execution/operator/order/physical_top_n.cpp:238-293)
// above PhysicalHashAggregate (src/execution/operator/aggregate/physical_hash_aggregate.cpp:152-266,
// src/execution/aggregate_hashtable.cpp:367-504) fed by the last hash join's ScanStructure::NextInnerJoin
// (src/execution/join_hashtable.cpp:442-476).  Here the walks are expanded, extended (gg_result_extend_edge), grouped
// (gg_result_group_by) and ordered (gg_khop_aggregate_top, GG_TOP_BY_WALKS descending) on the device, the walk table and the
// extended table are dropped before the first row leaves, and only the n rows of the answer are drained — by one thread,
// in rank order.  The graph is gg_khop_extend's (GGBuildExtendGraph: the walk CSR and GGGraph::filter_csr, never a pinned
// graph); filter_csr's vertex set is the persons united with ext_table's endpoints, so it is the key's table for every
// column.  No planner rule recognises the shape.
#include "duckdb.hpp"
#include "duckdb/catalog/catalog.hpp"
#include "duckdb/common/exception.hpp"
#include "duckdb/main/client_context.hpp"
#include "duckdb/parser/parsed_data/create_table_function_info.hpp"

#include "gg_extension.hpp"
#include "gg_operators.hpp"

namespace duckdb {

namespace {

class GroupState : public GlobalSourceState {
public:
	idx_t MaxThreads() override {
		return 1; // the rows leave in rank order
	}
	GGResultDrain drain;
	idx_t next_rank = 0;
};

class PhysicalGGExtendGroup : public PhysicalOperator {
public:
	PhysicalGGExtendGroup(shared_ptr<GGGraph> graph_p, int hops_p, vector<int64_t> sources_p, bool all_sources_p,
	                      int from_col_p, int key_col_p, uint64_t n_p)
	    : PhysicalOperator(PhysicalOperatorType::INVALID, OutputTypes(), 0), graph(move(graph_p)), hops(hops_p),
	      sources(move(sources_p)), all_sources(all_sources_p), from_col(from_col_p), key_col(key_col_p), n(n_p) {
	}
	static vector<LogicalType> OutputTypes() {
		return vector<LogicalType>(3, LogicalType::BIGINT);
	}

	shared_ptr<GGGraph> graph;
	int hops;
	vector<int64_t> sources;
	bool all_sources;
	int from_col, key_col;
	uint64_t n; // UINT64_MAX: every group

	unique_ptr<GlobalSourceState> GetGlobalSourceState(ClientContext &context) const override {
		auto state = make_unique<GroupState>();
		lock_guard<mutex> guard(graph->lock);
		if (!graph->csr || !graph->filter_csr) {
			throw InternalException("GG_EXTEND_GROUP scheduled before both CSRs were built");
		}
		static const int64_t none = 0; // an EMPTY list must not arrive as a null pointer (gg.h: null means every vertex)
		const int64_t *ids = all_sources ? nullptr : sources.empty() ? &none : sources.data();
		const int out_hops = hops + 1;
		state->drain.Replace(context, out_hops, [&](idx_t &rows) {
			GGResultPtr owner, groups;
			{
				GGResultPtr walks, extended; // (both gone before the groups are ordered, long before a row leaves)
				gg_khop_stats walk_stats;
				GGGraph::Check(gg_expand_khop_result(graph->ctx, graph->csr, ids, all_sources ? 0 : sources.size(), hops,
				                                     hops, &walk_stats, GGResultOut(walks)),
				               "gg_expand_khop_result");
				gg_extend_stats extend_stats {};
				GGGraph::Check(gg_result_extend_edge(graph->ctx, walks.get(), hops, graph->filter_csr, from_col, 0, 1,
				                                     &extend_stats, GGResultOut(extended)),
				               "gg_result_extend_edge");
				walks.reset();
				gg_group_stats group_stats {};
				GGGraph::Check(gg_result_group_by(graph->ctx, extended.get(), out_hops, key_col, graph->filter_csr, -1,
				                                  nullptr, nullptr, &group_stats, GGResultOut(groups)),
				               "gg_result_group_by");
			}
			gg_top_stats top {};
			GGGraph::Check(gg_khop_aggregate_top(graph->ctx, groups.get(), out_hops, GG_TOP_BY_WALKS, 1, n, nullptr, nullptr,
			                                     &top, GGResultOut(owner)),
			               "gg_khop_aggregate_top");
			rows = top.rows_out;
			return owner; // (the groups go back to the pool here: only the top rows stay in HBM)
		});
		return move(state);
	}

	unique_ptr<LocalSourceState> GetLocalSourceState(ExecutionContext &context, GlobalSourceState &gstate) const override {
		return make_unique<GGResultSlab>(graph);
	}

	void GetData(ExecutionContext &context, DataChunk &chunk, GlobalSourceState &gstate_p,
	             LocalSourceState &lstate) const override {
		auto &gstate = (GroupState &)gstate_p;
		if (context.client.interrupted) {
			throw InterruptException();
		}
		auto &slab = (GGResultSlab &)lstate;
		if (slab.pos >= slab.rows) {
			auto fetch = [](gg_result *result, int table, idx_t offset, uint32_t want, GGResultSlab &slab) {
				uint32_t got = 0;
				auto columns = slab.Columns(2); // the key's id, its rows (total = rows: not fetched)
				GGGraph::Check(gg_khop_aggregate_fetch(result, table, offset, want, columns[0], (uint64_t *)columns[1],
				                                       nullptr, nullptr, &got),
				               "gg_khop_aggregate_fetch");
				return got;
			};
			if (!gstate.drain.Refill(slab, [] { return false; }, fetch)) {
				return;
			}
		}
		const idx_t count = slab.Emit(chunk, 1, 2);
		auto rank = FlatVector::GetData<int64_t>(chunk.data[0]);
		for (idx_t i = 0; i < count; i++) {
			rank[i] = (int64_t)(gstate.next_rank + i); // (one thread: the slabs are claimed and emitted in order)
		}
		gstate.next_rank += count;
	}

	string GetName() const override {
		return "GG_EXTEND_GROUP";
	}
};

} // namespace

static unique_ptr<FunctionData> ExtendGroupBind(ClientContext &context, vector<Value> &inputs,
                                                unordered_map<string, Value> &named_parameters,
                                                vector<LogicalType> &input_table_types, vector<string> &input_table_names,
                                                vector<LogicalType> &return_types, vector<string> &names) {
	const string vertex_table = inputs[0].ToString(), vertex_key = inputs[1].ToString();
	const string edge_table = inputs[2].ToString(), edge_src = inputs[3].ToString(), edge_dst = inputs[4].ToString();
	const string sources_sql = inputs[5].is_null ? string() : inputs[5].ToString();
	for (idx_t i = 6; i <= 11; i++) {
		if (inputs[i].is_null) {
			throw BinderException("gg_khop_extend_group: hops, ext_table, ext_key_col, ext_next_col, from_col and key_col "
			                      "must not be NULL");
		}
	}
	const auto hops = inputs[6].GetValue<int64_t>(), from_col = inputs[10].GetValue<int64_t>();
	const auto key_col = inputs[11].GetValue<int64_t>();
	const string ext_table = inputs[7].ToString(), ext_key = inputs[8].ToString(), ext_next = inputs[9].ToString();
	const bool limited = !inputs[12].is_null;
	const auto n = limited ? inputs[12].GetValue<int64_t>() : 0;
	if (hops < 1 || hops + 1 > GG_MAX_HOPS) {
		throw BinderException("gg_khop_extend_group: need 1 <= hops <= " + to_string(GG_MAX_HOPS - 1));
	}
	if (from_col < 0 || from_col > hops) {
		throw BinderException("gg_khop_extend_group: from_col must lie in 0.." + to_string(hops));
	}
	if (key_col < 0 || key_col > hops + 1) {
		throw BinderException("gg_khop_extend_group: key_col must lie in 0.." + to_string(hops + 1));
	}
	if (n < 0) {
		throw BinderException("gg_khop_extend_group: n must not be negative");
	}
	auto data = make_unique<GGFunctionData>();
	data->open = [=](ClientContext &ctx, GGOpened &opened) {
		// (tables and columns are resolved at execution time: a missing one raises here)
		opened.graph = GGBuildExtendGraph(ctx, GGTableSource(ctx, vertex_table, {vertex_key}, false),
		                                  GGTableSource(ctx, edge_table, {edge_src, edge_dst}, false),
		                                  GGTableSource(ctx, ext_table, {ext_key, ext_next}, true));
		vector<int64_t> sources;
		if (!sources_sql.empty()) {
			sources = GGQueryInt64Column(ctx, sources_sql, "gg_khop_extend_group: sources");
		}
		opened.source = make_unique<PhysicalGGExtendGroup>(opened.graph, (int)hops, move(sources), sources_sql.empty(),
		                                                   (int)from_col, (int)key_col, limited ? (uint64_t)n : UINT64_MAX);
	};
	data->parallel_result = false; // the rows leave in rank order
	data->description = (limited ? "top " + to_string(n) : string("every group")) + " by count of " + to_string(hops) +
	                    "-hop walks of " + edge_table + " joined with " + ext_table + " on v" + to_string(from_col) + " = " +
	                    ext_key + ", grouped by column " + to_string(key_col);
	return_types = PhysicalGGExtendGroup::OutputTypes();
	names = {"rank", "key", "rows"};
	return move(data);
}

void GGRegisterGroupFunctions(ClientContext &context) {
	const vector<LogicalType> args = {LogicalType::VARCHAR, LogicalType::VARCHAR, LogicalType::VARCHAR,
	                                  LogicalType::VARCHAR, LogicalType::VARCHAR, LogicalType::VARCHAR,
	                                  LogicalType::BIGINT,  LogicalType::VARCHAR, LogicalType::VARCHAR,
	                                  LogicalType::VARCHAR, LogicalType::BIGINT,  LogicalType::BIGINT,
	                                  LogicalType::BIGINT};
	auto fn = GGScanFunction("gg_khop_extend_group", args, ExtendGroupBind);
	CreateTableFunctionInfo info(fn);
	Catalog::GetCatalog(context).CreateTableFunction(context, &info);
}

} // namespace duckdb
