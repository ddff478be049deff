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
#include "gg_table_function.hpp"

namespace duckdb {

namespace {

class PhysicalGGExtendGroup : public GGWalkSource {
public:
	PhysicalGGExtendGroup(shared_ptr<GGGraph> graph_p, int hops_p, vector<int64_t> sources_p, bool all_sources_p,
	                      int from_col_p, int key_col_p, uint64_t n_p)
	    : GGWalkSource(OutputTypes(), move(graph_p), hops_p, move(sources_p), all_sources_p), from_col(from_col_p),
	      key_col(key_col_p), n(n_p) {
	}
	static vector<LogicalType> OutputTypes() {
		return vector<LogicalType>(3, LogicalType::BIGINT);
	}
	typedef GGDrainStateOf<gg_top_stats> State; // (max_threads stays 1: the rows leave in rank order)

	int from_col, key_col;
	uint64_t n; // UINT64_MAX: every group

	unique_ptr<GlobalSourceState> GetGlobalSourceState(ClientContext &context) const override {
		auto state = make_unique<State>();
		lock_guard<mutex> guard(graph->lock);
		if (!graph->csr || !graph->filter_csr) {
			throw InternalException("GG_EXTEND_GROUP scheduled before both CSRs were built");
		}
		const int out_hops = hops + 1;
		state->drain.Replace(context, out_hops, [&](idx_t &rows) {
			GGResultPtr owner, groups;
			{
				GGResultPtr extended; // (gone before the groups are ordered, long before a row leaves)
				gg_extend_stats extend_stats {};
				ExpandExtended(from_col, false, true, extend_stats, &extended);
				gg_group_stats group_stats {};
				GGGraph::Check(gg_result_group_by(graph->ctx, extended.get(), out_hops, key_col, graph->filter_csr, -1,
				                                  nullptr, nullptr, &group_stats, GGResultOut(groups)),
				               "gg_result_group_by");
			}
			GGGraph::Check(gg_khop_aggregate_top(graph->ctx, groups.get(), out_hops, GG_TOP_BY_WALKS, 1, n, nullptr, nullptr,
			                                     &state->stats, GGResultOut(owner)),
			               "gg_khop_aggregate_top");
			rows = state->stats.rows_out;
			return owner; // (the groups go back to the pool here: only the top rows stay in HBM)
		});
		return move(state);
	}

	void GetData(ExecutionContext &context, DataChunk &chunk, GlobalSourceState &gstate_p,
	             LocalSourceState &lstate) const override {
		auto &gstate = (State &)gstate_p;
		PollInterrupt(context);
		auto &slab = (GGResultSlab &)lstate;
		auto fetch = [](gg_result *result, int table, idx_t offset, uint32_t want, GGResultSlab &slab) {
			uint32_t got = 0;
			auto columns = slab.Columns(2); // the key's id, its rows (total = rows: not fetched)
			GGGraph::Check(gg_khop_aggregate_fetch(result, table, offset, want, columns[0], (uint64_t *)columns[1], nullptr,
			                                       nullptr, &got),
			               "gg_khop_aggregate_fetch");
			return got;
		};
		if (Refill(gstate, slab, fetch)) {
			EmitRank(gstate, chunk, slab.Emit(chunk, 1, 2));
		}
	}

	string GetName() const override {
		return "GG_EXTEND_GROUP";
	}
};

unique_ptr<FunctionData> ExtendGroupBind(ClientContext &context, vector<Value> &inputs, vector<LogicalType> &return_types,
                                         vector<string> &names, int kind) {
	const GGWalkArguments args("gg_khop_extend_group", inputs, GGWalkArguments::EXTENSION, {6, 7, 8, 9, 10, 11},
	                           "hops, ext_table, ext_key_col, ext_next_col, from_col and key_col");
	const auto key_col = inputs[11].GetValue<int64_t>();
	const bool limited = !inputs[12].is_null;
	const auto n = limited ? inputs[12].GetValue<int64_t>() : 0;
	if (key_col < 0 || key_col > args.hops + 1) {
		throw BinderException(args.fn + ": key_col must lie in 0.." + to_string(args.hops + 1));
	}
	if (n < 0) {
		throw BinderException(args.fn + ": n must not be negative");
	}
	auto data = make_unique<GGFunctionData>();
	data->open = [=](ClientContext &ctx, GGOpened &opened) {
		opened.graph = args.BuildGraph(ctx);
		opened.source = make_unique<PhysicalGGExtendGroup>(opened.graph, (int)args.hops, args.Sources(ctx), args.AllSources(),
		                                                   (int)args.from_col, (int)key_col, limited ? (uint64_t)n : UINT64_MAX);
	};
	data->parallel_result = false; // the rows leave in rank order
	data->description = (limited ? "top " + to_string(n) : string("every group")) + " by count of " + args.Describe() +
	                    ", grouped by column " + to_string(key_col);
	return_types = PhysicalGGExtendGroup::OutputTypes();
	names = {"rank", "key", "rows"};
	return move(data);
}

} // namespace

void GGRegisterGroupFunctions(ClientContext &context) {
	auto args = GGWalkArguments::Types(true);
	args.insert(args.end(), {LogicalType::BIGINT, LogicalType::BIGINT});
	GGRegisterTableFunctions(context, {GGScanFunction("gg_khop_extend_group", args, GGBind<ExtendGroupBind>)});
}

} // namespace duckdb
