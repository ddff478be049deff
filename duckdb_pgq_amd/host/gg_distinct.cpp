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
// the pipeline's threads drain them together.  SQL gives DISTINCT no order; the rows
// happen to leave in the order of the first walk that holds each.
#include "gg_column_list.hpp"
#include "gg_table_function.hpp"

namespace duckdb {

namespace {

class PhysicalGGDistinct : public GGWalkSource {
public:
	PhysicalGGDistinct(shared_ptr<GGGraph> graph_p, int hops_p, vector<int64_t> sources_p, bool all_sources_p,
	                   bool extended_p, int from_col_p, vector<int> columns_p, bool count_only_p)
	    : GGWalkSource(OutputTypes(columns_p.size(), count_only_p), move(graph_p), hops_p, move(sources_p), all_sources_p),
	      extended(extended_p), from_col(from_col_p), columns(move(columns_p)), count_only(count_only_p) {
	}
	static vector<LogicalType> OutputTypes(idx_t n_columns, bool count_only) {
		return vector<LogicalType>(count_only ? 2 : n_columns, LogicalType::BIGINT);
	}
	typedef GGDrainStateOf<gg_distinct_stats> State;

	bool extended; // the walks are joined with GGGraph::filter_csr first
	int from_col;
	vector<int> columns;
	bool count_only;

	unique_ptr<GlobalSourceState> GetGlobalSourceState(ClientContext &context) const override {
		auto state = make_unique<State>();
		lock_guard<mutex> guard(graph->lock);
		if (!graph->csr || (extended && !graph->filter_csr)) {
			throw InternalException("GG_DISTINCT scheduled before its CSRs were built");
		}
		const int out_table = (int)columns.size() - 1;
		state->drain.Replace(context, out_table, [&](idx_t &rows) {
			GGResultPtr owner;
			{
				GGResultPtr table; // the walk table or the extended one (gone before the rows drain)
				if (extended) {
					gg_extend_stats extend_stats {};
					ExpandExtended(from_col, false, true, extend_stats, &table);
				} else {
					ExpandWalks(table);
				}
				GGGraph::Check(gg_result_distinct(graph->ctx, table.get(), hops + (extended ? 1 : 0), columns.data(),
				                                  (int)columns.size(), count_only ? 0 : 1, &state->stats,
				                                  count_only ? nullptr : static_cast<gg_result **>(GGResultOut(owner))),
				               "gg_result_distinct");
			}
			rows = count_only ? 0 : state->stats.rows_out;
			return owner;
		});
		state->max_threads = GGResultSlab::ThreadsFor(count_only ? 0 : state->stats.rows_out);
		return move(state);
	}

	void GetData(ExecutionContext &context, DataChunk &chunk, GlobalSourceState &gstate_p,
	             LocalSourceState &lstate) const override {
		auto &gstate = (State &)gstate_p;
		PollInterrupt(context);
		if (count_only) {
			EmitCountRow(gstate, chunk, {gstate.stats.rows_out, gstate.stats.rows_in});
			return;
		}
		auto &slab = (GGResultSlab &)lstate;
		if (FetchIds(gstate, slab, columns.size())) {
			slab.Emit(chunk, 0, columns.size());
		}
	}

	string GetName() const override {
		return "GG_DISTINCT";
	}
};

enum { ROWS, COUNT };

unique_ptr<FunctionData> DistinctBind(ClientContext &context, vector<Value> &inputs, vector<LogicalType> &return_types,
                                      vector<string> &names, int kind) {
	const bool count_only = kind == COUNT;
	const GGWalkArguments args(count_only ? "gg_khop_extend_distinct_count" : "gg_khop_extend_distinct", inputs,
	                           GGWalkArguments::OPTIONAL_EXTENSION, {6}, "hops");
	if (inputs[11].is_null) {
		throw InvalidInputException(args.fn + ": columns must not be NULL");
	}
	vector<int> columns;
	string problem;
	if (!GGParseColumnList(inputs[11].ToString(), (int)args.hops + (args.extended ? 1 : 0), columns, problem)) {
		throw InvalidInputException(args.fn + ": columns: " + problem);
	}
	auto data = make_unique<GGFunctionData>();
	data->open = [=](ClientContext &ctx, GGOpened &opened) {
		opened.graph = args.BuildGraph(ctx);
		opened.source = make_unique<PhysicalGGDistinct>(opened.graph, (int)args.hops, args.Sources(ctx), args.AllSources(),
		                                                args.extended, (int)args.from_col, columns, count_only);
	};
	data->parallel_result = !count_only;
	data->description = "distinct columns " + inputs[11].ToString() + " of " + args.Describe();
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

} // namespace

void GGRegisterDistinctFunctions(ClientContext &context) {
	auto args = GGWalkArguments::Types(true);
	args.push_back(LogicalType::VARCHAR);
	GGRegisterTableFunctions(context, {GGScanFunction("gg_khop_extend_distinct", args, GGBind<DistinctBind, ROWS>),
	                                   GGScanFunction("gg_khop_extend_distinct_count", args, GGBind<DistinctBind, COUNT>)});
}

} // namespace duckdb
