// gg_group_tuples.cpp — GROUP BY several columns of walk rows, joined with a second keyed table or not, with count(*) and
// count / sum / min / max of one integer column, as a table function over gg_khop_extend's eleven arguments
// (gg_extend.cpp) and graph (GGBuildExtendGraph):
//
//   gg_khop_extend_group_columns(<gg_khop_extend's 11 arguments>, columns VARCHAR, value_column VARCHAR, value_of BIGINT)
//        -> (k0 BIGINT, ..., k{n-1} BIGINT, rows BIGINT, valued BIGINT, sum HUGEINT, min BIGINT, max BIGINT)
//
// columns is gg_khop_extend_distinct's argument (gg_column_list.hpp): column numbers of the joined row (v0, ..., v{hops},
// w), pairwise different, in the output's order.  A NULL or empty ext_table groups the walk table itself, as
// gg_khop_extend_distinct deduplicates it.  value_column / value_of are gg_khop_extend_filter's: value_of names the column
// of the joined row whose value is aggregated — for hops + 1 (the column w) value_column is an integer column of ext_table,
// for 0..hops one of vertex_table — and a NULL value gives the vertex no value.  Per group: rows = count(*), valued =
// count(value), and sum, min and max over the valued rows, SQL NULL where valued = 0.  A NULL value_column is the count form:
// no value is looked up, value_of is not looked at, and the value columns are 0, 0, NULL, NULL.
// What that stands for in the reference: PhysicalHashAggregate (physical_hash_aggregate.cpp:152-266) above the join chain —
// `GROUP BY m.friendid, t.t_name` (benchmark/ldbc/queries/bi-10-shortestpath.sql:74), `min(hopCount) ... GROUP BY
// startPerson, friend` (bi-10-shortestpath.sql:28-30), `GROUP BY person1id, person2id` with a summed score (bi-14.sql:111),
// `max(l_creationdate) ... GROUP BY l_personid` (interactive-complex-7.sql:7-12).  No planner rule recognises these shapes
// (DESIGN.md section 7.11).
// The walk table and the extended table are dropped before the first row leaves; the groups stay on the device and the
// pipeline's threads drain them together.  SQL gives GROUP BY no order.
#include "gg_column_list.hpp"
#include "gg_table_function.hpp"

namespace duckdb {

namespace {

class PhysicalGGGroupTuples : public GGWalkSource {
public:
	PhysicalGGGroupTuples(shared_ptr<GGGraph> graph_p, int hops_p, vector<int64_t> sources_p, bool all_sources_p,
	                      bool extended_p, int from_col_p, vector<int> columns_p, int value_of_p, ValueColumn column_p)
	    : GGWalkSource(OutputTypes(columns_p.size()), move(graph_p), hops_p, move(sources_p), all_sources_p),
	      extended(extended_p), from_col(from_col_p), columns(move(columns_p)), value_of(value_of_p), column(move(column_p)) {
	}
	static vector<LogicalType> OutputTypes(idx_t n_columns) {
		vector<LogicalType> types(n_columns + 2, LogicalType::BIGINT); // the keys, rows, valued
		types.insert(types.end(), {LogicalType::HUGEINT, LogicalType::BIGINT, LogicalType::BIGINT});
		return types;
	}
	typedef GGDrainStateOf<gg_group_tuples_stats> State;

	bool extended; // the walks are joined with GGGraph::filter_csr first
	int from_col;
	vector<int> columns;
	int value_of; // -1: the count form
	ValueColumn column;

	unique_ptr<GlobalSourceState> GetGlobalSourceState(ClientContext &context) const override {
		auto state = make_unique<State>();
		lock_guard<mutex> guard(graph->lock);
		if (!graph->csr || (extended && !graph->filter_csr)) {
			throw InternalException("GG_GROUP_TUPLES scheduled before its CSRs were built");
		}
		const int in_hops = hops + (extended ? 1 : 0);
		const bool valued = value_of >= 0;
		const gg_csr *value_csr = !valued ? nullptr : extended && value_of == in_hops ? graph->filter_csr : graph->csr;
		state->drain.Replace(context, 0, [&](idx_t &rows) {
			GGResultPtr owner;
			{
				GGResultPtr table; // the walk table or the extended one (gone before the rows drain)
				if (extended) {
					gg_extend_stats extend_stats {};
					ExpandExtended(from_col, false, true, extend_stats, &table);
				} else {
					ExpandWalks(table);
				}
				GGGraph::Check(gg_result_group_tuples(graph->ctx, table.get(), in_hops, columns.data(), (int)columns.size(),
				                                      value_of, value_csr, valued ? column.values.data() : nullptr,
				                                      valued ? column.valid.data() : nullptr, &state->stats, GGResultOut(owner)),
				               "gg_result_group_tuples");
			}
			rows = state->stats.groups;
			return owner;
		});
		state->max_threads = GGResultSlab::ThreadsFor(state->stats.groups);
		return move(state);
	}

	void GetData(ExecutionContext &context, DataChunk &chunk, GlobalSourceState &gstate_p,
	             LocalSourceState &lstate) const override {
		auto &gstate = (State &)gstate_p;
		PollInterrupt(context);
		auto &slab = (GGResultSlab &)lstate;
		const idx_t keys = columns.size();
		// the slab: the key columns, then rows, valued, sum low, sum high, min, max
		auto fetch = [keys](gg_result *result, int table, idx_t offset, uint32_t want, GGResultSlab &slab) {
			uint32_t got = 0;
			auto c = slab.Columns(keys + 6);
			GGGraph::Check(gg_tuple_groups_fetch(result, offset, want, c, (uint64_t *)c[keys], (uint64_t *)c[keys + 1],
			                                     c[keys + 2], c[keys + 3], c[keys + 4], c[keys + 5], &got),
			               "gg_tuple_groups_fetch");
			return got;
		};
		if (!Refill(gstate, slab, fetch)) {
			return;
		}
		const idx_t at = slab.pos;
		const idx_t n = slab.Emit(chunk, 0, keys + 2);
		auto &sum = chunk.data[keys + 2], &min = chunk.data[keys + 3], &max = chunk.data[keys + 4];
		auto total = FlatVector::GetData<hugeint_t>(sum);
		memcpy(FlatVector::GetData<int64_t>(min), slab.column[keys + 4] + at, n * sizeof(int64_t));
		memcpy(FlatVector::GetData<int64_t>(max), slab.column[keys + 5] + at, n * sizeof(int64_t));
		for (idx_t i = 0; i < n; i++) {
			total[i].lower = (uint64_t)slab.column[keys + 2][at + i];
			total[i].upper = slab.column[keys + 3][at + i];
			if (slab.column[keys + 1][at + i] == 0) { // no valued row: NULL (the count form keeps its sum of 0)
				if (value_of >= 0) {
					FlatVector::SetNull(sum, i, true);
				}
				FlatVector::SetNull(min, i, true);
				FlatVector::SetNull(max, i, true);
			}
		}
	}

	string GetName() const override {
		return "GG_GROUP_TUPLES";
	}
};

unique_ptr<FunctionData> GroupTuplesBind(ClientContext &context, vector<Value> &inputs, vector<LogicalType> &return_types,
                                         vector<string> &names, int kind) {
	const GGWalkArguments args("gg_khop_extend_group_columns", inputs, GGWalkArguments::OPTIONAL_EXTENSION, {6}, "hops");
	if (inputs[11].is_null) {
		throw InvalidInputException(args.fn + ": columns must not be NULL");
	}
	const int max_col = (int)args.hops + (args.extended ? 1 : 0);
	vector<int> columns;
	string problem;
	if (!GGParseColumnList(inputs[11].ToString(), max_col, columns, problem)) {
		throw InvalidInputException(args.fn + ": columns: " + problem);
	}
	const bool valued = !inputs[12].is_null;
	const string value_column = valued ? inputs[12].ToString() : string();
	int64_t value_of = -1;
	if (valued) {
		GGRequireArguments(args.fn, inputs, {13}, "value_of", " where value_column is given");
		value_of = inputs[13].GetValue<int64_t>();
		if (value_of < 0 || value_of > max_col) {
			throw BinderException(args.fn + ": value_of must lie in 0.." + to_string(max_col));
		}
	}
	auto data = make_unique<GGFunctionData>();
	data->open = [=](ClientContext &ctx, GGOpened &opened) {
		opened.graph = args.BuildGraph(ctx);
		auto sources = args.Sources(ctx);
		ValueColumn column;
		if (valued) {
			const bool of_ext = args.extended && value_of == args.hops + 1;
			column = ValuesInVertexOrder(ctx, *opened.graph, of_ext ? opened.graph->filter_csr : opened.graph->csr,
			                             of_ext ? args.ext_table : args.vertex_table, of_ext ? args.ext_next : args.vertex_key,
			                             value_column, args.fn.c_str());
		}
		opened.source = make_unique<PhysicalGGGroupTuples>(opened.graph, (int)args.hops, move(sources), args.AllSources(),
		                                                   args.extended, (int)args.from_col, columns, (int)value_of,
		                                                   move(column));
	};
	data->parallel_result = true;
	data->description = "groups by columns " + inputs[11].ToString() + " of " + args.Describe() +
	                    (valued ? ", " + value_column + " of column " + to_string(value_of) : string(", counted"));
	return_types = PhysicalGGGroupTuples::OutputTypes(columns.size());
	for (idx_t c = 0; c < columns.size(); c++) {
		names.push_back("k" + to_string(c));
	}
	names.insert(names.end(), {"rows", "valued", "sum", "min", "max"});
	return move(data);
}

} // namespace

void GGRegisterGroupTuplesFunctions(ClientContext &context) {
	auto args = GGWalkArguments::Types(true);
	args.insert(args.end(), {LogicalType::VARCHAR, LogicalType::VARCHAR, LogicalType::BIGINT});
	GGRegisterTableFunctions(context, {GGScanFunction("gg_khop_extend_group_columns", args, GGBind<GroupTuplesBind>)});
}

} // namespace duckdb
