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
// stay on the device and the pipeline's threads drain them together.
#include "gg_table_function.hpp"

namespace duckdb {

namespace {

//! Source: the `hops`-hop walks from the sources, kept by the number m of edge rows that lead from column from_col to
//! column to_col of the walk (gg_result_filter_edge, include/gg.h).
//! Output: (v0 BIGINT, ..., v{hops} BIGINT); count_only: the one row (rows BIGINT, walks BIGINT, matches BIGINT).
class PhysicalGGEdgeFilter : public GGWalkSource {
public:
	PhysicalGGEdgeFilter(shared_ptr<GGGraph> graph_p, int hops_p, vector<int64_t> sources_p, bool all_sources_p,
	                     int from_col_p, int to_col_p, int mode_p, bool count_only_p)
	    : GGWalkSource(OutputTypes(hops_p, count_only_p), move(graph_p), hops_p, move(sources_p), all_sources_p),
	      from_col(from_col_p), to_col(to_col_p), mode(mode_p), count_only(count_only_p) {
	}
	static vector<LogicalType> OutputTypes(int hops, bool count_only) {
		return vector<LogicalType>(count_only ? 3 : hops + 1, LogicalType::BIGINT);
	}
	typedef GGDrainStateOf<gg_edge_filter_stats> State;

	int from_col, to_col;
	int mode; // GG_EDGE_INNER / GG_EDGE_SEMI / GG_EDGE_ANTI
	bool count_only;

	unique_ptr<GlobalSourceState> GetGlobalSourceState(ClientContext &context) const override {
		auto state = make_unique<State>();
		lock_guard<mutex> guard(graph->lock);
		if (!graph->csr) {
			throw InternalException("GG_EDGE_FILTER scheduled before the CSR was built");
		}
		state->drain.Replace(context, hops, [&](idx_t &rows) {
			GGResultPtr owner;
			GGResultPtr walks; // (gone once filtered: dropped before the rows drain)
			ExpandWalks(walks);
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

	void GetData(ExecutionContext &context, DataChunk &chunk, GlobalSourceState &gstate_p,
	             LocalSourceState &lstate) const override {
		auto &gstate = (State &)gstate_p;
		PollInterrupt(context);
		if (count_only) {
			EmitCountRow(gstate, chunk, {gstate.stats.rows_out, gstate.stats.rows_in, gstate.stats.matches});
			return;
		}
		auto &slab = (GGResultSlab &)lstate;
		const idx_t columns = (idx_t)hops + 1;
		if (FetchIds(gstate, slab, columns)) {
			slab.Emit(chunk, 0, columns);
		}
	}

	string GetName() const override {
		return "GG_EDGE_FILTER";
	}
};

enum { ROWS, COUNT };

unique_ptr<FunctionData> EdgeFilterBind(ClientContext &context, vector<Value> &inputs, vector<LogicalType> &return_types,
                                        vector<string> &names, int kind) {
	const bool count_only = kind == COUNT;
	const GGWalkArguments args(count_only ? "gg_khop_edge_filter_count" : "gg_khop_edge_filter", inputs,
	                           GGWalkArguments::NO_EXTENSION, {6, 7, 8, 9}, "hops, from_col, to_col and mode");
	const auto hops = args.hops, from_col = inputs[7].GetValue<int64_t>(), to_col = inputs[8].GetValue<int64_t>();
	const string mode_name = inputs[9].ToString();
	if (from_col < 0 || from_col > hops || to_col < 0 || to_col > hops) {
		throw BinderException(args.fn + ": from_col and to_col must lie in 0.." + to_string(hops));
	}
	int mode;
	if (mode_name == "inner") {
		mode = GG_EDGE_INNER;
	} else if (mode_name == "semi") {
		mode = GG_EDGE_SEMI;
	} else if (mode_name == "anti") {
		mode = GG_EDGE_ANTI;
	} else {
		throw BinderException(args.fn + ": mode '" + mode_name + "' (one of 'inner', 'semi', 'anti')");
	}
	auto data = make_unique<GGFunctionData>();
	data->open = [=](ClientContext &ctx, GGOpened &opened) {
		opened.graph = args.BuildGraph(ctx);
		opened.source = make_unique<PhysicalGGEdgeFilter>(opened.graph, (int)hops, args.Sources(ctx), args.AllSources(),
		                                                  (int)from_col, (int)to_col, mode, count_only);
	};
	data->parallel_result = !count_only;
	data->description = mode_name + " edge v" + to_string(from_col) + " -> v" + to_string(to_col) + " over " + args.Describe();
	return_types = PhysicalGGEdgeFilter::OutputTypes((int)hops, count_only);
	if (count_only) {
		names = {"rows", "walks", "matches"};
	} else {
		GGWalkColumnNames(names, hops);
	}
	return move(data);
}

} // namespace

void GGRegisterEdgeFilterFunctions(ClientContext &context) {
	auto args = GGWalkArguments::Types(false);
	args.insert(args.end(), {LogicalType::BIGINT, LogicalType::BIGINT, LogicalType::VARCHAR});
	GGRegisterTableFunctions(context, {GGScanFunction("gg_khop_edge_filter", args, GGBind<EdgeFilterBind, ROWS>),
	                                   GGScanFunction("gg_khop_edge_filter_count", args, GGBind<EdgeFilterBind, COUNT>)});
}

} // namespace duckdb
