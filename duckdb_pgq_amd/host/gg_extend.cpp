// gg_extend.cpp — walk rows joined with the rows of a second keyed table on one of their columns, as two table functions:
//
//   gg_khop_extend(vertex_table, vertex_key, edge_table, src_col, dst_col, sources_sql VARCHAR, hops BIGINT,
//                  ext_table VARCHAR, ext_key_col VARCHAR, ext_next_col VARCHAR, from_col BIGINT)
//        -> (v0 BIGINT, ..., v{hops} BIGINT, w BIGINT, ext_rowid BIGINT)  one row per row of ext_table that joins a walk
//   gg_khop_extend_count(same arguments)
//        -> (rows BIGINT, walks BIGINT, matched BIGINT)                   one row: rows out, walks looked at, walks that join
//
// The `hops`-hop walks over edge_table from the ids `sources_sql` yields (one integer column; NULL or '': from every
// vertex) are joined with ext_table on v{from_col} = ext_key_col; w is the row's ext_next_col and ext_rowid its rowid, by
// which the statement above fetches the row's other columns.  What that stands for in the reference: the next hash join
// of a chain when its build table is a different one — `knows k, message m WHERE m.m_creatorid = k.k_person2id`
// (benchmark/ldbc/queries/interactive-complex-2.sql:2-7; hops = 1, from_col = 1), friends and friends of friends and their
// messages (interactive-complex-9.sql:13-15; hops = 2, from_col = 2), forum_person joined on a middle column
// (interactive-complex-5.sql:15) — PhysicalHashJoin::Execute -> JoinHashTable::Probe + ScanStructure::NextInnerJoin with
// the payload gathered by row in ScanStructure::GatherResult (src/execution/join_hashtable.cpp:304-476).  No planner rule
// recognises these shapes.
//
// Every statement builds a graph of its own: the walk CSR as gg_khop_edge_filter builds it, then — on the same device
// context — the CSR of ext_table with its rowids, over the staged vertex ids united with the distinct endpoints of
// ext_table (PhysicalGGEdgeSink as_filter + derive_vertices + keep_vertices into GGGraph::filter_csr, the way
// ConnectedSegments holds its second CSR): no row of ext_table is dropped, and an id that is both a vertex and an
// endpoint of ext_table is one vertex.  A pinned graph is never used: a second CSR is not hung on a graph other
// statements share.  The walk table is expanded on the device, extended there (gg_result_extend_edge, include/gg.h) and
// dropped before the first row leaves; the longer rows stay on the device and the pipeline's threads drain them together.
#include "gg_table_function.hpp"

namespace duckdb {

namespace {

//! Source: the `hops`-hop walks from the sources joined with the rows of a second edge table (GGGraph::filter_csr, built
//! with rowids) whose key is column from_col of the walk.
//! Output: (v0 BIGINT, ..., v{hops} BIGINT, w BIGINT, ext_rowid BIGINT); count_only: the one row (rows BIGINT, walks
//! BIGINT, matched BIGINT).
class PhysicalGGExtend : public GGWalkSource {
public:
	PhysicalGGExtend(shared_ptr<GGGraph> graph_p, int hops_p, vector<int64_t> sources_p, bool all_sources_p, int from_col_p,
	                 bool count_only_p)
	    : GGWalkSource(OutputTypes(hops_p, count_only_p), move(graph_p), hops_p, move(sources_p), all_sources_p),
	      from_col(from_col_p), count_only(count_only_p) {
	}
	static vector<LogicalType> OutputTypes(int hops, bool count_only) {
		return vector<LogicalType>(count_only ? 3 : hops + 3, LogicalType::BIGINT);
	}
	typedef GGDrainStateOf<gg_extend_stats> State;

	int from_col;
	bool count_only;

	unique_ptr<GlobalSourceState> GetGlobalSourceState(ClientContext &context) const override {
		auto state = make_unique<State>();
		lock_guard<mutex> guard(graph->lock);
		if (!graph->csr || !graph->filter_csr) {
			throw InternalException("GG_EXTEND scheduled before both CSRs were built");
		}
		state->drain.Replace(context, hops + 1, [&](idx_t &rows) {
			GGResultPtr owner;
			ExpandExtended(from_col, !count_only, !count_only, state->stats, count_only ? nullptr : &owner);
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
			EmitCountRow(gstate, chunk, {gstate.stats.rows_out, gstate.stats.rows_in, gstate.stats.rows_matched});
			return;
		}
		// the slab: the id columns v0..v{hops}, w, then the edge columns e1..e{hops+1}, the last of which is ext_rowid
		auto &slab = (GGResultSlab &)lstate;
		const idx_t ids = (idx_t)hops + 2, edges = (idx_t)hops + 1;
		if (FetchIdsAndEdges(gstate, slab, ids, edges, "gg_khop_extend")) {
			EmitIdsAndRowid(slab, chunk, 0, ids, edges);
		}
	}

	string GetName() const override {
		return "GG_EXTEND";
	}
};

enum { ROWS, COUNT };

unique_ptr<FunctionData> ExtendBind(ClientContext &context, vector<Value> &inputs, vector<LogicalType> &return_types,
                                    vector<string> &names, int kind) {
	const bool count_only = kind == COUNT;
	const GGWalkArguments args(count_only ? "gg_khop_extend_count" : "gg_khop_extend", inputs, GGWalkArguments::EXTENSION,
	                           {6, 7, 8, 9, 10}, "hops, ext_table, ext_key_col, ext_next_col and from_col");
	auto data = make_unique<GGFunctionData>();
	data->open = [=](ClientContext &ctx, GGOpened &opened) {
		opened.graph = args.BuildGraph(ctx);
		opened.source = make_unique<PhysicalGGExtend>(opened.graph, (int)args.hops, args.Sources(ctx), args.AllSources(),
		                                              (int)args.from_col, count_only);
	};
	data->parallel_result = !count_only;
	data->description = args.Describe();
	return_types = PhysicalGGExtend::OutputTypes((int)args.hops, count_only);
	if (count_only) {
		names = {"rows", "walks", "matched"};
	} else {
		GGWalkColumnNames(names, args.hops, true);
	}
	return move(data);
}

} // namespace

//! The statement's own graph: the walk CSR over (vertices, edges), then the CSR of the joined table with its rowids over
//! the union of the vertex ids and its endpoints, in GGGraph::filter_csr
shared_ptr<GGGraph> GGBuildExtendGraph(ClientContext &context, const GGScanSource &vertices, const GGScanSource &edges,
                                       const GGScanSource &ext) {
	auto graph = make_shared<GGGraph>(0, false, 1); // (the walks carry no edge rowids)
	PhysicalGGVertexSink vsink(graph, {LogicalType::BIGINT}, 0);
	GGRunSinkPipeline(context, vertices, vsink);
	PhysicalGGEdgeSink esink(graph, vector<LogicalType>(2, LogicalType::BIGINT), 0);
	GGRunSinkPipeline(context, edges, esink);
	GGGraph::Check(gg_ctx_set_edge_rowid(graph->ctx, 1), "gg_ctx_set_edge_rowid");
	PhysicalGGEdgeSink xsink(graph, vector<LogicalType>(3, LogicalType::BIGINT), 0, true, true, true);
	GGRunSinkPipeline(context, ext, xsink);
	return graph;
}

void GGRegisterExtendFunctions(ClientContext &context) {
	const auto args = GGWalkArguments::Types(true);
	GGRegisterTableFunctions(context, {GGScanFunction("gg_khop_extend", args, GGBind<ExtendBind, ROWS>),
	                                   GGScanFunction("gg_khop_extend_count", args, GGBind<ExtendBind, COUNT>)});
}

} // namespace duckdb
