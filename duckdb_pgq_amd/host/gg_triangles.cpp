// gg_triangles.cpp — triangle rows (closed 3-edge walks) over one edge table, as three table functions:
//
//   gg_triangle_count(vertex_table, vertex_key, edge_table, src_col, dst_col, ordered BOOLEAN)
//        -> (rows BIGINT, digest BIGINT, wedges BIGINT)                      one row
//   gg_triangles(vertex_table, vertex_key, edge_table, src_col, dst_col, ordered BOOLEAN)
//        -> (v0 BIGINT, v1 BIGINT, v2 BIGINT)                                the rows, order unspecified
//   gg_triangle_edges(vertex_table, vertex_key, edge_table, src_col, dst_col, ordered BOOLEAN)
//        -> (v0, v1, v2, e1 BIGINT, e2 BIGINT, e3 BIGINT)                    the rows with the rowids in edge_table of
//                                                                            v0->v1, v1->v2, v2->v0
//
// What they stand for in the reference: `edge k1, edge k2, edge k3 WHERE k1.dst = k2.src AND k2.dst = k3.src AND
// k3.dst = k1.src` with every endpoint in the vertex table — three hash joins, the last on two conditions
// (PhysicalHashJoin::Execute, src/execution/operator/join/physical_hash_join.cpp:217-254; JoinHashTable::Probe +
// ScanStructure::NextInnerJoin, src/execution/join_hashtable.cpp:304-476).  ordered adds id(v0) < id(v1) < id(v2):
// "Friend triangles", benchmark/ldbc/queries/bi-11.sql:22-33, is
//   gg_triangle_count('persons_of_country', 'personid', 'knows', 'k_person1id', 'k_person2id', true).
// No planner rule recognises the cyclic chain by itself: the reference plans the closing condition as a two-condition
// join or as a filter depending on cardinalities.
//
// gg_triangle_edges is what a late join with the payload of k1, k2, k3 needs (`... t JOIN knows k3 ON k3.rowid = t.e3`):
// the reference gathers build-side columns per match (ScanStructure::GatherResult, src/execution/join_hashtable.cpp:
// 442-476), and parallel edge rows give result rows that are equal as ids.
//
// The graph comes from GGBuildGraph — the sink / finalize machinery of every other scan, without the rowid payload,
// or the pinned graph of these tables if the connection asked for pinned graphs.  gg_triangle_edges scans the edge table
// with its rowid (GGBuildGraphWithRowids: a pinned graph carries none, so its rowid-carrying companion is used, or the
// function builds its own graph).  The rows stay on the device
// (gg_triangles, include/gg.h) and the pipeline's threads drain them together, each through its own page-locked slab.
#include "gg_table_function.hpp"

namespace duckdb {

namespace {

//! Source: the triangle rows (closed 3-edge walks, include/gg.h gg_triangles) of the graph from every vertex.
//! Output: (v0 BIGINT, v1 BIGINT, v2 BIGINT), one row per triple of edge rows v0->v1, v1->v2, v2->v0; ordered: only
//! id(v0) < id(v1) < id(v2).  count_only: the one row (rows BIGINT, digest BIGINT, wedges BIGINT).  with_edges
//! (gg_triangles_edges; the graph carries edge rowids): three more columns (e1 BIGINT, e2 BIGINT, e3 BIGINT), the rowids
//! of those three edge rows.
class PhysicalGGTriangles : public GGResultSource {
public:
	PhysicalGGTriangles(shared_ptr<GGGraph> graph_p, bool ordered_p, bool count_only_p, bool with_edges_p)
	    : GGResultSource(OutputTypes(count_only_p, with_edges_p), move(graph_p)), ordered(ordered_p),
	      count_only(count_only_p), with_edges(with_edges_p) {
	}
	static vector<LogicalType> OutputTypes(bool count_only, bool with_edges) {
		return vector<LogicalType>(!count_only && with_edges ? 6 : 3, LogicalType::BIGINT);
	}
	typedef GGDrainStateOf<gg_tri_stats> State;

	bool ordered;
	bool count_only;
	bool with_edges;

	unique_ptr<GlobalSourceState> GetGlobalSourceState(ClientContext &context) const override {
		auto state = make_unique<State>();
		lock_guard<mutex> guard(graph->lock);
		if (!graph->csr) {
			throw InternalException("GG_TRIANGLES scheduled before the CSR was built");
		}
		state->drain.Replace(context, 2, [&](idx_t &rows) {
			GGResultPtr owner;
			if (with_edges && !count_only) {
				GGGraph::Check(gg_triangles_edges(graph->ctx, graph->csr, nullptr, 0, ordered ? 1 : 0, &state->stats,
				                                  GGResultOut(owner)),
				               "gg_triangles_edges");
			} else {
				GGGraph::Check(gg_triangles(graph->ctx, graph->csr, nullptr, 0, ordered ? 1 : 0, count_only ? 0 : 1,
				                            &state->stats,
				                            count_only ? nullptr : static_cast<gg_result **>(GGResultOut(owner))),
				               "gg_triangles");
			}
			rows = count_only ? 0 : state->stats.rows;
			return owner;
		});
		state->max_threads = GGResultSlab::ThreadsFor(state->stats.rows);
		return move(state);
	}

	void GetData(ExecutionContext &context, DataChunk &chunk, GlobalSourceState &gstate_p,
	             LocalSourceState &lstate) const override {
		auto &gstate = (State &)gstate_p;
		PollInterrupt(context);
		if (count_only) {
			EmitCountRow(gstate, chunk, {gstate.stats.rows, gstate.stats.digest, gstate.stats.wedges});
			return;
		}
		auto &slab = (GGResultSlab &)lstate;
		const bool edges = with_edges;
		auto fetch = [edges](gg_result *result, int table, idx_t offset, uint32_t want, GGResultSlab &slab) {
			uint32_t got = 0, got_edges = 0;
			auto columns = slab.Columns(edges ? 6 : 3);
			GGGraph::Check(gg_result_fetch(result, table, offset, want, columns, &got), "gg_result_fetch");
			if (edges) {
				GGGraph::Check(gg_triangles_fetch_edges(result, offset, want, columns + 3, &got_edges),
				               "gg_triangles_fetch_edges");
				if (got_edges != got) {
					throw InternalException("gg_triangle_edges: id and edge columns of different lengths");
				}
			}
			return got;
		};
		if (Refill(gstate, slab, fetch)) {
			slab.Emit(chunk, 0, with_edges ? 6 : 3);
		}
	}

	string GetName() const override {
		return "GG_TRIANGLES";
	}
};

enum { ROWS, COUNT, EDGES };

unique_ptr<FunctionData> TrianglesBind(ClientContext &context, vector<Value> &inputs, vector<LogicalType> &return_types,
                                       vector<string> &names, int kind) {
	const bool count_only = kind == COUNT, with_edges = kind == EDGES;
	const GraphArguments args(inputs);
	const bool ordered = !inputs[5].is_null && inputs[5].GetValue<bool>();
	auto data = make_unique<GGFunctionData>();
	data->open = [=](ClientContext &ctx, GGOpened &opened) {
		opened.graph = args.Build(ctx, with_edges);
		opened.source = make_unique<PhysicalGGTriangles>(opened.graph, ordered, count_only, with_edges);
	};
	data->parallel_result = !count_only;
	data->description =
	    string(ordered ? "ordered " : "") + "triangles of " + args.edge_table + (with_edges ? " with edge rowids" : "");
	return_types = PhysicalGGTriangles::OutputTypes(count_only, with_edges);
	if (count_only) {
		names = {"rows", "digest", "wedges"};
	} else {
		names = {"v0", "v1", "v2"};
		if (with_edges) {
			names.insert(names.end(), {"e1", "e2", "e3"});
		}
	}
	return move(data);
}

} // namespace

void GGRegisterTriangleFunctions(ClientContext &context) {
	auto args = GraphArguments::Types();
	args.push_back(LogicalType::BOOLEAN);
	GGRegisterTableFunctions(context, {GGScanFunction("gg_triangles", args, GGBind<TrianglesBind, ROWS>),
	                                   GGScanFunction("gg_triangle_count", args, GGBind<TrianglesBind, COUNT>),
	                                   GGScanFunction("gg_triangle_edges", args, GGBind<TrianglesBind, EDGES>)});
}

} // namespace duckdb
