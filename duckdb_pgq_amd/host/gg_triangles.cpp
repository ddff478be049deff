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
// (gg_triangles, include/gg.h) and the pipeline's threads drain them together, each through its own page-locked slab
// (GGResultDrain, gg_operators.hpp: one result, one table).
#include "duckdb.hpp"
#include "duckdb/catalog/catalog.hpp"
#include "duckdb/common/exception.hpp"
#include "duckdb/main/client_context.hpp"
#include "duckdb/parser/parsed_data/create_table_function_info.hpp"

#include "gg_extension.hpp"
#include "gg_operators.hpp"

namespace duckdb {

namespace {

class TrianglesState : public GlobalSourceState {
public:
	idx_t MaxThreads() override {
		return max_threads;
	}
	gg_tri_stats stats {};
	GGResultDrain drain;  // the rows (count_only: none)
	bool counted = false; // count_only: the one row went out (under drain.lock)
	idx_t max_threads = 1;
};

} // namespace

PhysicalGGTriangles::PhysicalGGTriangles(shared_ptr<GGGraph> graph_p, bool ordered_p, bool count_only_p,
                                         bool with_edges_p, idx_t estimated_cardinality)
    : PhysicalOperator(PhysicalOperatorType::INVALID, OutputTypes(count_only_p, with_edges_p), estimated_cardinality),
      graph(move(graph_p)), ordered(ordered_p), count_only(count_only_p), with_edges(with_edges_p) {
}

vector<LogicalType> PhysicalGGTriangles::OutputTypes(bool count_only, bool with_edges) {
	return vector<LogicalType>(!count_only && with_edges ? 6 : 3, LogicalType::BIGINT);
}

unique_ptr<GlobalSourceState> PhysicalGGTriangles::GetGlobalSourceState(ClientContext &context) const {
	auto state = make_unique<TrianglesState>();
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

unique_ptr<LocalSourceState> PhysicalGGTriangles::GetLocalSourceState(ExecutionContext &context,
                                                                      GlobalSourceState &gstate) const {
	return make_unique<GGResultSlab>(graph);
}

void PhysicalGGTriangles::GetData(ExecutionContext &context, DataChunk &chunk, GlobalSourceState &gstate_p,
                                  LocalSourceState &lstate) const {
	auto &gstate = (TrianglesState &)gstate_p;
	if (count_only) {
		lock_guard<mutex> guard(gstate.drain.lock);
		if (gstate.counted) {
			return;
		}
		gstate.counted = true;
		FlatVector::GetData<int64_t>(chunk.data[0])[0] = (int64_t)gstate.stats.rows;
		FlatVector::GetData<int64_t>(chunk.data[1])[0] = (int64_t)gstate.stats.digest;
		FlatVector::GetData<int64_t>(chunk.data[2])[0] = (int64_t)gstate.stats.wedges;
		chunk.SetCardinality(1);
		return;
	}
	if (context.client.interrupted) {
		throw InterruptException();
	}
	auto &slab = (GGResultSlab &)lstate;
	if (slab.pos >= slab.rows) {
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
		if (!gstate.drain.Refill(slab, [] { return false; }, fetch)) { // (one table: nothing to advance to)
			return;
		}
	}
	slab.Emit(chunk, 0, with_edges ? 6 : 3);
}

static unique_ptr<FunctionData> TrianglesBindInternal(vector<Value> &inputs, vector<LogicalType> &return_types,
                                                      vector<string> &names, bool count_only, bool with_edges = false) {
	const string vertex_table = inputs[0].ToString(), vertex_key = inputs[1].ToString();
	const string edge_table = inputs[2].ToString(), edge_src = inputs[3].ToString(), edge_dst = inputs[4].ToString();
	const bool ordered = !inputs[5].is_null && inputs[5].GetValue<bool>();
	auto data = make_unique<GGFunctionData>();
	data->open = [=](ClientContext &ctx, GGOpened &opened) {
		GGGraphSpec spec; // (tables and columns are resolved at execution time: a missing one raises here)
		spec.vertices = GGTableSource(ctx, vertex_table, {vertex_key}, false);
		spec.edges = GGTableSource(ctx, edge_table, {edge_src, edge_dst}, with_edges);
		spec.edges_with_rowid = with_edges;
		opened.graph = with_edges ? GGBuildGraphWithRowids(ctx, spec) : GGBuildGraph(ctx, spec);
		opened.source = make_unique<PhysicalGGTriangles>(opened.graph, ordered, count_only, with_edges, 0);
	};
	data->parallel_result = !count_only;
	data->description = string(ordered ? "ordered " : "") + "triangles of " + edge_table + (with_edges ? " with edge rowids" : "");
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

static unique_ptr<FunctionData> TrianglesBind(ClientContext &context, vector<Value> &inputs,
                                              unordered_map<string, Value> &named_parameters,
                                              vector<LogicalType> &input_table_types, vector<string> &input_table_names,
                                              vector<LogicalType> &return_types, vector<string> &names) {
	return TrianglesBindInternal(inputs, return_types, names, false);
}

static unique_ptr<FunctionData> TriangleCountBind(ClientContext &context, vector<Value> &inputs,
                                                  unordered_map<string, Value> &named_parameters,
                                                  vector<LogicalType> &input_table_types,
                                                  vector<string> &input_table_names, vector<LogicalType> &return_types,
                                                  vector<string> &names) {
	return TrianglesBindInternal(inputs, return_types, names, true);
}

static unique_ptr<FunctionData> TriangleEdgesBind(ClientContext &context, vector<Value> &inputs,
                                                  unordered_map<string, Value> &named_parameters,
                                                  vector<LogicalType> &input_table_types,
                                                  vector<string> &input_table_names, vector<LogicalType> &return_types,
                                                  vector<string> &names) {
	return TrianglesBindInternal(inputs, return_types, names, false, true);
}

void GGRegisterTriangleFunctions(ClientContext &context) {
	const vector<LogicalType> args = {LogicalType::VARCHAR, LogicalType::VARCHAR, LogicalType::VARCHAR,
	                                  LogicalType::VARCHAR, LogicalType::VARCHAR, LogicalType::BOOLEAN};
	auto rows = GGScanFunction("gg_triangles", args, TrianglesBind);
	auto count = GGScanFunction("gg_triangle_count", args, TriangleCountBind);
	auto edges = GGScanFunction("gg_triangle_edges", args, TriangleEdgesBind);
	CreateTableFunctionInfo rows_info(rows), count_info(count), edges_info(edges);
	auto &catalog = Catalog::GetCatalog(context);
	catalog.CreateTableFunction(context, &rows_info);
	catalog.CreateTableFunction(context, &count_info);
	catalog.CreateTableFunction(context, &edges_info);
}

} // namespace duckdb
