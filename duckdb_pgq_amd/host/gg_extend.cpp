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
// dropped before the first row leaves; the longer rows stay on the device and the pipeline's threads drain them together
// (GGResultDrain, gg_operators.hpp).
#include "duckdb.hpp"
#include "duckdb/catalog/catalog.hpp"
#include "duckdb/common/exception.hpp"
#include "duckdb/main/client_context.hpp"
#include "duckdb/parser/parsed_data/create_table_function_info.hpp"

#include "gg_extension.hpp"
#include "gg_operators.hpp"

namespace duckdb {

namespace {

class ExtendState : public GlobalSourceState {
public:
	idx_t MaxThreads() override {
		return max_threads;
	}
	gg_extend_stats stats {};
	GGResultDrain drain;  // the rows (count_only: none)
	bool counted = false; // count_only: the one row went out (under drain.lock)
	idx_t max_threads = 1;
};

} // namespace

PhysicalGGExtend::PhysicalGGExtend(shared_ptr<GGGraph> graph_p, int hops_p, vector<int64_t> sources_p, bool all_sources_p,
                                   int from_col_p, bool count_only_p, idx_t estimated_cardinality)
    : PhysicalOperator(PhysicalOperatorType::INVALID, OutputTypes(hops_p, count_only_p), estimated_cardinality),
      graph(move(graph_p)), hops(hops_p), sources(move(sources_p)), all_sources(all_sources_p), from_col(from_col_p),
      count_only(count_only_p) {
}

vector<LogicalType> PhysicalGGExtend::OutputTypes(int hops, bool count_only) {
	return vector<LogicalType>(count_only ? 3 : hops + 3, LogicalType::BIGINT);
}

unique_ptr<GlobalSourceState> PhysicalGGExtend::GetGlobalSourceState(ClientContext &context) const {
	auto state = make_unique<ExtendState>();
	lock_guard<mutex> guard(graph->lock);
	if (!graph->csr || !graph->filter_csr) {
		throw InternalException("GG_EXTEND scheduled before both CSRs were built");
	}
	static const int64_t none = 0; // an EMPTY list must not arrive as a null pointer (gg.h: null means every vertex)
	const int64_t *ids = all_sources ? nullptr : sources.empty() ? &none : sources.data();
	state->drain.Replace(context, hops + 1, [&](idx_t &rows) {
		GGResultPtr owner;
		gg_khop_stats walk_stats;
		GGResultPtr walks; // (gone once extended: dropped before the rows drain)
		GGGraph::Check(gg_expand_khop_result(graph->ctx, graph->csr, ids, all_sources ? 0 : sources.size(), hops, hops,
		                                     &walk_stats, GGResultOut(walks)),
		               "gg_expand_khop_result");
		GGGraph::Check(gg_result_extend_edge(graph->ctx, walks.get(), hops, graph->filter_csr, from_col,
		                                     count_only ? 0 : 1, count_only ? 0 : 1, &state->stats,
		                                     count_only ? nullptr : static_cast<gg_result **>(GGResultOut(owner))),
		               "gg_result_extend_edge");
		rows = count_only ? 0 : state->stats.rows_out;
		return owner;
	});
	state->max_threads = GGResultSlab::ThreadsFor(count_only ? 0 : state->stats.rows_out);
	return move(state);
}

unique_ptr<LocalSourceState> PhysicalGGExtend::GetLocalSourceState(ExecutionContext &context,
                                                                   GlobalSourceState &gstate) const {
	return make_unique<GGResultSlab>(graph);
}

void PhysicalGGExtend::GetData(ExecutionContext &context, DataChunk &chunk, GlobalSourceState &gstate_p,
                               LocalSourceState &lstate) const {
	auto &gstate = (ExtendState &)gstate_p;
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
		FlatVector::GetData<int64_t>(chunk.data[2])[0] = (int64_t)gstate.stats.rows_matched;
		chunk.SetCardinality(1);
		return;
	}
	auto &slab = (GGResultSlab &)lstate;
	// the slab: the id columns v0..v{hops}, w, then the edge columns e1..e{hops+1} — of which only the last, the joined
	// row's rowid, goes out (the walk carries no edge columns: the others hold -1)
	const idx_t ids = (idx_t)hops + 2, edges = (idx_t)hops + 1;
	if (slab.pos >= slab.rows) {
		auto fetch = [ids, edges](gg_result *result, int table, idx_t offset, uint32_t want, GGResultSlab &slab) {
			uint32_t got = 0, got_edges = 0;
			auto columns = slab.Columns(ids + edges);
			GGGraph::Check(gg_result_fetch(result, table, offset, want, columns, &got), "gg_result_fetch");
			GGGraph::Check(gg_result_fetch_edges(result, table, offset, want, columns + ids, &got_edges),
			               "gg_result_fetch_edges");
			if (got_edges != got) {
				throw InternalException("gg_khop_extend: id and edge columns of different lengths");
			}
			return got;
		};
		if (!gstate.drain.Refill(slab, [] { return false; }, fetch)) { // (one table: nothing to advance to)
			return;
		}
	}
	const idx_t n = MinValue<idx_t>(STANDARD_VECTOR_SIZE, slab.rows - slab.pos);
	memcpy(FlatVector::GetData<int64_t>(chunk.data[ids]), slab.column[ids + edges - 1] + slab.pos, n * sizeof(int64_t));
	slab.Emit(chunk, 0, ids);
}

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

static unique_ptr<FunctionData> ExtendBindInternal(vector<Value> &inputs, vector<LogicalType> &return_types,
                                                   vector<string> &names, bool count_only) {
	const char *fn = count_only ? "gg_khop_extend_count" : "gg_khop_extend";
	const string vertex_table = inputs[0].ToString(), vertex_key = inputs[1].ToString();
	const string edge_table = inputs[2].ToString(), edge_src = inputs[3].ToString(), edge_dst = inputs[4].ToString();
	const string sources_sql = inputs[5].is_null ? string() : inputs[5].ToString();
	for (idx_t i = 6; i <= 10; i++) {
		if (inputs[i].is_null) {
			throw BinderException(string(fn) + ": hops, ext_table, ext_key_col, ext_next_col and from_col must not be NULL");
		}
	}
	const auto hops = inputs[6].GetValue<int64_t>(), from_col = inputs[10].GetValue<int64_t>();
	const string ext_table = inputs[7].ToString(), ext_key = inputs[8].ToString(), ext_next = inputs[9].ToString();
	if (hops < 1 || hops + 1 > GG_MAX_HOPS) {
		throw BinderException(string(fn) + ": need 1 <= hops <= " + to_string(GG_MAX_HOPS - 1));
	}
	if (from_col < 0 || from_col > hops) {
		throw BinderException(string(fn) + ": from_col must lie in 0.." + to_string(hops));
	}
	auto data = make_unique<GGFunctionData>();
	data->open = [=](ClientContext &ctx, GGOpened &opened) {
		// (tables and columns are resolved at execution time: a missing one raises here)
		opened.graph = GGBuildExtendGraph(ctx, GGTableSource(ctx, vertex_table, {vertex_key}, false),
		                                  GGTableSource(ctx, edge_table, {edge_src, edge_dst}, false),
		                                  GGTableSource(ctx, ext_table, {ext_key, ext_next}, true));
		vector<int64_t> sources;
		if (!sources_sql.empty()) {
			sources = GGQueryInt64Column(ctx, sources_sql, count_only ? "gg_khop_extend_count: sources"
			                                                          : "gg_khop_extend: sources");
		}
		opened.source = make_unique<PhysicalGGExtend>(opened.graph, (int)hops, move(sources), sources_sql.empty(),
		                                              (int)from_col, count_only, 0);
	};
	data->parallel_result = !count_only;
	data->description = to_string(hops) + "-hop walks of " + edge_table + " joined with " + ext_table + " on v" +
	                    to_string(from_col) + " = " + ext_key;
	return_types = PhysicalGGExtend::OutputTypes((int)hops, count_only);
	if (count_only) {
		names = {"rows", "walks", "matched"};
	} else {
		for (int64_t c = 0; c <= hops; c++) {
			names.push_back("v" + to_string(c));
		}
		names.push_back("w");
		names.push_back("ext_rowid");
	}
	return move(data);
}

static unique_ptr<FunctionData> ExtendBind(ClientContext &context, vector<Value> &inputs,
                                           unordered_map<string, Value> &named_parameters,
                                           vector<LogicalType> &input_table_types, vector<string> &input_table_names,
                                           vector<LogicalType> &return_types, vector<string> &names) {
	return ExtendBindInternal(inputs, return_types, names, false);
}

static unique_ptr<FunctionData> ExtendCountBind(ClientContext &context, vector<Value> &inputs,
                                                unordered_map<string, Value> &named_parameters,
                                                vector<LogicalType> &input_table_types, vector<string> &input_table_names,
                                                vector<LogicalType> &return_types, vector<string> &names) {
	return ExtendBindInternal(inputs, return_types, names, true);
}

void GGRegisterExtendFunctions(ClientContext &context) {
	const vector<LogicalType> args = {LogicalType::VARCHAR, LogicalType::VARCHAR, LogicalType::VARCHAR,
	                                  LogicalType::VARCHAR, LogicalType::VARCHAR, LogicalType::VARCHAR,
	                                  LogicalType::BIGINT,  LogicalType::VARCHAR, LogicalType::VARCHAR,
	                                  LogicalType::VARCHAR, LogicalType::BIGINT};
	auto rows = GGScanFunction("gg_khop_extend", args, ExtendBind);
	auto count = GGScanFunction("gg_khop_extend_count", args, ExtendCountBind);
	CreateTableFunctionInfo rows_info(rows), count_info(count);
	auto &catalog = Catalog::GetCatalog(context);
	catalog.CreateTableFunction(context, &rows_info);
	catalog.CreateTableFunction(context, &count_info);
}

} // namespace duckdb
