// gg_components.cpp — weakly connected components as table functions:
//
//   gg_components(vertex_table, vertex_key, edge_table, src_col, dst_col)      -> (vertex BIGINT, component BIGINT, size BIGINT)
//   gg_component_sizes(vertex_table, vertex_key, edge_table, src_col, dst_col) -> (component BIGINT, size BIGINT)
//
// gg_components has one row per row of the vertex table: the vertex, the id of its component (the id of the component's
// first vertex in the vertex table) and the number of the component's members; gg_component_sizes one row per component.
// Two vertices are in one component iff edge rows whose endpoints are both vertices join them, direction ignored.  What
// that stands for in the reference is a UNION recursive CTE under an aggregate,
//     WITH RECURSIVE cc(v, root) AS (SELECT id, id FROM vertices UNION SELECT u.b, cc.root FROM cc, und u WHERE cc.v = u.a)
//     SELECT v, min(root), count(*) FROM cc GROUP BY v             -- und: every kept edge row in both directions
// PhysicalRecursiveCTE (src/execution/operator/set/physical_recursive_cte.cpp:47-139) re-running the arm's hash join per
// level, sum |component|^2 rows probed against one GroupedAggregateHashTable (src/execution/aggregate_hashtable.cpp:367-504),
// then PhysicalHashAggregate (src/execution/operator/aggregate/physical_hash_aggregate.cpp:152-266).  Here it is one pass
// over the edge entries (gg_components, include/gg.h).  No planner rule recognises the shape.
//
// The graph comes from GGBuildGraph — or is the pinned graph of these tables if the connection asked for pinned graphs.
// The call runs under the graph's lock; the rows stay on the device and the pipeline's threads drain them together, each
// through its own page-locked slab (GGResultDrain, gg_operators.hpp: one result, one table of it).
#include "duckdb.hpp"
#include "duckdb/catalog/catalog.hpp"
#include "duckdb/common/exception.hpp"
#include "duckdb/main/client_context.hpp"
#include "duckdb/parser/parsed_data/create_table_function_info.hpp"

#include "gg_extension.hpp"
#include "gg_operators.hpp"

namespace duckdb {

namespace {

class ComponentsState : public GlobalSourceState {
public:
	idx_t MaxThreads() override {
		return max_threads;
	}
	gg_cc_stats stats {};
	GGResultDrain drain;
	idx_t max_threads = 1;
};

class PhysicalGGComponents : public PhysicalOperator {
public:
	PhysicalGGComponents(shared_ptr<GGGraph> graph_p, bool sizes_only_p)
	    : PhysicalOperator(PhysicalOperatorType::INVALID, OutputTypes(sizes_only_p), 0), graph(move(graph_p)),
	      sizes_only(sizes_only_p) {
	}
	static vector<LogicalType> OutputTypes(bool sizes_only) {
		return vector<LogicalType>(sizes_only ? 2 : 3, LogicalType::BIGINT);
	}

	shared_ptr<GGGraph> graph;
	bool sizes_only; // table 1 of the result, not table 0

	unique_ptr<GlobalSourceState> GetGlobalSourceState(ClientContext &context) const override {
		auto state = make_unique<ComponentsState>();
		lock_guard<mutex> guard(graph->lock);
		if (!graph->csr) {
			throw InternalException("GG_COMPONENTS scheduled before the CSR was built");
		}
		state->drain.Replace(context, sizes_only ? 1 : 0, [&](idx_t &rows) {
			GGResultPtr owner;
			GGGraph::Check(gg_components(graph->ctx, graph->csr, &state->stats, GGResultOut(owner)), "gg_components");
			rows = sizes_only ? state->stats.components : state->stats.vertices;
			return owner;
		});
		state->max_threads = GGResultSlab::ThreadsFor(state->drain.Rows());
		return move(state);
	}

	unique_ptr<LocalSourceState> GetLocalSourceState(ExecutionContext &context, GlobalSourceState &gstate) const override {
		return make_unique<GGResultSlab>(graph);
	}

	void GetData(ExecutionContext &context, DataChunk &chunk, GlobalSourceState &gstate_p,
	             LocalSourceState &lstate) const override {
		auto &gstate = (ComponentsState &)gstate_p;
		auto &slab = (GGResultSlab &)lstate;
		if (context.client.interrupted) {
			throw InterruptException();
		}
		if (slab.pos >= slab.rows) {
			auto fetch = [](gg_result *result, int table, idx_t offset, uint32_t want, GGResultSlab &slab) {
				uint32_t got = 0;
				if (table == 1) {
					auto columns = slab.Columns(2);
					GGGraph::Check(gg_components_fetch_sizes(result, offset, want, columns[0], (uint64_t *)columns[1], &got),
					               "gg_components_fetch_sizes");
				} else {
					auto columns = slab.Columns(3);
					GGGraph::Check(gg_components_fetch(result, offset, want, columns[0], columns[1],
					                                   (uint64_t *)columns[2], &got),
					               "gg_components_fetch");
				}
				return got;
			};
			if (!gstate.drain.Refill(slab, [] { return false; }, fetch)) { // (one table: nothing to advance to)
				return;
			}
		}
		slab.Emit(chunk, 0, sizes_only ? 2 : 3);
	}

	string GetName() const override {
		return sizes_only ? "GG_COMPONENT_SIZES" : "GG_COMPONENTS";
	}
};

} // namespace

static unique_ptr<FunctionData> ComponentsBindInternal(vector<Value> &inputs, vector<LogicalType> &return_types,
                                                       vector<string> &names, bool sizes_only) {
	const char *fn = sizes_only ? "gg_component_sizes" : "gg_components";
	for (idx_t i = 0; i < 5; i++) {
		if (inputs[i].is_null) {
			throw BinderException(string(fn) + ": table and column names must not be NULL");
		}
	}
	const string vertex_table = inputs[0].ToString(), vertex_key = inputs[1].ToString();
	const string edge_table = inputs[2].ToString(), edge_src = inputs[3].ToString(), edge_dst = inputs[4].ToString();
	auto data = make_unique<GGFunctionData>();
	data->open = [=](ClientContext &ctx, GGOpened &opened) {
		GGGraphSpec spec; // (tables and columns are resolved at execution time: a missing one raises here)
		spec.vertices = GGTableSource(ctx, vertex_table, {vertex_key}, false);
		spec.edges = GGTableSource(ctx, edge_table, {edge_src, edge_dst}, false);
		opened.graph = GGBuildGraph(ctx, spec);
		opened.source = make_unique<PhysicalGGComponents>(opened.graph, sizes_only);
	};
	data->parallel_result = true;
	data->description = string(sizes_only ? "component sizes of " : "components of ") + edge_table;
	return_types = PhysicalGGComponents::OutputTypes(sizes_only);
	if (sizes_only) {
		names = {"component", "size"};
	} else {
		names = {"vertex", "component", "size"};
	}
	return move(data);
}

static unique_ptr<FunctionData> ComponentsBind(ClientContext &context, vector<Value> &inputs,
                                               unordered_map<string, Value> &named_parameters,
                                               vector<LogicalType> &input_table_types, vector<string> &input_table_names,
                                               vector<LogicalType> &return_types, vector<string> &names) {
	return ComponentsBindInternal(inputs, return_types, names, false);
}

static unique_ptr<FunctionData> ComponentSizesBind(ClientContext &context, vector<Value> &inputs,
                                                   unordered_map<string, Value> &named_parameters,
                                                   vector<LogicalType> &input_table_types,
                                                   vector<string> &input_table_names, vector<LogicalType> &return_types,
                                                   vector<string> &names) {
	return ComponentsBindInternal(inputs, return_types, names, true);
}

void GGRegisterComponentFunctions(ClientContext &context) {
	const vector<LogicalType> args(5, LogicalType::VARCHAR);
	auto rows = GGScanFunction("gg_components", args, ComponentsBind);
	auto sizes = GGScanFunction("gg_component_sizes", args, ComponentSizesBind);
	CreateTableFunctionInfo rows_info(rows), sizes_info(sizes);
	auto &catalog = Catalog::GetCatalog(context);
	catalog.CreateTableFunction(context, &rows_info);
	catalog.CreateTableFunction(context, &sizes_info);
}

} // namespace duckdb
