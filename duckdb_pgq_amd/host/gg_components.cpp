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
// through its own page-locked slab.
#include "gg_table_function.hpp"

namespace duckdb {

namespace {

class PhysicalGGComponents : public GGResultSource {
public:
	PhysicalGGComponents(shared_ptr<GGGraph> graph_p, bool sizes_only_p)
	    : GGResultSource(OutputTypes(sizes_only_p), move(graph_p)), sizes_only(sizes_only_p) {
	}
	static vector<LogicalType> OutputTypes(bool sizes_only) {
		return vector<LogicalType>(sizes_only ? 2 : 3, LogicalType::BIGINT);
	}
	typedef GGDrainStateOf<gg_cc_stats> State;

	bool sizes_only; // table 1 of the result, not table 0

	unique_ptr<GlobalSourceState> GetGlobalSourceState(ClientContext &context) const override {
		auto state = make_unique<State>();
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

	void GetData(ExecutionContext &context, DataChunk &chunk, GlobalSourceState &gstate,
	             LocalSourceState &lstate) const override {
		auto &slab = (GGResultSlab &)lstate;
		PollInterrupt(context);
		auto fetch = [](gg_result *result, int table, idx_t offset, uint32_t want, GGResultSlab &slab) {
			uint32_t got = 0;
			if (table == 1) {
				auto columns = slab.Columns(2);
				GGGraph::Check(gg_components_fetch_sizes(result, offset, want, columns[0], (uint64_t *)columns[1], &got),
				               "gg_components_fetch_sizes");
			} else {
				auto columns = slab.Columns(3);
				GGGraph::Check(gg_components_fetch(result, offset, want, columns[0], columns[1], (uint64_t *)columns[2], &got),
				               "gg_components_fetch");
			}
			return got;
		};
		if (Refill((State &)gstate, slab, fetch)) {
			slab.Emit(chunk, 0, sizes_only ? 2 : 3);
		}
	}

	string GetName() const override {
		return sizes_only ? "GG_COMPONENT_SIZES" : "GG_COMPONENTS";
	}
};

enum { ROWS, SIZES };

unique_ptr<FunctionData> ComponentsBind(ClientContext &context, vector<Value> &inputs, vector<LogicalType> &return_types,
                                        vector<string> &names, int kind) {
	const bool sizes_only = kind == SIZES;
	GGRequireArguments(sizes_only ? "gg_component_sizes" : "gg_components", inputs, {0, 1, 2, 3, 4}, "table and column names");
	const GraphArguments args(inputs);
	auto data = make_unique<GGFunctionData>();
	data->open = [=](ClientContext &ctx, GGOpened &opened) {
		opened.graph = args.Build(ctx);
		opened.source = make_unique<PhysicalGGComponents>(opened.graph, sizes_only);
	};
	data->parallel_result = true;
	data->description = string(sizes_only ? "component sizes of " : "components of ") + args.edge_table;
	return_types = PhysicalGGComponents::OutputTypes(sizes_only);
	if (sizes_only) {
		names = {"component", "size"};
	} else {
		names = {"vertex", "component", "size"};
	}
	return move(data);
}

} // namespace

void GGRegisterComponentFunctions(ClientContext &context) {
	const auto args = GraphArguments::Types();
	GGRegisterTableFunctions(context, {GGScanFunction("gg_components", args, GGBind<ComponentsBind, ROWS>),
	                                   GGScanFunction("gg_component_sizes", args, GGBind<ComponentsBind, SIZES>)});
}

} // namespace duckdb
