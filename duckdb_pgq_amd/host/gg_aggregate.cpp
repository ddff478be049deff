// gg_aggregate.cpp — count(*) and sum(weight) over walks, grouped by one end of the walk, as a table function:
//
//   gg_khop_aggregate(vertex_table, vertex_key, edge_table, src_col, dst_col,
//                     sources_sql VARCHAR, hops BIGINT, group_by VARCHAR, weight_column VARCHAR)
//        -> (vertex BIGINT, walks BIGINT, total HUGEINT)
//
// One row per vertex that starts (group_by 'start') or ends ('end') a `hops`-hop walk from the ids `sources_sql` yields
// (one integer column; NULL or '': from every vertex): how many such walks, and the sum of weight_column — an integer
// column of vertex_table — over their other end.  weight_column NULL: counts only, total = walks.  What that stands for in
// the reference is a grouped aggregate above a join chain,
//     SELECT p0.id, count(*), sum(p2.score) FROM person p0, knows k1, person p1, knows k2, person p2 WHERE ... GROUP BY p0.id
// (the shape of benchmark/ldbc/queries/bi-8.sql:41-53): PhysicalHashAggregate
// (src/execution/operator/aggregate/physical_hash_aggregate.cpp:152-266) fed by the hash joins' probes
// (ScanStructure::NextInnerJoin, src/execution/join_hashtable.cpp:442-476), every walk row formed to be folded away.  Here
// it is `hops` passes over the CSR on the device (gg_khop_aggregate, include/gg.h) and at most one row per vertex comes
// back; total is the reference's own sum(BIGINT) type, HUGEINT (src/function/aggregate/distributive/sum.cpp:115-143).
// One difference from SQL: a NULL weight weighs 0, so a group whose weights are all NULL sums to 0, not NULL.
// No planner rule recognises the shape.
//
//   gg_khop_aggregate_top(vertex_table, vertex_key, edge_table, src_col, dst_col, sources_sql VARCHAR, hops BIGINT,
//                         group_by VARCHAR, weight_column VARCHAR, order_by VARCHAR, descending BOOLEAN,
//                         bias_column VARCHAR, n BIGINT)
//        -> (rank BIGINT, vertex BIGINT, walks BIGINT, total HUGEINT)
//
// The same groups, but only the first n of them under ORDER BY key [DESC], vertex — the tail of bi-8.sql:41-53,
//     ... GROUP BY p.personid, p.score ORDER BY p.score + sum(f.score) DESC, p.personid LIMIT 100
// which the reference runs as PhysicalTopN (src/execution/operator/order/physical_top_n.cpp:238-293, 421-454) above
// PhysicalHashAggregate (src/execution/operator/aggregate/physical_hash_aggregate.cpp:152-266).  order_by 'total': key =
// total + bias_column of the group's vertex (an integer column of vertex_table, read like weight_column; NULL: no bias);
// 'walks': key = walks.  The operator runs gg_khop_aggregate, then gg_khop_aggregate_top on the device, and drains the n
// rows of the answer only; rank is their 0-based place, and they leave in that order (one thread drains).  total is the
// unbiased sum.  As with the weights, a NULL bias adds 0 (in SQL the key would be NULL and sort last or first).
//
// The graph comes from GGBuildGraph — or is the pinned graph of these tables if the connection asked for pinned graphs.
// The weights are read in the statement's own transaction and brought into the order of the graph's vertex table.  The
// groups stay on the device and the pipeline's threads drain them together.
#include <unordered_map>

#include "gg_table_function.hpp"

namespace duckdb {

namespace {

//! a sink that collects (key, value) pairs on the host (GGKeyedValues, gg_extension.hpp): rows with a NULL key are skipped,
//! a NULL value is kept as 0 with has = 0
class PairsGlobalState : public GlobalSinkState {
public:
	mutex lock;
	GGKeyedValues pairs;
};

//! row `idx` of an integer vector as int64
static int64_t IntegerAt(const VectorData &v, PhysicalType type, idx_t idx, const string &fn, const char *what) {
	switch (type) {
	case PhysicalType::INT64:
		return ((const int64_t *)v.data)[idx];
	case PhysicalType::INT32:
		return ((const int32_t *)v.data)[idx];
	case PhysicalType::INT16:
		return ((const int16_t *)v.data)[idx];
	case PhysicalType::INT8:
		return ((const int8_t *)v.data)[idx];
	default:
		throw BinderException(fn + ": " + what + " must be an integer column (TINYINT .. BIGINT)");
	}
}

class PhysicalGGCollectPairs : public PhysicalOperator {
public:
	PhysicalGGCollectPairs(string fn_p, string value_name_p)
	    : PhysicalOperator(PhysicalOperatorType::INVALID, {LogicalType::BIGINT, LogicalType::BIGINT}, 0), fn(move(fn_p)),
	      value_name(move(value_name_p)) {
	}
	string fn, value_name; // for the error that names a column of another type
	unique_ptr<GlobalSinkState> GetGlobalSinkState(ClientContext &context) const override {
		return make_unique<PairsGlobalState>();
	}
	unique_ptr<LocalSinkState> GetLocalSinkState(ExecutionContext &context) const override {
		return make_unique<LocalSinkState>();
	}
	SinkResultType Sink(ExecutionContext &context, GlobalSinkState &gstate_p, LocalSinkState &lstate,
	                    DataChunk &input) const override {
		auto &gstate = (PairsGlobalState &)gstate_p;
		const idx_t count = input.size();
		const auto key_type = input.data[0].GetType().InternalType(), value_type = input.data[1].GetType().InternalType();
		VectorData key, value;
		input.data[0].Orrify(count, key);
		input.data[1].Orrify(count, value);
		GGKeyedValues got;
		got.keys.reserve(count);
		got.values.reserve(count);
		got.has.reserve(count);
		for (idx_t i = 0; i < count; i++) {
			const idx_t k = key.sel->get_index(i), v = value.sel->get_index(i);
			if (!key.validity.RowIsValid(k)) {
				continue;
			}
			const bool valid = value.validity.RowIsValid(v);
			got.keys.push_back(IntegerAt(key, key_type, k, fn, "the key"));
			got.values.push_back(valid ? IntegerAt(value, value_type, v, fn, value_name.c_str()) : 0);
			got.has.push_back(valid);
		}
		lock_guard<mutex> guard(gstate.lock);
		auto &all = gstate.pairs;
		all.keys.insert(all.keys.end(), got.keys.begin(), got.keys.end());
		all.values.insert(all.values.end(), got.values.begin(), got.values.end());
		all.has.insert(all.has.end(), got.has.begin(), got.has.end());
		return SinkResultType::NEED_MORE_INPUT;
	}
	bool IsSink() const override {
		return true;
	}
	bool ParallelSink() const override {
		return true;
	}
	string GetName() const override {
		return "GG_COLLECT_PAIRS";
	}
};

} // namespace

GGKeyedValues GGCollectKeyedValues(ClientContext &context, const GGScanSource &source, const string &fn,
                                   const string &value_name) {
	PhysicalGGCollectPairs collect(fn, value_name);
	GGRunSinkPipeline(context, source, collect);
	return move(((PairsGlobalState &)*collect.sink_state).pairs);
}

namespace {

//! weight_column of vertex_table in the order of the graph's vertex table (a vertex the scan did not see weighs 0)
static vector<int64_t> WeightsInVertexOrder(ClientContext &context, GGGraph &graph, const string &vertex_table,
                                            const string &vertex_key, const string &weight_column) {
	// (a NULL weight arrives as 0: it weighs nothing)
	const auto pairs = GGCollectKeyedValues(context, GGTableSource(context, vertex_table, {vertex_key, weight_column}, false),
	                                        "gg_khop_aggregate", "weight_column");
	std::unordered_map<int64_t, int64_t> weight_of;
	weight_of.reserve(pairs.keys.size());
	for (idx_t i = 0; i < pairs.keys.size(); i++) {
		weight_of[pairs.keys[i]] = pairs.values[i];
	}
	shared_ptr<const vector<int64_t>> ids;
	{
		lock_guard<mutex> guard(graph.lock);
		ids = graph.VertexIds();
	}
	vector<int64_t> weights(ids->size(), 0);
	for (idx_t v = 0; v < ids->size(); v++) {
		auto it = weight_of.find((*ids)[v]);
		if (it != weight_of.end()) {
			weights[v] = it->second;
		}
	}
	return weights;
}

//! Source: one row (vertex BIGINT, walks BIGINT, total HUGEINT) per vertex that starts (group_by GG_GROUP_START) or ends
//! (GG_GROUP_END) a `hops`-hop walk from the sources: the number of such walks and the sum of the weights at their other
//! end (gg_khop_aggregate, include/gg.h).  weights: one per vertex in the graph's vertex-table order (weighted false:
//! counts only, total = walks).
class PhysicalGGKhopAggregate : public GGWalkSource {
public:
	PhysicalGGKhopAggregate(shared_ptr<GGGraph> graph_p, int hops_p, vector<int64_t> sources_p, bool all_sources_p,
	                        int group_by_p, vector<int64_t> weights_p, bool weighted_p,
	                        vector<LogicalType> types = OutputTypes())
	    : GGWalkSource(move(types), move(graph_p), hops_p, move(sources_p), all_sources_p), group_by(group_by_p),
	      weights(move(weights_p)), weighted(weighted_p) {
	}
	static vector<LogicalType> OutputTypes() {
		return {LogicalType::BIGINT, LogicalType::BIGINT, LogicalType::HUGEINT};
	}
	typedef GGDrainStateOf<gg_agg_stats> State;

	int group_by; // GG_GROUP_START / GG_GROUP_END
	vector<int64_t> weights;
	bool weighted;

	//! the groups, on the device; caller holds graph->lock
	void Aggregate(State &state, GGResultPtr &out) const {
		GGGraph::Check(gg_khop_aggregate(graph->ctx, graph->csr, SourceIds(), SourceCount(), hops, hops, group_by,
		                                 weighted ? weights.data() : nullptr, &state.stats, GGResultOut(out)),
		               "gg_khop_aggregate");
	}

	unique_ptr<GlobalSourceState> GetGlobalSourceState(ClientContext &context) const override {
		auto state = make_unique<State>();
		lock_guard<mutex> guard(graph->lock);
		if (!graph->csr) {
			throw InternalException("GG_KHOP_AGGREGATE scheduled before the CSR was built");
		}
		state->drain.Replace(context, hops, [&](idx_t &rows) {
			GGResultPtr owner;
			Aggregate(*state, owner);
			rows = state->stats.groups[hops];
			return owner;
		});
		state->max_threads = GGResultSlab::ThreadsFor(state->stats.groups[hops]);
		return move(state);
	}

	//! Serves the next groups: vertex and walks as they are into chunk.data[first ..], then the total, whose halves lie
	//! side by side in the slab.  Returns their number (0: nothing is left).
	idx_t EmitGroups(State &gstate, GGResultSlab &slab, DataChunk &chunk, idx_t first) const {
		auto fetch = [](gg_result *result, int table, idx_t offset, uint32_t want, GGResultSlab &slab) {
			uint32_t got = 0;
			auto columns = slab.Columns(4); // vertex id, walks, low and high half of the total
			GGGraph::Check(gg_khop_aggregate_fetch(result, table, offset, want, columns[0], (uint64_t *)columns[1],
			                                       (uint64_t *)columns[2], columns[3], &got),
			               "gg_khop_aggregate_fetch");
			return got;
		};
		if (!Refill(gstate, slab, fetch)) {
			return 0;
		}
		const idx_t at = slab.pos;
		const idx_t n = slab.Emit(chunk, first, 2);
		auto total = FlatVector::GetData<hugeint_t>(chunk.data[first + 2]);
		for (idx_t i = 0; i < n; i++) {
			total[i].lower = (uint64_t)slab.column[2][at + i];
			total[i].upper = slab.column[3][at + i];
		}
		return n;
	}

	void GetData(ExecutionContext &context, DataChunk &chunk, GlobalSourceState &gstate,
	             LocalSourceState &lstate) const override {
		PollInterrupt(context);
		EmitGroups((State &)gstate, (GGResultSlab &)lstate, chunk, 0);
	}

	string GetName() const override {
		return "GG_KHOP_AGGREGATE";
	}
};

//! The first n groups of PhysicalGGKhopAggregate's answer in rank order: gg_khop_aggregate_top behind gg_khop_aggregate
class PhysicalGGKhopAggregateTop : public PhysicalGGKhopAggregate {
public:
	PhysicalGGKhopAggregateTop(shared_ptr<GGGraph> graph_p, int hops_p, vector<int64_t> sources_p, bool all_sources_p,
	                           int group_by_p, vector<int64_t> weights_p, bool weighted_p, int order_by_p, bool descending_p,
	                           vector<int64_t> bias_p, bool biased_p, uint64_t n_p)
	    : PhysicalGGKhopAggregate(move(graph_p), hops_p, move(sources_p), all_sources_p, group_by_p, move(weights_p),
	                              weighted_p, OutputTypes()),
	      order_by(order_by_p), descending(descending_p), bias(move(bias_p)), biased(biased_p), n(n_p) {
	}
	static vector<LogicalType> OutputTypes() {
		return {LogicalType::BIGINT, LogicalType::BIGINT, LogicalType::BIGINT, LogicalType::HUGEINT};
	}

	int order_by; // GG_TOP_BY_TOTAL / GG_TOP_BY_WALKS
	bool descending;
	vector<int64_t> bias; // one per vertex in the graph's vertex-table order
	bool biased;
	uint64_t n;

	unique_ptr<GlobalSourceState> GetGlobalSourceState(ClientContext &context) const override {
		auto state = make_unique<State>(); // (max_threads stays 1: the rows leave in rank order)
		lock_guard<mutex> guard(graph->lock);
		if (!graph->csr) {
			throw InternalException("GG_KHOP_AGGREGATE_TOP scheduled before the CSR was built");
		}
		state->drain.Replace(context, hops, [&](idx_t &rows) {
			GGResultPtr groups, owner;
			Aggregate(*state, groups);
			gg_top_stats top {};
			GGGraph::Check(gg_khop_aggregate_top(graph->ctx, groups.get(), hops, order_by, descending ? 1 : 0, n,
			                                     biased ? graph->csr : nullptr, biased ? bias.data() : nullptr, &top,
			                                     GGResultOut(owner)),
			               "gg_khop_aggregate_top");
			rows = top.rows_out;
			return owner; // (the groups go back to the pool here: only the top rows stay in HBM)
		});
		return move(state);
	}

	void GetData(ExecutionContext &context, DataChunk &chunk, GlobalSourceState &gstate,
	             LocalSourceState &lstate) const override {
		PollInterrupt(context);
		EmitRank((State &)gstate, chunk, EmitGroups((State &)gstate, (GGResultSlab &)lstate, chunk, 1));
	}

	string GetName() const override {
		return "GG_KHOP_AGGREGATE_TOP";
	}
};

enum { GROUPS, TOP };

//! gg_khop_aggregate, and with four more arguments gg_khop_aggregate_top
unique_ptr<FunctionData> KhopAggregateBind(ClientContext &context, vector<Value> &inputs, vector<LogicalType> &return_types,
                                           vector<string> &names, int kind) {
	const bool top = kind == TOP;
	const GGWalkArguments args = top ? GGWalkArguments("gg_khop_aggregate_top", inputs, GGWalkArguments::NO_EXTENSION,
	                                                   {6, 7, 9, 10, 12}, "hops, group_by, order_by, descending and n")
	                                 : GGWalkArguments("gg_khop_aggregate", inputs, GGWalkArguments::NO_EXTENSION, {6, 7},
	                                                   "hops and group_by");
	const string &fn = args.fn;
	const string group_name = inputs[7].ToString();
	const bool weighted = !inputs[8].is_null;
	const string weight_column = weighted ? inputs[8].ToString() : string();
	const string order_name = top ? inputs[9].ToString() : string();
	const bool descending = top && inputs[10].GetValue<bool>();
	const bool biased = top && !inputs[11].is_null;
	const string bias_column = biased ? inputs[11].ToString() : string();
	const auto n = top ? inputs[12].GetValue<int64_t>() : 0;
	if (n < 0) {
		throw BinderException(fn + ": n must not be negative");
	}
	int group_by, order_by = GG_TOP_BY_TOTAL;
	if (group_name == "start") {
		group_by = GG_GROUP_START;
	} else if (group_name == "end") {
		group_by = GG_GROUP_END;
	} else {
		throw BinderException(fn + ": group_by '" + group_name + "' (one of 'start', 'end')");
	}
	if (top && order_name == "walks") {
		order_by = GG_TOP_BY_WALKS;
	} else if (top && order_name != "total") {
		throw BinderException(fn + ": order_by '" + order_name + "' (one of 'total', 'walks')");
	}
	if (biased && order_by == GG_TOP_BY_WALKS) {
		throw BinderException(fn + ": a bias_column is added to the total only");
	}
	auto data = make_unique<GGFunctionData>();
	data->open = [=](ClientContext &ctx, GGOpened &opened) {
		opened.graph = args.BuildGraph(ctx);
		vector<int64_t> sources = args.Sources(ctx), weights, bias;
		if (weighted) {
			weights = WeightsInVertexOrder(ctx, *opened.graph, args.vertex_table, args.vertex_key, weight_column);
		}
		if (biased) {
			bias = WeightsInVertexOrder(ctx, *opened.graph, args.vertex_table, args.vertex_key, bias_column);
		}
		if (top) {
			opened.source = make_unique<PhysicalGGKhopAggregateTop>(opened.graph, (int)args.hops, move(sources),
			                                                        args.AllSources(), group_by, move(weights), weighted,
			                                                        order_by, descending, move(bias), biased, (uint64_t)n);
		} else {
			opened.source = make_unique<PhysicalGGKhopAggregate>(opened.graph, (int)args.hops, move(sources), args.AllSources(),
			                                                     group_by, move(weights), weighted);
		}
	};
	data->parallel_result = !top; // (the top's rows leave in rank order)
	data->description = (weighted ? "count, sum(" + weight_column + ")" : string("count")) + " by " + group_name + " over " +
	                    args.Describe();
	if (top) {
		data->description = "top " + to_string(n) + " by " + (biased ? bias_column + " + " : string()) + order_name +
		                    (descending ? " desc" : "") + " of " + data->description;
		return_types = PhysicalGGKhopAggregateTop::OutputTypes();
		names = {"rank", "vertex", "walks", "total"};
	} else {
		return_types = PhysicalGGKhopAggregate::OutputTypes();
		names = {"vertex", "walks", "total"};
	}
	return move(data);
}

} // namespace

void GGRegisterAggregateFunctions(ClientContext &context) {
	auto args = GGWalkArguments::Types(false);
	args.insert(args.end(), {LogicalType::VARCHAR, LogicalType::VARCHAR});
	auto top_args = args;
	top_args.insert(top_args.end(), {LogicalType::VARCHAR, LogicalType::BOOLEAN, LogicalType::VARCHAR, LogicalType::BIGINT});
	GGRegisterTableFunctions(context, {GGScanFunction("gg_khop_aggregate", args, GGBind<KhopAggregateBind, GROUPS>),
	                                   GGScanFunction("gg_khop_aggregate_top", top_args, GGBind<KhopAggregateBind, TOP>)});
}

} // namespace duckdb
