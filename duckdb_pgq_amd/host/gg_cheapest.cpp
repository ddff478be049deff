// gg_cheapest.cpp — the cheapest walks over a weighted edge table, as a table function:
//
//   gg_cheapest_path(vertex_table, vertex_key, edge_table, src_col, dst_col, weight_column VARCHAR,
//                    sources_sql VARCHAR, targets_sql VARCHAR, max_hops BIGINT)
//        -> (source BIGINT, vertex BIGINT, cost BIGINT, hops INTEGER)
//
// One row per (source, vertex) pair joined by a walk of at most `max_hops` edge rows (NULL or negative: of any length),
// with the smallest sum of `weight_column` over such a walk — saturating at INT64_MAX — and the fewest edges of a walk of
// that cost; the source itself is a row of cost 0 and 0 hops.  The sources are the distinct non-NULL values `sources_sql`
// yields (one integer column), in first-occurrence order; NULL or '': every vertex.  `targets_sql` restricts the reported
// vertices likewise; NULL or '': no restriction.  What that stands for in the reference is the weighted half of its
// shortest-path family (cheapest_path_length), or by hand a UNION ALL recursive CTE under min(cost):
//     WITH RECURSIVE w(s, v, cost, hops) AS (SELECT id, id, 0, 0 FROM person WHERE id IN (...) UNION ALL
//       SELECT w.s, k.dst, w.cost + k.weight, w.hops + 1 FROM w, knows k, person p WHERE w.v = k.src AND k.dst = p.id
//       AND w.hops < H) SELECT s, v, min(cost) ... GROUP BY s, v
// — PhysicalRecursiveCTE (src/execution/operator/set/physical_recursive_cte.cpp) re-running a hash join per round and a
// two-key PhysicalHashAggregate over every walk row it formed.  Here it is one min-plus pass over the reverse CSR per round
// and batch of 64 sources (gg_cheapest64, include/gg.h).
// No planner rule recognises the shape.
//
//   gg_cheapest_path_rows(vertex_table, vertex_key, edge_table, src_col, dst_col, weight_column VARCHAR, pairs_sql VARCHAR)
//        -> (src BIGINT, dst BIGINT, step INTEGER, vertex BIGINT, edge_rowid BIGINT, cost BIGINT)
//
// The cheapest paths themselves, unnested: for every pair (src, dst) `pairs_sql` yields (two integer columns; a row with a
// NULL is no pair, duplicate pairs each get their rows) one row per step 0..hops of the pinned cheapest path
// (gg_cheapest64_paths, include/gg.h: the fewest edges of a cheapest walk, the predecessor with the smallest vertex-table
// position, among parallel rows the one appended first) with the rowid of the edge into the step's vertex (NULL at step 0)
// and the cost up to it.  Always to the fixpoint: the state of a hop-bounded search cannot be traced.  A pair without a walk,
// or whose cost saturates at INT64_MAX, has no rows.  Pairs are grouped by source, 64 distinct sources to a batch in
// first-occurrence order, and drained as gg_shortest_path_rows drains them (ShortestPathRowsState, gg_operators.hpp).
//
// The graph comes from GGBuildGraphWithRowids — the rowid-carrying companion of the pinned graph of these tables if the
// connection asked for pinned graphs.  (rowid, weight_column) is read in the statement's own transaction, laid out densely
// by rowid and handed over as GG_WEIGHTS_BY_ROWID, once per statement; a NULL or negative weight and a column that is no
// integer raise.  One batch of 64 sources is resident at a time: the pipeline's threads drain its rows together
// (GGResultDrain, gg_operators.hpp), and whoever claims the last of them runs the next batch under the graph's lock.
#include <unordered_set>

#include "gg_table_function.hpp"

namespace duckdb {

namespace {

class CheapestState : public GlobalSourceState {
public:
	idx_t MaxThreads() override {
		return max_threads;
	}
	vector<int64_t> uniq; // the sources, deduplicated, in 64-lane batches
	//! the rows of the current batch; its table is the batch's first source
	GGResultDrain drain;
	idx_t max_threads = 1;
};

//! the distinct values of `ids` in first-occurrence order
static vector<int64_t> Distinct(const vector<int64_t> &ids) {
	vector<int64_t> out;
	std::unordered_set<int64_t> seen;
	for (auto id : ids) {
		if (seen.insert(id).second) {
			out.push_back(id);
		}
	}
	return out;
}

struct GGWeightsDestroy {
	void operator()(gg_edge_weights *weights) const {
		gg_edge_weights_destroy(weights);
	}
};
typedef std::unique_ptr<gg_edge_weights, GGWeightsDestroy> GGWeightsPtr;

class PhysicalGGCheapestPath : public GGResultSource {
public:
	PhysicalGGCheapestPath(shared_ptr<GGGraph> graph_p, GGWeightsPtr weights_p, int64_t max_hops_p,
	                       vector<int64_t> sources_p, bool all_sources_p, vector<int64_t> targets_p, bool all_targets_p)
	    : GGResultSource(OutputTypes(), move(graph_p)), weights(move(weights_p)), max_hops(max_hops_p),
	      sources(move(sources_p)), all_sources(all_sources_p), targets(move(targets_p)), all_targets(all_targets_p) {
	}
	static vector<LogicalType> OutputTypes() {
		return {LogicalType::BIGINT, LogicalType::BIGINT, LogicalType::BIGINT, LogicalType::INTEGER};
	}

	GGWeightsPtr weights; // (a member of the derived class: destroyed before the base's graph, as gg.h asks)
	int64_t max_hops;
	vector<int64_t> sources; // distinct (ignored if all_sources)
	bool all_sources;
	vector<int64_t> targets; // (ignored if all_targets)
	bool all_targets;

	//! the rows of the batch starting at source batch_base; caller holds graph->lock
	GGResultPtr RunBatch(CheapestState &state, idx_t batch_base, idx_t &rows) const {
		const int n = (int)MinValue<idx_t>(GG_BFS_LANES, state.uniq.size() - batch_base);
		const int64_t *dst = all_targets ? nullptr : GGSourceIds(targets);
		GGResultPtr owner;
		GGGraph::Check(gg_cheapest64(graph->ctx, graph->csr, weights.get(), state.uniq.data() + batch_base, n, max_hops, dst,
		                             all_targets ? 0 : targets.size(), nullptr, GGResultOut(owner)),
		               "gg_cheapest64");
		uint64_t n_rows = 0;
		GGGraph::Check(gg_cheapest64_rows(owner.get(), &n_rows), "gg_cheapest64_rows");
		rows = n_rows;
		return owner;
	}

	unique_ptr<GlobalSourceState> GetGlobalSourceState(ClientContext &context) const override {
		auto state = make_unique<CheapestState>();
		lock_guard<mutex> guard(graph->lock);
		if (!graph->csr) {
			throw InternalException("GG_CHEAPEST_PATH scheduled before the CSR was built");
		}
		if (all_sources) {
			state->uniq = *graph->VertexIds(); // vertex-table order (a vertex table's key is unique)
		} else {
			state->uniq = sources;
		}
		if (!state->uniq.empty()) {
			state->drain.Replace(context, 0, [&](idx_t &rows) { return RunBatch(*state, 0, rows); });
		}
		// the first batch's size is the only estimate there is of how much the threads will have to drain
		const idx_t batches = (state->uniq.size() + GG_BFS_LANES - 1) / GG_BFS_LANES;
		state->max_threads = GGResultSlab::ThreadsFor(state->drain.Rows() * batches);
		return move(state);
	}

	void GetData(ExecutionContext &context, DataChunk &chunk, GlobalSourceState &gstate_p,
	             LocalSourceState &lstate) const override {
		auto &gstate = (CheapestState &)gstate_p;
		auto &slab = (GGResultSlab &)lstate;
		PollInterrupt(context);
		if (slab.pos >= slab.rows) {
			auto &drain = gstate.drain;
			auto advance = [&]() -> bool { // current batch claimed completely: run the next one
				const idx_t next = (idx_t)drain.Table() + GG_BFS_LANES;
				if (next >= gstate.uniq.size()) {
					return false;
				}
				// (the drain's lock stays held through the rounds on purpose: the other threads have nothing to claim
				// until the next batch's rows exist)
				drain.Replace(context.client, (int)next, [&](idx_t &rows) {
					lock_guard<mutex> device_guard(graph->lock);
					return RunBatch(gstate, next, rows);
				});
				return true;
			};
			auto fetch = [](gg_result *result, int, idx_t offset, uint32_t want, GGResultSlab &slab) {
				uint32_t got = 0;
				// vertex id, cost, then the source's index in its batch and the hops (int32 cells in an int64 column's room)
				auto columns = slab.Columns(4);
				GGGraph::Check(gg_cheapest64_fetch(result, offset, want, columns[2], columns[0], columns[1],
				                                   (int32_t *)columns[3], &got),
				               "gg_cheapest64_fetch");
				return got;
			};
			if (!drain.Refill(slab, advance, fetch)) { // (lane i of a slab's rows is source uniq[slab.table + i])
				return;
			}
		}
		const idx_t first = slab.pos;
		const idx_t n = slab.Emit(chunk, 1, 2);
		auto source = FlatVector::GetData<int64_t>(chunk.data[0]);
		auto hops = FlatVector::GetData<int32_t>(chunk.data[3]);
		const int64_t *lane_source = gstate.uniq.data() + slab.table;
		const int32_t *slab_hops = (const int32_t *)slab.column[3];
		for (idx_t i = 0; i < n; i++) {
			source[i] = lane_source[slab.column[2][first + i]];
			hops[i] = slab_hops[first + i];
		}
	}

	string GetName() const override {
		return "GG_CHEAPEST_PATH";
	}
};

//! The path rows of gg_cheapest64_paths, batch by batch.
class PhysicalGGCheapestPathRows : public GGResultSource {
public:
	PhysicalGGCheapestPathRows(shared_ptr<GGGraph> graph_p, GGWeightsPtr weights_p, vector<int64_t> src_p,
	                           vector<int64_t> dst_p)
	    : GGResultSource(OutputTypes(), move(graph_p)), weights(move(weights_p)), src(move(src_p)), dst(move(dst_p)) {
		D_ASSERT(src.size() == dst.size());
	}
	static vector<LogicalType> OutputTypes() {
		return {LogicalType::BIGINT, LogicalType::BIGINT, LogicalType::INTEGER,
		        LogicalType::BIGINT, LogicalType::BIGINT, LogicalType::BIGINT};
	}

	GGWeightsPtr weights; // (a member of the derived class: destroyed before the base's graph, as gg.h asks)
	vector<int64_t> src, dst;

	//! trace the pairs of a batch; caller holds graph->lock
	GGResultPtr RunBatch(ShortestPathRowsState &state, idx_t batch, idx_t &rows) const {
		const idx_t base = batch * GG_BFS_LANES;
		const int n = (int)MinValue<idx_t>(GG_BFS_LANES, state.uniq.size() - base);
		auto &members = state.members[batch];
		vector<int64_t> targets(members.size());
		for (idx_t i = 0; i < members.size(); i++) {
			targets[i] = dst[members[i]];
		}
		GGResultPtr owner;
		GGGraph::Check(gg_cheapest64_paths(graph->ctx, graph->csr, weights.get(), state.uniq.data() + base, n,
		                                   state.lanes[batch].data(), targets.data(), targets.size(), 1, nullptr,
		                                   GGResultOut(owner)),
		               "gg_cheapest64_paths");
		uint64_t n_rows = 0;
		GGGraph::Check(gg_cheapest64_paths_rows(owner.get(), 1, &n_rows), "gg_cheapest64_paths_rows");
		rows = n_rows;
		return owner;
	}

	unique_ptr<GlobalSourceState> GetGlobalSourceState(ClientContext &context) const override {
		auto state = make_unique<ShortestPathRowsState>();
		lock_guard<mutex> guard(graph->lock);
		if (!graph->csr) {
			throw InternalException("GG_CHEAPEST_PATH_ROWS scheduled before the CSR was built");
		}
		state->Group(src);
		if (!state->members.empty()) {
			state->drain.Replace(context, 0, [&](idx_t &rows) { return RunBatch(*state, 0, rows); });
		}
		// the first batch's size is the only estimate there is of how much the threads will have to drain
		state->max_threads = GGResultSlab::ThreadsFor(state->drain.Rows() * state->members.size());
		return move(state);
	}

	void GetData(ExecutionContext &context, DataChunk &chunk, GlobalSourceState &gstate_p,
	             LocalSourceState &lstate) const override {
		auto &gstate = (ShortestPathRowsState &)gstate_p;
		auto &slab = (GGResultSlab &)lstate;
		PollInterrupt(context);
		if (slab.pos >= slab.rows) {
			auto &drain = gstate.drain;
			auto advance = [&]() -> bool { // current batch claimed completely: run the next one
				const idx_t next = (idx_t)drain.Table() + 1;
				if (next >= gstate.members.size()) {
					return false;
				}
				if (context.client.interrupted) {
					throw InterruptException();
				}
				// (the drain's lock stays held through the rounds on purpose: the other threads have nothing to claim
				// until the next batch's rows exist)
				drain.Replace(context.client, (int)next, [&](idx_t &rows) {
					lock_guard<mutex> device_guard(graph->lock);
					return RunBatch(gstate, next, rows);
				});
				return true;
			};
			auto fetch = [](gg_result *result, int, idx_t offset, uint32_t want, GGResultSlab &slab) {
				// columns 0..3: pair, vertex, edge rowid, cost; column 4's memory holds the int32 steps
				auto columns = slab.Columns(5);
				uint32_t got = 0;
				GGGraph::Check(gg_cheapest64_paths_fetch(result, offset, want, columns[0], (int32_t *)columns[4], columns[1],
				                                         columns[2], columns[3], &got),
				               "gg_cheapest64_paths_fetch");
				return got;
			};
			if (!drain.Refill(slab, advance, fetch)) { // (pair i of a slab's rows is members[slab.table][i])
				return;
			}
		}
		const idx_t n = MinValue<idx_t>(STANDARD_VECTOR_SIZE, slab.rows - slab.pos);
		auto out_src = FlatVector::GetData<int64_t>(chunk.data[0]);
		auto out_dst = FlatVector::GetData<int64_t>(chunk.data[1]);
		auto out_step = FlatVector::GetData<int32_t>(chunk.data[2]);
		auto out_vertex = FlatVector::GetData<int64_t>(chunk.data[3]);
		auto out_edge = FlatVector::GetData<int64_t>(chunk.data[4]);
		auto out_cost = FlatVector::GetData<int64_t>(chunk.data[5]);
		auto &edge_validity = FlatVector::Validity(chunk.data[4]);
		auto &members = gstate.members[slab.table]; // (filled before the first batch ran; never changed afterwards)
		const int64_t *pair = slab.column[0] + slab.pos, *vertex = slab.column[1] + slab.pos;
		const int64_t *edge = slab.column[2] + slab.pos, *cost = slab.column[3] + slab.pos;
		const int32_t *step = (const int32_t *)slab.column[4] + slab.pos;
		for (idx_t i = 0; i < n; i++) {
			const idx_t p = members[(idx_t)pair[i]];
			out_src[i] = src[p];
			out_dst[i] = dst[p];
			out_step[i] = step[i];
			out_vertex[i] = vertex[i];
			out_edge[i] = edge[i];
			out_cost[i] = cost[i];
			if (step[i] == 0) { // no edge leads into the path's first vertex
				edge_validity.SetInvalid(i);
			}
		}
		slab.pos += n;
		chunk.SetCardinality(n);
	}

	string GetName() const override {
		return "GG_CHEAPEST_PATH_ROWS";
	}
};

//! weight_column of edge_table as one weight per rowid (a rowid no row has weighs 0 and is never read), on the device
static GGWeightsPtr WeightsByRowid(ClientContext &context, GGGraph &graph, const string &edge_table,
                                   const string &weight_column) {
	const string column_name = "weight column " + GGQuote(weight_column);
	auto source = GGTableSource(context, edge_table, {weight_column}, true); // (weight, rowid)
	if (source.table) {
		std::swap(source.columns[0], source.columns[1]);
	} else {
		source.sql = "SELECT rowid, " + GGQuote(weight_column) + " FROM " + GGQuote(edge_table);
	}
	const auto pairs = GGCollectKeyedValues(context, source, "gg_cheapest_path", column_name);
	int64_t top = -1;
	for (idx_t i = 0; i < pairs.keys.size(); i++) {
		if (!pairs.has[i]) {
			throw InvalidInputException("gg_cheapest_path: " + column_name + " of " + edge_table + " holds a NULL");
		}
		if (pairs.values[i] < 0) {
			throw InvalidInputException("gg_cheapest_path: " + column_name + " of " + edge_table +
			                            " holds a negative weight (" + to_string(pairs.values[i]) + ")");
		}
		if (pairs.keys[i] < 0) {
			throw InternalException("gg_cheapest_path: a negative rowid");
		}
		top = MaxValue<int64_t>(top, pairs.keys[i]);
	}
	vector<int64_t> by_rowid((idx_t)(top + 1), 0);
	for (idx_t i = 0; i < pairs.keys.size(); i++) {
		by_rowid[pairs.keys[i]] = pairs.values[i];
	}
	gg_edge_weights *made = nullptr;
	lock_guard<mutex> guard(graph.lock);
	if (!graph.csr) {
		throw InternalException("gg_cheapest_path: the CSR was not built");
	}
	GGGraph::Check(gg_edge_weights_create(graph.ctx, graph.csr, by_rowid.data(), by_rowid.size(), GG_WEIGHTS_BY_ROWID, &made),
	               "gg_edge_weights_create");
	return GGWeightsPtr(made);
}

unique_ptr<FunctionData> CheapestPathBind(ClientContext &context, vector<Value> &inputs, vector<LogicalType> &return_types,
                                          vector<string> &names, int kind) {
	const GraphArguments args(inputs);
	GGRequireArguments("gg_cheapest_path", inputs, {5}, "weight_column");
	const string weight_column = inputs[5].ToString();
	const string sources_sql = inputs[6].is_null ? string() : inputs[6].ToString();
	const string targets_sql = inputs[7].is_null ? string() : inputs[7].ToString();
	const int64_t max_hops = inputs[8].is_null ? -1 : MaxValue<int64_t>(-1, inputs[8].GetValue<int64_t>());
	auto data = make_unique<GGFunctionData>();
	data->open = [=](ClientContext &ctx, GGOpened &opened) {
		opened.graph = args.Build(ctx, true);
		auto weights = WeightsByRowid(ctx, *opened.graph, args.edge_table, weight_column);
		vector<int64_t> sources, targets;
		if (!sources_sql.empty()) {
			sources = Distinct(GGQueryInt64Column(ctx, sources_sql, "gg_cheapest_path: sources"));
		}
		if (!targets_sql.empty()) {
			targets = GGQueryInt64Column(ctx, targets_sql, "gg_cheapest_path: targets");
		}
		opened.source = make_unique<PhysicalGGCheapestPath>(opened.graph, move(weights), max_hops, move(sources),
		                                                    sources_sql.empty(), move(targets), targets_sql.empty());
	};
	data->parallel_result = true;
	data->description = "cheapest walks of " + (max_hops < 0 ? string("any length") : "at most " + to_string(max_hops) + " hops") +
	                    " over " + args.edge_table + " weighted by " + weight_column;
	return_types = PhysicalGGCheapestPath::OutputTypes();
	names = {"source", "vertex", "cost", "hops"};
	return move(data);
}

unique_ptr<FunctionData> CheapestPathRowsBind(ClientContext &context, vector<Value> &inputs,
                                              vector<LogicalType> &return_types, vector<string> &names, int kind) {
	const GraphArguments args(inputs);
	GGRequireArguments("gg_cheapest_path_rows", inputs, {5, 6}, "weight_column and pairs_sql");
	const string weight_column = inputs[5].ToString(), pairs_sql = inputs[6].ToString();
	auto data = make_unique<GGFunctionData>();
	data->open = [=](ClientContext &ctx, GGOpened &opened) {
		opened.graph = args.Build(ctx, true);
		auto weights = WeightsByRowid(ctx, *opened.graph, args.edge_table, weight_column);
		vector<int64_t> src, dst;
		GGQueryInt64Pairs(ctx, pairs_sql, "gg_cheapest_path_rows: pairs", src, dst);
		opened.source = make_unique<PhysicalGGCheapestPathRows>(opened.graph, move(weights), move(src), move(dst));
	};
	data->parallel_result = true;
	data->description = "cheapest paths over " + args.edge_table + " weighted by " + weight_column;
	return_types = PhysicalGGCheapestPathRows::OutputTypes();
	names = {"src", "dst", "step", "vertex", "edge_rowid", "cost"};
	return move(data);
}

} // namespace

void GGRegisterCheapestFunctions(ClientContext &context) {
	auto rows_args = GraphArguments::Types();
	rows_args.insert(rows_args.end(), {LogicalType::VARCHAR, LogicalType::VARCHAR});
	auto args = rows_args;
	args.insert(args.end(), {LogicalType::VARCHAR, LogicalType::BIGINT});
	GGRegisterTableFunctions(context, {GGScanFunction("gg_cheapest_path", args, GGBind<CheapestPathBind>),
	                                   GGScanFunction("gg_cheapest_path_rows", rows_args, GGBind<CheapestPathRowsBind>)});
}

} // namespace duckdb
