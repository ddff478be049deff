// gg_pair_counts.cpp — count(*) over walks grouped by BOTH ends of the walk, as a table function:
//
//   gg_khop_pair_counts(vertex_table, vertex_key, edge_table, src_col, dst_col,
//                       sources_sql VARCHAR, targets_sql VARCHAR, hops BIGINT)
//        -> (source BIGINT, vertex BIGINT, walks BIGINT)
//
// One row per (source, vertex) pair joined by at least one `hops`-hop walk, with the number of such walks.  The sources
// are the distinct non-NULL values `sources_sql` yields (one integer column), in first-occurrence order — an IN list does
// not multiply; NULL or '': every vertex.  `targets_sql` restricts the end vertices likewise; NULL or '': no restriction.
// What that stands for in the reference is a grouped aggregate on two keys above a join chain,
//     SELECT p0.id, p2.id, count(*) FROM person p0, knows k1, person p1, knows k2, person p2 WHERE ... GROUP BY p0.id, p2.id
// (the pair form of benchmark/ldbc/queries/bi-14.sql:103-112; with hops = 2 over a mirrored knows the mutual-friend count
// behind interactive-complex-10.sql:19-24): PhysicalHashAggregate
// (src/execution/operator/aggregate/physical_hash_aggregate.cpp:152-266) fed by the hash joins' probes
// (ScanStructure::NextInnerJoin, src/execution/join_hashtable.cpp:442-476), every walk row formed to be folded away.  Here
// it is `hops` passes over the reverse CSR per batch of 64 sources (gg_khop_pair_counts, include/gg.h).  walks is the
// library's u64 as a BIGINT, the way gg_khop_aggregate reports its walks column.
// No planner rule recognises the shape.
//
// The graph comes from GGBuildGraph — or is the pinned graph of these tables if the connection asked for pinned graphs.
// One batch of 64 sources is resident at a time: the pipeline's threads drain its rows together (GGResultDrain,
// gg_operators.hpp), and whoever claims the last of them runs the next batch under the graph's lock.
#include <unordered_set>

#include "gg_table_function.hpp"

namespace duckdb {

namespace {

class PairCountsState : public GlobalSourceState {
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

class PhysicalGGKhopPairCounts : public GGResultSource {
public:
	PhysicalGGKhopPairCounts(shared_ptr<GGGraph> graph_p, int hops_p, vector<int64_t> sources_p, bool all_sources_p,
	                         vector<int64_t> targets_p, bool all_targets_p)
	    : GGResultSource(OutputTypes(), move(graph_p)), hops(hops_p), sources(move(sources_p)), all_sources(all_sources_p),
	      targets(move(targets_p)), all_targets(all_targets_p) {
	}
	static vector<LogicalType> OutputTypes() {
		return {LogicalType::BIGINT, LogicalType::BIGINT, LogicalType::BIGINT};
	}

	int hops;
	vector<int64_t> sources; // distinct (ignored if all_sources)
	bool all_sources;
	vector<int64_t> targets; // (ignored if all_targets)
	bool all_targets;

	//! the pair counts of the batch starting at source batch_base; caller holds graph->lock
	GGResultPtr RunBatch(PairCountsState &state, idx_t batch_base, idx_t &rows) const {
		const int n = (int)MinValue<idx_t>(GG_BFS_LANES, state.uniq.size() - batch_base);
		const int64_t *dst = all_targets ? nullptr : GGSourceIds(targets);
		gg_pair_stats stats {};
		GGResultPtr owner;
		GGGraph::Check(gg_khop_pair_counts(graph->ctx, graph->csr, state.uniq.data() + batch_base, n, hops, hops, dst,
		                                   all_targets ? 0 : targets.size(), &stats, GGResultOut(owner)),
		               "gg_khop_pair_counts");
		rows = stats.pairs[hops];
		return owner;
	}

	unique_ptr<GlobalSourceState> GetGlobalSourceState(ClientContext &context) const override {
		auto state = make_unique<PairCountsState>();
		lock_guard<mutex> guard(graph->lock);
		if (!graph->csr) {
			throw InternalException("GG_KHOP_PAIR_COUNTS scheduled before the CSR was built");
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
		auto &gstate = (PairCountsState &)gstate_p;
		auto &slab = (GGResultSlab &)lstate;
		PollInterrupt(context);
		if (slab.pos >= slab.rows) {
			auto &drain = gstate.drain;
			auto advance = [&]() -> bool { // current batch claimed completely: run the next one
				const idx_t next = (idx_t)drain.Table() + GG_BFS_LANES;
				if (next >= gstate.uniq.size()) {
					return false;
				}
				// (the drain's lock stays held through the passes on purpose: the other threads have nothing to claim
				// until the next batch's rows exist)
				drain.Replace(context.client, (int)next, [&](idx_t &rows) {
					lock_guard<mutex> device_guard(graph->lock);
					return RunBatch(gstate, next, rows);
				});
				return true;
			};
			const int level = hops;
			auto fetch = [level](gg_result *result, int, idx_t offset, uint32_t want, GGResultSlab &slab) {
				uint32_t got = 0;
				auto columns = slab.Columns(3); // vertex id, walks, then the source's index in its batch
				GGGraph::Check(gg_khop_pair_counts_fetch(result, level, offset, want, columns[2], columns[0],
				                                         (uint64_t *)columns[1], &got),
				               "gg_khop_pair_counts_fetch");
				return got;
			};
			if (!drain.Refill(slab, advance, fetch)) { // (lane i of a slab's rows is source uniq[slab.table + i])
				return;
			}
		}
		const idx_t first = slab.pos;
		const idx_t n = slab.Emit(chunk, 1, 2);
		auto source = FlatVector::GetData<int64_t>(chunk.data[0]);
		const int64_t *lane_source = gstate.uniq.data() + slab.table;
		for (idx_t i = 0; i < n; i++) {
			source[i] = lane_source[slab.column[2][first + i]];
		}
	}

	string GetName() const override {
		return "GG_KHOP_PAIR_COUNTS";
	}
};

unique_ptr<FunctionData> KhopPairCountsBind(ClientContext &context, vector<Value> &inputs, vector<LogicalType> &return_types,
                                            vector<string> &names, int kind) {
	const string fn = "gg_khop_pair_counts";
	const GraphArguments args(inputs);
	const string sources_sql = inputs[5].is_null ? string() : inputs[5].ToString();
	const string targets_sql = inputs[6].is_null ? string() : inputs[6].ToString();
	GGRequireArguments(fn, inputs, {7}, "hops");
	const auto hops = GGHopsArgument(fn, inputs[7], GG_MAX_HOPS);
	auto data = make_unique<GGFunctionData>();
	data->open = [=](ClientContext &ctx, GGOpened &opened) {
		opened.graph = args.Build(ctx);
		vector<int64_t> sources, targets;
		if (!sources_sql.empty()) {
			sources = Distinct(GGQueryInt64Column(ctx, sources_sql, "gg_khop_pair_counts: sources"));
		}
		if (!targets_sql.empty()) {
			targets = GGQueryInt64Column(ctx, targets_sql, "gg_khop_pair_counts: targets");
		}
		opened.source = make_unique<PhysicalGGKhopPairCounts>(opened.graph, (int)hops, move(sources), sources_sql.empty(),
		                                                      move(targets), targets_sql.empty());
	};
	data->parallel_result = true;
	data->description = "count by (source, end) over " + to_string(hops) + "-hop walks of " + args.edge_table;
	return_types = PhysicalGGKhopPairCounts::OutputTypes();
	names = {"source", "vertex", "walks"};
	return move(data);
}

} // namespace

void GGRegisterPairCountFunctions(ClientContext &context) {
	auto args = GraphArguments::Types();
	args.insert(args.end(), {LogicalType::VARCHAR, LogicalType::VARCHAR, LogicalType::BIGINT});
	GGRegisterTableFunctions(context, {GGScanFunction("gg_khop_pair_counts", args, GGBind<KhopPairCountsBind>)});
}

} // namespace duckdb
