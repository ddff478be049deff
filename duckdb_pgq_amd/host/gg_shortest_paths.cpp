// gg_shortest_paths.cpp — the shortest paths themselves as rows: (src, dst, step, vertex, edge_rowid).
//
// The reference has no relation for this: benchmark/ldbc/queries/bi-10-shortestpath.sql:26-31 stops at min(hopCount).
// With its operators a path is read backwards by one hash join of friends_shortest with knows per step
// (PhysicalHashJoin::Execute, src/execution/operator/join/physical_hash_join.cpp:217-254) under a min(rowid) aggregate
// (src/execution/operator/aggregate/physical_hash_aggregate.cpp:152-266).  Here gg_bfs64_paths reads the paths off the
// distances of a 64-source BFS batch while they are still on the device (include/gg.h pins WHICH shortest path: the
// predecessor with the smallest vertex-table position, among parallel edges the one appended first).
//
// Pairs are grouped by source, 64 distinct sources to a batch, in the order the sources first occur; one batch's rows are
// resident at a time and the pipeline's threads drain them together, each through its own page-locked slab
// (GGResultDrain, gg_operators.hpp).  Rows of one pair arrive in step order inside a slab, pairs in no promised order.
//
// PhysicalGGAllShortestPaths beside it is ALL SHORTEST and its count: (src, dst, path, step, vertex, edge_rowid) for every
// shortest path of every pair, or (src, dst, hops, paths).  With the reference's operators that is a recursive UNION ALL CTE
// over friends_shortest joined with knows once per level (src/execution/operator/set/physical_recursive_cte.cpp:60-139,
// src/execution/join_hashtable.cpp:304-476) and a hash aggregate above it for the count; here gg_bfs64_all_paths counts the
// paths over the shortest-path DAG and unranks them on the device (include/gg.h pins their order).  The same batching, the
// same drain; in count mode the drained table is the batch's pair table.
#include "duckdb.hpp"
#include "duckdb/common/exception.hpp"
#include "duckdb/main/client_context.hpp"

#include "gg_extension.hpp"
#include "gg_operators.hpp"

namespace duckdb {

PhysicalGGShortestPathRows::PhysicalGGShortestPathRows(shared_ptr<GGGraph> graph_p, vector<int64_t> src_p,
                                                       vector<int64_t> dst_p, int max_hops_p,
                                                       idx_t estimated_cardinality)
    : PhysicalOperator(PhysicalOperatorType::INVALID, OutputTypes(), estimated_cardinality), graph(move(graph_p)),
      src(move(src_p)), dst(move(dst_p)), max_hops(max_hops_p) {
	D_ASSERT(src.size() == dst.size());
}

vector<LogicalType> PhysicalGGShortestPathRows::OutputTypes() {
	return {LogicalType::BIGINT, LogicalType::BIGINT, LogicalType::INTEGER, LogicalType::BIGINT, LogicalType::BIGINT};
}

//! Trace the pairs of a batch; the rows stay on the device until the pipeline threads have fetched them.
GGResultPtr PhysicalGGShortestPathRows::RunBatch(GlobalSourceState &gstate_p, idx_t batch, idx_t &rows) const {
	auto &state = (ShortestPathRowsState &)gstate_p;
	const idx_t base = batch * GG_BFS_LANES;
	const int n = (int)MinValue<idx_t>(GG_BFS_LANES, state.uniq.size() - base);
	auto &members = state.members[batch];
	vector<int64_t> targets(members.size());
	for (idx_t i = 0; i < members.size(); i++) {
		targets[i] = dst[members[i]];
	}
	GGResultPtr owner;
	GGGraph::Check(gg_bfs64_paths(graph->ctx, graph->csr, state.uniq.data() + base, n, max_hops,
	                              state.lanes[batch].data(), targets.data(), targets.size(), 1, nullptr,
	                              GGResultOut(owner)),
	               "gg_bfs64_paths");
	uint64_t n_rows = 0;
	GGGraph::Check(gg_bfs64_paths_rows(owner.get(), &n_rows), "gg_bfs64_paths_rows");
	rows = n_rows;
	return owner;
}

unique_ptr<GlobalSourceState> PhysicalGGShortestPathRows::GetGlobalSourceState(ClientContext &context) const {
	auto state = make_unique<ShortestPathRowsState>();
	lock_guard<mutex> guard(graph->lock);
	if (!graph->csr) {
		throw InternalException("GG_SHORTEST_PATH_ROWS scheduled before the CSR was built");
	}
	state->Group(src);
	if (!state->members.empty()) {
		state->drain.Replace(context, 0, [&](idx_t &rows) { return RunBatch(*state, 0, rows); });
	}
	// the first batch's size is the only estimate there is of how much the threads will have to drain
	state->max_threads = GGResultSlab::ThreadsFor(state->drain.Rows() * state->members.size());
	return move(state);
}

unique_ptr<LocalSourceState> PhysicalGGShortestPathRows::GetLocalSourceState(ExecutionContext &context,
                                                                             GlobalSourceState &gstate) const {
	return make_unique<GGResultSlab>(graph);
}

void PhysicalGGShortestPathRows::GetData(ExecutionContext &context, DataChunk &chunk, GlobalSourceState &gstate_p,
                                         LocalSourceState &lstate) const {
	auto &gstate = (ShortestPathRowsState &)gstate_p;
	auto &slab = (GGResultSlab &)lstate;
	if (context.client.interrupted) {
		throw InterruptException();
	}
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
			// (the drain's lock stays held through RunBatch on purpose: the other threads have nothing to claim until
			// the next batch's rows exist)
			drain.Replace(context.client, (int)next, [&](idx_t &rows) {
				lock_guard<mutex> device_guard(graph->lock);
				return RunBatch(gstate, next, rows);
			});
			return true;
		};
		auto fetch = [](gg_result *result, int, idx_t offset, uint32_t want, GGResultSlab &slab) {
			// columns 0..2: pair, vertex, edge rowid; column 3's memory holds the int32 steps
			auto columns = slab.Columns(4);
			uint32_t got = 0;
			GGGraph::Check(gg_bfs64_paths_fetch(result, offset, want, columns[0], (int32_t *)columns[3], columns[1],
			                                    columns[2], &got),
			               "gg_bfs64_paths_fetch");
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
	auto &edge_validity = FlatVector::Validity(chunk.data[4]);
	auto &members = gstate.members[slab.table]; // (filled before the first batch ran; never changed afterwards)
	const int64_t *pair = slab.column[0] + slab.pos, *vertex = slab.column[1] + slab.pos;
	const int64_t *edge = slab.column[2] + slab.pos;
	const int32_t *step = (const int32_t *)slab.column[3] + slab.pos;
	for (idx_t i = 0; i < n; i++) {
		const idx_t p = members[(idx_t)pair[i]];
		out_src[i] = src[p];
		out_dst[i] = dst[p];
		out_step[i] = step[i];
		out_vertex[i] = vertex[i];
		out_edge[i] = edge[i];
		if (step[i] == 0) { // no edge leads into the path's first vertex
			edge_validity.SetInvalid(i);
		}
	}
	slab.pos += n;
	chunk.SetCardinality(n);
}

// ---- ALL SHORTEST and its count

PhysicalGGAllShortestPaths::PhysicalGGAllShortestPaths(shared_ptr<GGGraph> graph_p, vector<int64_t> src_p,
                                                       vector<int64_t> dst_p, int max_hops_p, uint64_t path_limit_p,
                                                       bool count_only_p, idx_t estimated_cardinality)
    : PhysicalOperator(PhysicalOperatorType::INVALID, OutputTypes(count_only_p), estimated_cardinality),
      graph(move(graph_p)), src(move(src_p)), dst(move(dst_p)), max_hops(max_hops_p), path_limit(path_limit_p),
      count_only(count_only_p) {
	D_ASSERT(src.size() == dst.size());
}

vector<LogicalType> PhysicalGGAllShortestPaths::OutputTypes(bool count_only) {
	if (count_only) {
		return {LogicalType::BIGINT, LogicalType::BIGINT, LogicalType::INTEGER, LogicalType::HUGEINT};
	}
	return {LogicalType::BIGINT, LogicalType::BIGINT, LogicalType::BIGINT,
	        LogicalType::INTEGER, LogicalType::BIGINT, LogicalType::BIGINT};
}

//! Count (and unrank) the shortest paths of a batch's pairs; the rows stay on the device until the threads fetched them.
GGResultPtr PhysicalGGAllShortestPaths::RunBatch(GlobalSourceState &gstate_p, idx_t batch, idx_t &rows) const {
	auto &state = (ShortestPathRowsState &)gstate_p;
	const idx_t base = batch * GG_BFS_LANES;
	const int n = (int)MinValue<idx_t>(GG_BFS_LANES, state.uniq.size() - base);
	auto &members = state.members[batch];
	vector<int64_t> targets(members.size());
	for (idx_t i = 0; i < members.size(); i++) {
		targets[i] = dst[members[i]];
	}
	GGResultPtr owner;
	GGGraph::Check(gg_bfs64_all_paths(graph->ctx, graph->csr, state.uniq.data() + base, n, max_hops,
	                                  state.lanes[batch].data(), targets.data(), targets.size(), path_limit, 1,
	                                  count_only ? 0 : 1, nullptr, GGResultOut(owner)),
	               "gg_bfs64_all_paths");
	uint64_t n_rows = 0;
	GGGraph::Check(gg_bfs64_all_paths_rows(owner.get(), count_only ? 0 : 1, &n_rows), "gg_bfs64_all_paths_rows");
	rows = n_rows;
	return owner;
}

unique_ptr<GlobalSourceState> PhysicalGGAllShortestPaths::GetGlobalSourceState(ClientContext &context) const {
	auto state = make_unique<ShortestPathRowsState>();
	lock_guard<mutex> guard(graph->lock);
	if (!graph->csr) {
		throw InternalException("GG_ALL_SHORTEST_PATHS scheduled before the CSR was built");
	}
	state->Group(src);
	if (!state->members.empty()) {
		state->drain.Replace(context, 0, [&](idx_t &rows) { return RunBatch(*state, 0, rows); });
	}
	state->max_threads = GGResultSlab::ThreadsFor(state->drain.Rows() * state->members.size());
	return move(state);
}

unique_ptr<LocalSourceState> PhysicalGGAllShortestPaths::GetLocalSourceState(ExecutionContext &context,
                                                                             GlobalSourceState &gstate) const {
	return make_unique<GGResultSlab>(graph);
}

void PhysicalGGAllShortestPaths::GetData(ExecutionContext &context, DataChunk &chunk, GlobalSourceState &gstate_p,
                                         LocalSourceState &lstate) const {
	auto &gstate = (ShortestPathRowsState &)gstate_p;
	auto &slab = (GGResultSlab &)lstate;
	if (context.client.interrupted) {
		throw InterruptException();
	}
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
			drain.Replace(context.client, (int)next, [&](idx_t &rows) {
				lock_guard<mutex> device_guard(graph->lock);
				return RunBatch(gstate, next, rows);
			});
			return true;
		};
		const bool counts = count_only;
		auto fetch = [counts](gg_result *result, int, idx_t offset, uint32_t want, GGResultSlab &slab) {
			uint32_t got = 0;
			if (counts) { // columns 0, 1: pair, paths; column 2's memory holds the int32 hops
				auto columns = slab.Columns(3);
				GGGraph::Check(gg_bfs64_all_paths_fetch_pairs(result, offset, want, columns[0], (int32_t *)columns[2],
				                                              (uint64_t *)columns[1], nullptr, &got),
				               "gg_bfs64_all_paths_fetch_pairs");
			} else { // columns 0..3: pair, path, vertex, edge rowid; column 4's memory holds the int32 steps
				auto columns = slab.Columns(5);
				GGGraph::Check(gg_bfs64_all_paths_fetch(result, offset, want, columns[0], columns[1],
				                                        (int32_t *)columns[4], columns[2], columns[3], &got),
				               "gg_bfs64_all_paths_fetch");
			}
			return got;
		};
		if (!drain.Refill(slab, advance, fetch)) { // (pair i of a slab's rows is members[slab.table][i])
			return;
		}
	}
	const idx_t n = MinValue<idx_t>(STANDARD_VECTOR_SIZE, slab.rows - slab.pos);
	auto out_src = FlatVector::GetData<int64_t>(chunk.data[0]);
	auto out_dst = FlatVector::GetData<int64_t>(chunk.data[1]);
	auto &members = gstate.members[slab.table]; // (filled before the first batch ran; never changed afterwards)
	const int64_t *pair = slab.column[0] + slab.pos;
	for (idx_t i = 0; i < n; i++) {
		const idx_t p = members[(idx_t)pair[i]];
		out_src[i] = src[p];
		out_dst[i] = dst[p];
	}
	if (count_only) {
		auto out_hops = FlatVector::GetData<int32_t>(chunk.data[2]);
		auto out_paths = FlatVector::GetData<hugeint_t>(chunk.data[3]);
		const uint64_t *paths = (const uint64_t *)slab.column[1] + slab.pos;
		const int32_t *hops = (const int32_t *)slab.column[2] + slab.pos;
		for (idx_t i = 0; i < n; i++) {
			out_hops[i] = hops[i];
			out_paths[i].lower = paths[i]; // (2^64 - 1 stands for that many or more)
			out_paths[i].upper = 0;
		}
	} else {
		auto out_path = FlatVector::GetData<int64_t>(chunk.data[2]);
		auto out_step = FlatVector::GetData<int32_t>(chunk.data[3]);
		auto out_vertex = FlatVector::GetData<int64_t>(chunk.data[4]);
		auto out_edge = FlatVector::GetData<int64_t>(chunk.data[5]);
		auto &edge_validity = FlatVector::Validity(chunk.data[5]);
		const int64_t *path = slab.column[1] + slab.pos, *vertex = slab.column[2] + slab.pos;
		const int64_t *edge = slab.column[3] + slab.pos;
		const int32_t *step = (const int32_t *)slab.column[4] + slab.pos;
		for (idx_t i = 0; i < n; i++) {
			out_path[i] = path[i];
			out_step[i] = step[i];
			out_vertex[i] = vertex[i];
			out_edge[i] = edge[i];
			if (step[i] == 0) { // no edge leads into the path's first vertex
				edge_validity.SetInvalid(i);
			}
		}
	}
	slab.pos += n;
	chunk.SetCardinality(n);
}

} // namespace duckdb
