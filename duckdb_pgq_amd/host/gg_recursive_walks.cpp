// gg_recursive_walks.cpp — a UNION ALL recursive CTE over one keyed table as one device walk closure.
//
// benchmark/ldbc/queries/bi-9.sql (post_all) and interactive-short-6.sql (chain) recurse as
//     anchor  UNION ALL  SELECT <carried cte columns, T columns, constants, cte.counter + c> FROM T, cte
//                        WHERE T.key = cte.link [AND cte.counter < K]
// with the arm's column at the link's position a column of T (the next link).  The reference runs
// PhysicalRecursiveCTE: the arm's pipeline, hash-join build over T included, once per level
// (src/execution/operator/set/physical_recursive_cte.cpp:60-139).  Here both inputs are pipeline sinks
// (gg_pipeline.cpp): the anchor's rows and T's rows are kept on the host, T's rows go to the device as edges
// key -> next with their row number as rowid, and gg_walk_closure returns every walk (seed row, last edge's row,
// level).  Each output row gathers its carried columns from its seed's anchor row and its T columns from its edge's
// row — the same rows the reference's UNION ALL emits, anchor rows first, then level by level.
//
// NULLs as the reference's join treats them: a T row with a NULL key joins nothing (no edge); a NULL next is staged
// as a sentinel id that is neither a key nor an anchor link (a vertex without out-edges: the row is emitted, never
// expanded); an anchor row with a NULL link seeds nothing.
#include <algorithm>
#include <limits>

#include "duckdb.hpp"
#include "duckdb/common/types/chunk_collection.hpp"
#include "duckdb/common/vector_operations/vector_operations.hpp"

#include "gg_extension.hpp"
#include "gg_operators.hpp"
#include "gg_pipeline.hpp"

namespace duckdb {

//! column `col` of every row of `rows` as int64 (NULL: valid[r] = false)
void GGIntegerColumn(ChunkCollection &rows, idx_t col, vector<int64_t> &out, vector<bool> &valid) {
	out.clear();
	valid.clear();
	out.reserve(rows.Count());
	valid.reserve(rows.Count());
	for (idx_t c = 0; c < rows.ChunkCount(); c++) {
		auto &chunk = rows.GetChunk(c);
		Vector cast(LogicalType::BIGINT);
		VectorOperations::Cast(chunk.data[col], cast, chunk.size());
		VectorData data;
		cast.Orrify(chunk.size(), data);
		auto values = (const int64_t *)data.data;
		for (idx_t r = 0; r < chunk.size(); r++) {
			auto at = data.sel->get_index(r);
			valid.push_back(data.validity.RowIsValid(at));
			out.push_back(valid.back() ? values[at] : 0);
		}
	}
}

namespace {

class RowSinkState : public GlobalSinkState {};

} // namespace

PhysicalGGWalkRowSink::PhysicalGGWalkRowSink(shared_ptr<GGWalkInput> input_p, shared_ptr<GGGraphSlot> slot_p,
                                             bool table_side_p, vector<LogicalType> types, idx_t estimated_cardinality)
    : PhysicalOperator(PhysicalOperatorType::INVALID, move(types), estimated_cardinality), input(move(input_p)),
      slot(move(slot_p)), table_side(table_side_p) {
}

unique_ptr<GlobalSinkState> PhysicalGGWalkRowSink::GetGlobalSinkState(ClientContext &context) const {
	lock_guard<mutex> guard(input->lock);
	(table_side ? input->table : input->anchor).Reset(); // (a prepared plan executed again)
	return make_unique<RowSinkState>();
}

SinkResultType PhysicalGGWalkRowSink::Sink(ExecutionContext &context, GlobalSinkState &gstate, LocalSinkState &lstate,
                                           DataChunk &chunk) const {
	lock_guard<mutex> guard(input->lock);
	(table_side ? input->table : input->anchor).Append(chunk);
	return SinkResultType::NEED_MORE_INPUT;
}

SinkFinalizeType PhysicalGGWalkRowSink::Finalize(Pipeline &pipeline, Event &event, ClientContext &context,
                                                 GlobalSinkState &gstate) const {
	if (!table_side) {
		return SinkFinalizeType::READY;
	}
	// the anchor's sink ran first (its pipeline is a dependency of this one): the sentinel avoids its links too, and the
	// next values (GG_RECURSIVE_REACH emits the vertex a row reached, so a real next must never be the sentinel)
	lock_guard<mutex> guard(input->lock);
	vector<int64_t> key, next, link;
	vector<bool> key_valid, next_valid, link_valid;
	GGIntegerColumn(input->table, input->key_column, key, key_valid);
	GGIntegerColumn(input->table, input->next_column, next, next_valid);
	GGIntegerColumn(input->anchor, input->link_column, link, link_valid);
	int64_t lo = std::numeric_limits<int64_t>::max(), hi = std::numeric_limits<int64_t>::min();
	for (idx_t r = 0; r < key.size(); r++) {
		if (key_valid[r]) {
			lo = std::min(lo, key[r]);
			hi = std::max(hi, key[r]);
		}
	}
	for (idx_t r = 0; r < link.size(); r++) {
		if (link_valid[r]) {
			lo = std::min(lo, link[r]);
			hi = std::max(hi, link[r]);
		}
	}
	for (idx_t r = 0; r < next.size(); r++) {
		if (next_valid[r]) {
			lo = std::min(lo, next[r]);
			hi = std::max(hi, next[r]);
		}
	}
	int64_t sentinel = 0;
	if (lo <= hi) {
		if (lo > std::numeric_limits<int64_t>::min()) {
			sentinel = lo - 1;
		} else if (hi < std::numeric_limits<int64_t>::max()) {
			sentinel = hi + 1;
		} else {
			throw NotImplementedException("GG_RECURSIVE_WALKS: keys and links span every BIGINT value");
		}
	}
	vector<int64_t> src, dst, rowid;
	for (idx_t r = 0; r < key.size(); r++) {
		if (!key_valid[r]) {
			continue; // a NULL key joins nothing
		}
		src.push_back(key[r]);
		dst.push_back(next_valid[r] ? next[r] : sentinel);
		rowid.push_back((int64_t)r);
	}
	input->sentinel = sentinel;
	input->has_edges = !src.empty();
	if (src.empty()) { // a graph needs an edge: one that no seed reaches (the sentinel is no link)
		src.push_back(sentinel);
		dst.push_back(sentinel);
		rowid.push_back(0);
	}
	auto graph = make_shared<GGGraph>(0, true);
	lock_guard<std::mutex> graph_guard(graph->lock);
	GGGraph::Check(gg_ctx_set_edge_rowid(graph->ctx, 1), "gg_ctx_set_edge_rowid");
	GGGraph::Check(gg_edges_append(graph->ctx, src.data(), dst.data(), rowid.data(), src.size()), "gg_edges_append");
	GGGraph::Check(gg_vertices_from_edges(graph->ctx, 0, nullptr), "gg_vertices_from_edges");
	GGGraph::Check(gg_csr_build(graph->ctx, &graph->csr), "gg_csr_build");
	lock_guard<mutex> slot_guard(slot->lock);
	slot->graph = graph;
	return SinkFinalizeType::READY;
}

string PhysicalGGWalkRowSink::GetName() const {
	return table_side ? "GG_WALK_TABLE_SINK" : "GG_WALK_ANCHOR_SINK";
}

//===--------------------------------------------------------------------===//
// The source
//===--------------------------------------------------------------------===//
PhysicalGGRecursiveWalks::PhysicalGGRecursiveWalks(vector<LogicalType> types, shared_ptr<GGGraph> graph_p,
                                                   shared_ptr<GGWalkInput> input_p, idx_t estimated_cardinality)
    : PhysicalOperator(PhysicalOperatorType::INVALID, move(types), estimated_cardinality), graph(move(graph_p)),
      input(move(input_p)) {
}

namespace {
class RecursiveWalksState : public GlobalSourceState {
public:
	vector<int64_t> seed_row; // anchor row of every seed
	vector<int64_t> seed, rowid;
	vector<int32_t> level;
	idx_t anchor_chunk = 0; // next anchor chunk to emit
	idx_t next_row = 0;     // next walk row to emit
};
} // namespace

unique_ptr<GlobalSourceState> PhysicalGGRecursiveWalks::GetGlobalSourceState(ClientContext &context) const {
	auto state = make_unique<RecursiveWalksState>();
	vector<int64_t> link;
	vector<bool> valid;
	{
		lock_guard<mutex> guard(input->lock);
		GGIntegerColumn(input->anchor, input->link_column, link, valid);
	}
	vector<int64_t> seeds;
	for (idx_t r = 0; r < link.size(); r++) {
		if (valid[r]) { // a NULL link seeds nothing
			seeds.push_back(link[r]);
			state->seed_row.push_back((int64_t)r);
		}
	}
	lock_guard<std::mutex> guard(graph->lock);
	GGResultPtr owner;
	GGGraph::Check(gg_walk_closure(graph->ctx, graph->csr, seeds.data(), seeds.size(), input->max_levels,
	                               GGResultOut(owner)),
	               "gg_walk_closure");
	gg_result *res = owner.get();
	int n_levels = 0;
	GGGraph::Check(gg_walk_closure_levels(res, nullptr, 0, &n_levels), "gg_walk_closure_levels");
	vector<uint64_t> per_level(MaxValue<int>(n_levels, 1));
	GGGraph::Check(gg_walk_closure_levels(res, per_level.data(), n_levels, &n_levels), "gg_walk_closure_levels");
	uint64_t total = 0;
	for (int l = 0; l < n_levels; l++) {
		total += per_level[l];
	}
	state->seed.resize(total);
	state->rowid.resize(total);
	state->level.resize(total);
	for (uint64_t at = 0; at < total;) {
		uint32_t got = 0;
		const uint32_t want = (uint32_t)MinValue<uint64_t>(total - at, 1u << 24);
		GGGraph::Check(gg_walk_closure_fetch(res, at, want, state->seed.data() + at, state->rowid.data() + at,
		                                     state->level.data() + at, &got),
		               "gg_walk_closure_fetch");
		if (got == 0) {
			throw InternalException("gg_walk_closure_fetch returned no rows");
		}
		at += got;
	}
	return move(state);
}

//! target[i] = column `col` of row row[i] of `rows`, i < n: one vectorised copy per run of consecutive output rows whose
//! source rows lie in one chunk of the collection (a chunk holds STANDARD_VECTOR_SIZE rows, ChunkCollection::LocateChunk)
void GGGatherRows(ChunkCollection &rows, idx_t col, const idx_t *row, idx_t n, Vector &target) {
	SelectionVector sel(STANDARD_VECTOR_SIZE);
	for (idx_t i = 0; i < n;) {
		const idx_t chunk = row[i] / STANDARD_VECTOR_SIZE;
		idx_t j = i;
		for (; j < n && row[j] / STANDARD_VECTOR_SIZE == chunk; j++) {
			sel.set_index(j - i, row[j] % STANDARD_VECTOR_SIZE);
		}
		VectorOperations::Copy(rows.GetChunk(chunk).data[col], target, sel, j - i, 0, i);
		i = j;
	}
}

void PhysicalGGRecursiveWalks::GetData(ExecutionContext &context, DataChunk &chunk, GlobalSourceState &gstate_p,
                                       LocalSourceState &lstate) const {
	auto &state = (RecursiveWalksState &)gstate_p;
	lock_guard<mutex> guard(input->lock);
	if (state.anchor_chunk < input->anchor.ChunkCount()) { // the anchor's rows first, as UNION ALL has them
		chunk.Reference(input->anchor.GetChunk(state.anchor_chunk++));
		return;
	}
	const idx_t n = MinValue<idx_t>(STANDARD_VECTOR_SIZE, state.seed.size() - state.next_row);
	if (n == 0) {
		chunk.SetCardinality(0);
		return;
	}
	idx_t anchor_row[STANDARD_VECTOR_SIZE], table_row[STANDARD_VECTOR_SIZE];
	for (idx_t i = 0; i < n; i++) {
		const idx_t w = state.next_row + i;
		anchor_row[i] = (idx_t)state.seed_row[state.seed[w]];
		table_row[i] = (idx_t)state.rowid[w];
	}
	for (idx_t c = 0; c < input->columns.size(); c++) {
		auto &spec = input->columns[c];
		switch (spec.kind) {
		case GGWalkColumn::CARRIED:
			GGGatherRows(input->anchor, c, anchor_row, n, chunk.data[c]);
			break;
		case GGWalkColumn::TABLE:
			GGGatherRows(input->table, spec.index, table_row, n, chunk.data[c]);
			break;
		case GGWalkColumn::CONSTANT:
			chunk.data[c].Reference(spec.constant);
			break;
		case GGWalkColumn::COUNTER: { // the anchor's value + step x level, computed in BIGINT
			Vector start(types[c]), wide(LogicalType::BIGINT);
			GGGatherRows(input->anchor, c, anchor_row, n, start);
			VectorOperations::Cast(start, wide, n);
			auto values = FlatVector::GetData<int64_t>(wide);
			for (idx_t i = 0; i < n; i++) {
				values[i] += spec.step * state.level[state.next_row + i];
			}
			VectorOperations::Cast(wide, chunk.data[c], n);
			break;
		}
		}
	}
	state.next_row += n;
	chunk.SetCardinality(n);
}

string PhysicalGGRecursiveWalks::ParamsToString() const {
	return input->description;
}

} // namespace duckdb
