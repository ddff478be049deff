// gg_recursive_levels.cpp — a UNION recursive CTE with a depth counter over one keyed table as device level sets.
//
// "Everybody within K hops, and at which hop counts" (the friends(startPerson, hopCount, friend) CTE that
// benchmark/ldbc/queries/bi-10-shortestpath.sql:8-25 opens with) recurses as
//     anchor  UNION  SELECT <carried cte columns, T.next at the link's position, constants, counter + step>
//                    FROM T, cte WHERE T.key = cte.link [AND counter < K]
// The reference runs PhysicalRecursiveCTE with union_all == false: the arm's pipeline, hash-join build over T included,
// once per level, every produced row probed against a GroupedAggregateHashTable of all rows emitted so far
// (src/execution/operator/set/physical_recursive_cte.cpp:47-70 ProbeHT / Sink, :75-139).  A counter's anchor value is
// a constant and its step is positive (the rule checks both), so a row of level L carries start + step * L and differs
// from every row of another level, the anchor's (level 0) included: that hash table only ever removes duplicates inside
// a level.  An arm row is (C(parent), next, K_arm, start + step * L): level L is the set of (class, vertex) that L edges
// of T lead to from the anchor rows' (class, link), the class a distinct C of the anchor rows (gg_level_sets).  Here, on
// the host and exactly as the reference's hash table compares rows (NULL equal to NULL):
//   - the anchor rows are deduplicated (the reference's Sink deduplicates the anchor as well);
//   - classes are the distinct C of the distinct anchor rows; seeds are the distinct (class, link).
// There are no seen flags as in gg_recursive_reach.cpp: an arm row never equals an anchor row.
// The rows: the distinct anchor rows, then level by level the level sets' members, carried columns gathered from the
// class's first anchor row, the link as the vertex id cast to the CTE column's type, the arm's constants, every counter
// start + step * L in its column's type (the rule declined if that could overflow within the bound).
//
// NULLs as in gg_recursive_reach.cpp: a NULL next is the sentinel vertex, a member of its level that is never expanded; an
// anchor row with a NULL link seeds the sentinel and so contributes nothing.
#include "duckdb.hpp"
#include "duckdb/common/types/chunk_collection.hpp"
#include "duckdb/common/vector_operations/vector_operations.hpp"

#include <algorithm>

#include "gg_extension.hpp"
#include "gg_operators.hpp"
#include "gg_pipeline.hpp"

namespace duckdb {

PhysicalGGRecursiveLevels::PhysicalGGRecursiveLevels(vector<LogicalType> types, shared_ptr<GGGraph> graph_p,
                                                     shared_ptr<GGWalkInput> input_p, idx_t estimated_cardinality)
    : PhysicalOperator(PhysicalOperatorType::INVALID, move(types), estimated_cardinality), graph(move(graph_p)),
      input(move(input_p)) {
}

namespace {

class RecursiveLevelsState : public GlobalSourceState {
public:
	ChunkCollection distinct;  // the distinct anchor rows, in their first occurrence's order
	vector<idx_t> class_row;   // class -> its first distinct anchor row
	vector<int64_t> row_class; // level-set row -> class
	vector<int64_t> vertex;    // level-set row -> vertex id
	vector<uint64_t> level_end; // level_end[L - 1]: one past the last row of level L
	idx_t distinct_chunk = 0;  // next distinct anchor chunk to emit
	idx_t next_row = 0;        // next level-set row to emit
	idx_t next_level = 1;      // its level
};

} // namespace

unique_ptr<GlobalSourceState> PhysicalGGRecursiveLevels::GetGlobalSourceState(ClientContext &context) const {
	auto state = make_unique<RecursiveLevelsState>();
	vector<idx_t> carried;
	vector<LogicalType> carried_types;
	for (idx_t c = 0; c < input->columns.size(); c++) {
		if (input->columns[c].kind == GGWalkColumn::CARRIED) {
			carried.push_back(c);
			carried_types.push_back(types[c]);
		}
	}
	lock_guard<mutex> guard(input->lock);
	GGDistinctRows(context, input->anchor, types, state->distinct);
	vector<uint32_t> anchor_class;
	GGRowClasses(context, state->distinct, carried, carried_types, anchor_class, state->class_row);
	if (!input->has_edges || state->distinct.Count() == 0 || input->max_levels == 0) {
		return move(state); // no edge, no anchor row or `counter < start`: the anchor alone, and no device call
	}
	// ---- seeds: the distinct (class, link) of the distinct anchor rows (NULL link: the sentinel)
	vector<int64_t> links;
	vector<bool> valid;
	GGIntegerColumn(state->distinct, input->link_column, links, valid);
	vector<std::pair<uint32_t, int64_t>> pairs(links.size());
	for (idx_t r = 0; r < links.size(); r++) {
		pairs[r] = std::make_pair(anchor_class[r], valid[r] ? links[r] : input->sentinel);
	}
	std::sort(pairs.begin(), pairs.end());
	pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
	vector<int64_t> seeds(pairs.size());
	vector<uint32_t> seed_class(pairs.size());
	for (idx_t i = 0; i < pairs.size(); i++) {
		seed_class[i] = pairs[i].first;
		seeds[i] = pairs[i].second;
	}
	lock_guard<std::mutex> graph_guard(graph->lock);
	GGResultPtr owner;
	GGGraph::Check(gg_level_sets(graph->ctx, graph->csr, seeds.data(), seed_class.data(), seeds.size(),
	                             (uint32_t)state->class_row.size(), input->max_levels, GGResultOut(owner)),
	               "gg_level_sets");
	gg_result *res = owner.get();
	GGFetchPairRows(res, gg_level_sets_levels, gg_level_sets_fetch, "gg_level_sets", state->row_class, state->vertex,
	                state->level_end);
	for (idx_t l = 1; l < state->level_end.size(); l++) {
		state->level_end[l] += state->level_end[l - 1];
	}
	return move(state);
}

void PhysicalGGRecursiveLevels::GetData(ExecutionContext &context, DataChunk &chunk, GlobalSourceState &gstate_p,
                                        LocalSourceState &lstate) const {
	auto &state = (RecursiveLevelsState &)gstate_p;
	if (state.distinct_chunk < state.distinct.ChunkCount()) { // the distinct anchor rows first
		chunk.Reference(state.distinct.GetChunk(state.distinct_chunk++));
		return;
	}
	const idx_t n = MinValue<idx_t>(STANDARD_VECTOR_SIZE, state.vertex.size() - state.next_row);
	if (n == 0) {
		chunk.SetCardinality(0);
		return;
	}
	idx_t anchor_row[STANDARD_VECTOR_SIZE];
	int64_t level[STANDARD_VECTOR_SIZE];
	for (idx_t i = 0; i < n; i++) {
		anchor_row[i] = state.class_row[state.row_class[state.next_row + i]];
		while (state.next_row + i >= state.level_end[state.next_level - 1]) { // (no level is empty)
			state.next_level++;
		}
		level[i] = (int64_t)state.next_level;
	}
	for (idx_t c = 0; c < input->columns.size(); c++) {
		auto &spec = input->columns[c];
		switch (spec.kind) {
		case GGWalkColumn::CARRIED:
			GGGatherRows(state.distinct, c, anchor_row, n, chunk.data[c]);
			break;
		case GGWalkColumn::CONSTANT:
			chunk.data[c].Reference(spec.constant);
			break;
		case GGWalkColumn::TABLE: // the next link: the vertex reached, the sentinel as NULL
			GGLinkColumn(state.vertex.data() + state.next_row, n, input->sentinel, chunk.data[c]);
			break;
		case GGWalkColumn::COUNTER: { // the anchor's constant + step x level, computed in BIGINT
			Vector start(types[c]), wide(LogicalType::BIGINT);
			GGGatherRows(state.distinct, c, anchor_row, n, start);
			VectorOperations::Cast(start, wide, n);
			auto values = FlatVector::GetData<int64_t>(wide);
			for (idx_t i = 0; i < n; i++) {
				values[i] += spec.step * level[i];
			}
			VectorOperations::Cast(wide, chunk.data[c], n);
			break;
		}
		}
	}
	state.next_row += n;
	chunk.SetCardinality(n);
}

string PhysicalGGRecursiveLevels::ParamsToString() const {
	return input->description;
}

} // namespace duckdb
