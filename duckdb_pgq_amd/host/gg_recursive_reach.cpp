// gg_recursive_reach.cpp — a UNION recursive CTE over one keyed table as one device reachability closure.
//
// Reachability and transitive closures (interactive-complex-12.sql's extended_tags; `reach(p)` over a mirrored knows)
// recurse as
//     anchor  UNION  SELECT <carried cte columns, T.next at the link's position, constants> FROM T, cte
//                    WHERE T.key = cte.link
// The reference runs PhysicalRecursiveCTE with union_all == false: the arm's pipeline, hash-join build over T included,
// once per level, every produced row probed against a GroupedAggregateHashTable of all rows emitted so far and kept
// only if it is a new group (src/execution/operator/set/physical_recursive_cte.cpp:47-70 ProbeHT / Sink, :75-139).
// Every arm row is (C(parent), next, K_arm): its carried columns C come unchanged from the anchor row it descends from,
// its constants K are the arm's.  So a row is (class, vertex) with the class a distinct C of the anchor rows, and the
// recursion is a multi-source BFS over the CSR of T's edges key -> next with a visited set keyed by (class, vertex)
// (gg_reach_closure).  Here, on the host and exactly as the reference's hash table compares rows (NULL equal to NULL):
//   - the anchor rows are deduplicated (the reference's Sink deduplicates the anchor as well);
//   - classes are the distinct C of the distinct anchor rows (the group a hash table over C gives a row);
//   - a distinct anchor row is "seen" if its K equals the arm's constants: then the arm row (C, link, K_arm) equals it,
//     and its (class, link) is visited from the start; otherwise it is still expanded and its (class, link) is a new row
//     of the first level that reaches it.
// The rows: the distinct anchor rows, then level by level the closure's rows, carried columns gathered from the class's
// first anchor row, the link as the vertex id cast to the CTE column's type, the constants.
//
// NULLs as the reference's join treats them: a T row with a NULL key joins nothing; a NULL next is staged as the
// sentinel id, a vertex without out-edges that is no key, link or next, so (class, NULL) is one row per class; an anchor
// row with a NULL link seeds the sentinel (it joins nothing, but if it is seen the arm's (C, NULL, K) equals it).
#include "duckdb.hpp"
#include "duckdb/common/types/chunk_collection.hpp"
#include "duckdb/common/vector_operations/vector_operations.hpp"
#include "duckdb/execution/aggregate_hashtable.hpp"
#include "duckdb/storage/buffer_manager.hpp"

#include <unordered_map>

#include "gg_extension.hpp"
#include "gg_operators.hpp"
#include "gg_pipeline.hpp"

namespace duckdb {

PhysicalGGRecursiveReach::PhysicalGGRecursiveReach(vector<LogicalType> types, shared_ptr<GGGraph> graph_p,
                                                   shared_ptr<GGWalkInput> input_p, idx_t estimated_cardinality)
    : PhysicalOperator(PhysicalOperatorType::INVALID, move(types), estimated_cardinality), graph(move(graph_p)),
      input(move(input_p)) {
}

namespace {

class RecursiveReachState : public GlobalSourceState {
public:
	ChunkCollection distinct;  // the distinct anchor rows, in their first occurrence's order
	vector<idx_t> class_row;   // class -> its first distinct anchor row
	vector<int64_t> row_class; // closure row -> class
	vector<int64_t> vertex;    // closure row -> vertex id
	idx_t distinct_chunk = 0;  // next distinct anchor chunk to emit
	idx_t next_row = 0;        // next closure row to emit
};

//! the columns `cols` of `chunk` as a chunk of their own (referenced, not copied)
void Project(DataChunk &chunk, const vector<idx_t> &cols, const vector<LogicalType> &types, DataChunk &out) {
	out.Initialize(types);
	for (idx_t i = 0; i < cols.size(); i++) {
		out.data[i].Reference(chunk.data[cols[i]]);
	}
	out.SetCardinality(chunk.size());
}

} // namespace

void GGDistinctRows(ClientContext &context, ChunkCollection &rows, const vector<LogicalType> &types,
                    ChunkCollection &distinct) {
	GroupedAggregateHashTable rows_ht(BufferManager::GetBufferManager(context), types);
	Vector addresses(LogicalType::POINTER);
	SelectionVector new_groups(STANDARD_VECTOR_SIZE);
	for (idx_t c = 0; c < rows.ChunkCount(); c++) {
		DataChunk chunk;
		chunk.Initialize(types);
		rows.GetChunk(c).Copy(chunk);
		const idx_t n_new = rows_ht.FindOrCreateGroups(chunk, addresses, new_groups);
		if (n_new > 0) {
			chunk.Slice(new_groups, n_new);
			distinct.Append(chunk);
		}
	}
}

void GGRowClasses(ClientContext &context, ChunkCollection &rows, const vector<idx_t> &carried,
                  const vector<LogicalType> &carried_types, vector<uint32_t> &row_class, vector<idx_t> &class_row) {
	row_class.assign(rows.Count(), 0);
	class_row.clear();
	if (carried.empty()) {
		if (rows.Count() > 0) {
			class_row.push_back(0);
		}
		return;
	}
	GroupedAggregateHashTable class_ht(BufferManager::GetBufferManager(context), carried_types);
	std::unordered_map<uintptr_t, uint32_t> class_of;
	Vector addresses(LogicalType::POINTER);
	idx_t at = 0;
	for (idx_t c = 0; c < rows.ChunkCount(); c++) {
		auto &chunk = rows.GetChunk(c);
		DataChunk groups;
		Project(chunk, carried, carried_types, groups);
		class_ht.FindOrCreateGroups(groups, addresses);
		auto address = FlatVector::GetData<data_ptr_t>(addresses);
		for (idx_t r = 0; r < chunk.size(); r++, at++) {
			auto entry = class_of.emplace((uintptr_t)address[r], (uint32_t)class_row.size());
			if (entry.second) {
				class_row.push_back(at);
			}
			row_class[at] = entry.first->second;
		}
	}
}

void GGFetchPairRows(gg_result *res, GGPairLevelsFn levels_fn, GGPairFetchFn fetch_fn, const char *what,
                     vector<int64_t> &row_class, vector<int64_t> &vertex, vector<uint64_t> &per_level) {
	int n_levels = 0;
	GGGraph::Check(levels_fn(res, nullptr, 0, &n_levels), what);
	per_level.assign(MaxValue<int>(n_levels, 1), 0);
	GGGraph::Check(levels_fn(res, per_level.data(), n_levels, &n_levels), what);
	per_level.resize(n_levels);
	uint64_t total = 0;
	for (int l = 0; l < n_levels; l++) {
		total += per_level[l];
	}
	row_class.resize(total);
	vertex.resize(total);
	for (uint64_t at = 0; at < total;) {
		uint32_t got = 0;
		const uint32_t want = (uint32_t)MinValue<uint64_t>(total - at, 1u << 24);
		GGGraph::Check(fetch_fn(res, at, want, row_class.data() + at, vertex.data() + at, nullptr, &got), what);
		if (got == 0) {
			throw InternalException(string(what) + ": a fetch returned no rows");
		}
		at += got;
	}
}

void GGLinkColumn(const int64_t *vertex, idx_t n, int64_t sentinel, Vector &target) {
	Vector wide(LogicalType::BIGINT);
	auto values = FlatVector::GetData<int64_t>(wide);
	auto &validity = FlatVector::Validity(wide);
	for (idx_t i = 0; i < n; i++) {
		values[i] = vertex[i];
		if (values[i] == sentinel) {
			validity.SetInvalid(i);
		}
	}
	VectorOperations::Cast(wide, target, n);
}

unique_ptr<GlobalSourceState> PhysicalGGRecursiveReach::GetGlobalSourceState(ClientContext &context) const {
	auto state = make_unique<RecursiveReachState>();
	auto &buffer_manager = BufferManager::GetBufferManager(context);
	vector<idx_t> carried, constants;
	vector<LogicalType> carried_types, constant_types;
	for (idx_t c = 0; c < input->columns.size(); c++) {
		if (input->columns[c].kind == GGWalkColumn::CARRIED) {
			carried.push_back(c);
			carried_types.push_back(types[c]);
		} else if (input->columns[c].kind == GGWalkColumn::CONSTANT) {
			constants.push_back(c);
			constant_types.push_back(types[c]);
		}
	}
	lock_guard<mutex> guard(input->lock);
	// ---- the distinct anchor rows: the groups a hash table over every column creates, in order
	GGDistinctRows(context, input->anchor, types, state->distinct);
	const idx_t n_distinct = state->distinct.Count();
	// ---- classes (the group of C), seen flags (K equal to the arm's constants)
	vector<uint32_t> seed_class;
	vector<uint8_t> seen(n_distinct, 1);
	GGRowClasses(context, state->distinct, carried, carried_types, seed_class, state->class_row);
	if (!constants.empty()) {
		GroupedAggregateHashTable constant_ht(buffer_manager, constant_types);
		Vector addresses(LogicalType::POINTER);
		DataChunk arm;
		arm.Initialize(constant_types);
		for (idx_t i = 0; i < constants.size(); i++) {
			arm.SetValue(i, 0, input->columns[constants[i]].constant);
		}
		arm.SetCardinality(1);
		constant_ht.FindOrCreateGroups(arm, addresses);
		const auto arm_group = FlatVector::GetData<data_ptr_t>(addresses)[0];
		idx_t at = 0;
		for (idx_t c = 0; c < state->distinct.ChunkCount(); c++) {
			auto &chunk = state->distinct.GetChunk(c);
			DataChunk groups;
			Project(chunk, constants, constant_types, groups);
			constant_ht.FindOrCreateGroups(groups, addresses);
			auto address = FlatVector::GetData<data_ptr_t>(addresses);
			for (idx_t r = 0; r < chunk.size(); r++, at++) {
				seen[at] = address[r] == arm_group;
			}
		}
	}
	if (!input->has_edges || n_distinct == 0) {
		return move(state); // no edge (the CSR holds only the dummy sentinel edge) or no anchor row: the anchor alone
	}
	// ---- seeds: the distinct anchor rows' links (NULL: the sentinel)
	vector<int64_t> seeds;
	vector<bool> valid;
	GGIntegerColumn(state->distinct, input->link_column, seeds, valid);
	for (idx_t r = 0; r < seeds.size(); r++) {
		if (!valid[r]) {
			seeds[r] = input->sentinel;
		}
	}
	lock_guard<std::mutex> graph_guard(graph->lock);
	GGResultPtr owner;
	GGGraph::Check(gg_reach_closure(graph->ctx, graph->csr, seeds.data(), seed_class.data(), seen.data(), seeds.size(),
	                                (uint32_t)state->class_row.size(), GGResultOut(owner)),
	               "gg_reach_closure");
	gg_result *res = owner.get();
	vector<uint64_t> per_level;
	GGFetchPairRows(res, gg_reach_closure_levels, gg_reach_closure_fetch, "gg_reach_closure", state->row_class,
	                state->vertex, per_level);
	return move(state);
}

void PhysicalGGRecursiveReach::GetData(ExecutionContext &context, DataChunk &chunk, GlobalSourceState &gstate_p,
                                       LocalSourceState &lstate) const {
	auto &state = (RecursiveReachState &)gstate_p;
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
	for (idx_t i = 0; i < n; i++) {
		anchor_row[i] = state.class_row[state.row_class[state.next_row + i]];
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
		case GGWalkColumn::COUNTER:
			throw InternalException("GG_RECURSIVE_REACH: a depth counter");
		}
	}
	state.next_row += n;
	chunk.SetCardinality(n);
}

string PhysicalGGRecursiveReach::ParamsToString() const {
	return input->description;
}

} // namespace duckdb
