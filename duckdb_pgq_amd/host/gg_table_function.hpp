// gg_table_function.hpp — what the table functions over the device operators share (gg_duckdb_extension.cpp and the
// gg_*.cpp files that register functions): the parsers of the argument prefixes every function repeats, the one bind
// adapter, registration, the column names of walk rows, and the bases of the sources whose rows stay on the device as ONE
// table of one result (GGResultDrain, gg_operators.hpp).  DESIGN.md section 7.11, "How to add a table function", says
// which piece goes where.
#pragma once

#include <initializer_list>

#include "duckdb.hpp"
#include "duckdb/catalog/catalog.hpp"
#include "duckdb/common/exception.hpp"
#include "duckdb/main/client_context.hpp"
#include "duckdb/parser/parsed_data/create_table_function_info.hpp"

#include "gg_extension.hpp"
#include "gg_operators.hpp"

namespace duckdb {

//===--------------------------------------------------------------------===//
// Arguments
//===--------------------------------------------------------------------===//
//! (vertex_table, vertex_key, edge_table, src_col, dst_col) arguments -> scans, resolved at execution time (a missing
//! table or column raises when the scan opens, not at bind time)
struct GraphArguments {
	string vertex_table, vertex_key, edge_table, edge_src, edge_dst;
	explicit GraphArguments(vector<Value> &inputs)
	    : vertex_table(inputs[0].ToString()), vertex_key(inputs[1].ToString()), edge_table(inputs[2].ToString()),
	      edge_src(inputs[3].ToString()), edge_dst(inputs[4].ToString()) {
	}
	static vector<LogicalType> Types() {
		return vector<LogicalType>(5, LogicalType::VARCHAR);
	}
	//! edge_rowid: the edge scan ends in the edge table's rowid
	GGGraphSpec Resolve(ClientContext &context, bool edge_rowid = false) const {
		GGGraphSpec spec;
		spec.vertices = GGTableSource(context, vertex_table, {vertex_key}, false);
		spec.edges = GGTableSource(context, edge_table, {edge_src, edge_dst}, edge_rowid);
		spec.edges_with_rowid = edge_rowid;
		return spec;
	}
	//! The graph of these tables: GGBuildGraph, or with the edge rowids GGBuildGraphWithRowids (gg_extension.hpp: either
	//! may hand back a pinned graph)
	shared_ptr<GGGraph> Build(ClientContext &context, bool edge_rowid = false) const {
		const auto spec = Resolve(context, edge_rowid);
		return edge_rowid ? GGBuildGraphWithRowids(context, spec) : GGBuildGraph(context, spec);
	}
};

//! "<fn>: <names> must not be NULL<when>" if one of inputs[which] is
inline void GGRequireArguments(const string &fn, const vector<Value> &inputs, std::initializer_list<idx_t> which,
                               const char *names, const char *when = "") {
	for (auto i : which) {
		if (inputs[i].is_null) {
			throw BinderException(fn + ": " + names + " must not be NULL" + when);
		}
	}
}

//! a `hops` argument in 1..max_hops
inline int64_t GGHopsArgument(const string &fn, const Value &value, int64_t max_hops) {
	const auto hops = value.GetValue<int64_t>();
	if (hops < 1 || hops > max_hops) {
		throw BinderException(fn + ": need 1 <= hops <= " + to_string(max_hops));
	}
	return hops;
}

//! The arguments of a function over walk rows: the graph's five, sources_sql VARCHAR (inputs[5]; NULL or '': from every
//! vertex), hops BIGINT (inputs[6]) and, for the functions that join the walks with a second keyed table, ext_table,
//! ext_key_col, ext_next_col VARCHAR and from_col BIGINT in 0..hops (inputs[7..10]).  The joined row is one column longer,
//! so hops may reach GG_MAX_HOPS - 1 with an extension and GG_MAX_HOPS without.
struct GGWalkArguments : public GraphArguments {
	enum Extension {
		NO_EXTENSION,
		EXTENSION,
		OPTIONAL_EXTENSION // a NULL or empty ext_table: no extension, and the other three are not looked at
	};
	//! required, required_names: the arguments that must not be NULL (hops among them) and how the message lists them;
	//! they are checked first, then the ranges of hops and from_col
	GGWalkArguments(string fn_p, vector<Value> &inputs, Extension extension, std::initializer_list<idx_t> required,
	                const char *required_names)
	    : GraphArguments(inputs), fn(move(fn_p)), sources_sql(inputs[5].is_null ? string() : inputs[5].ToString()),
	      extended(extension == EXTENSION) {
		GGRequireArguments(fn, inputs, required, required_names);
		if (extension == OPTIONAL_EXTENSION && !inputs[7].is_null && !inputs[7].ToString().empty()) {
			extended = true;
			GGRequireArguments(fn, inputs, {8, 9, 10}, "ext_key_col, ext_next_col and from_col", " where ext_table is given");
		}
		hops = GGHopsArgument(fn, inputs[6], GG_MAX_HOPS - (extended ? 1 : 0));
		if (extended) {
			ext_table = inputs[7].ToString(), ext_key = inputs[8].ToString(), ext_next = inputs[9].ToString();
			from_col = inputs[10].GetValue<int64_t>();
			if (from_col < 0 || from_col > hops) {
				throw BinderException(fn + ": from_col must lie in 0.." + to_string(hops));
			}
		}
	}
	static vector<LogicalType> Types(bool extension) {
		auto types = GraphArguments::Types();
		types.insert(types.end(), {LogicalType::VARCHAR, LogicalType::BIGINT});
		if (extension) {
			types.insert(types.end(), {LogicalType::VARCHAR, LogicalType::VARCHAR, LogicalType::VARCHAR, LogicalType::BIGINT});
		}
		return types;
	}

	string fn;          // the function's name, for its messages
	string sources_sql; // empty: walks start at every vertex
	int64_t hops;
	bool extended;
	string ext_table, ext_key, ext_next;
	int64_t from_col = 0;

	bool AllSources() const {
		return sources_sql.empty();
	}
	//! the ids sources_sql yields (none where AllSources())
	vector<int64_t> Sources(ClientContext &context) const {
		return AllSources() ? vector<int64_t>() : GGQueryInt64Column(context, sources_sql, (fn + ": sources").c_str());
	}
	//! The statement's graph: with an extension GGBuildExtendGraph (the walk CSR and the joined table's in
	//! GGGraph::filter_csr; never a pinned graph), otherwise GraphArguments::Build
	shared_ptr<GGGraph> BuildGraph(ClientContext &context) const {
		if (!extended) {
			return Build(context);
		}
		return GGBuildExtendGraph(context, GGTableSource(context, vertex_table, {vertex_key}, false),
		                          GGTableSource(context, edge_table, {edge_src, edge_dst}, false),
		                          GGTableSource(context, ext_table, {ext_key, ext_next}, true));
	}
	//! for EXPLAIN: "2-hop walks of knows[ joined with message on v2 = m_creatorid]"
	string Describe() const {
		return to_string(hops) + "-hop walks of " + edge_table +
		       (extended ? " joined with " + ext_table + " on v" + to_string(from_col) + " = " + ext_key : string());
	}
};

//! Appends the column names of walk rows: [rank,] v0 .. v{hops} [, w, ext_rowid]
inline void GGWalkColumnNames(vector<string> &names, int64_t hops, bool extended = false, bool ranked = false) {
	if (ranked) {
		names.push_back("rank");
	}
	for (int64_t c = 0; c <= hops; c++) {
		names.push_back("v" + to_string(c));
	}
	if (extended) {
		names.push_back("w");
		names.push_back("ext_rowid");
	}
}

//===--------------------------------------------------------------------===//
// Values
//===--------------------------------------------------------------------===//
//! a value per vertex of one CSR, in its vertex-table order (include/gg.h, "the value of a row")
struct ValueColumn {
	vector<int64_t> values;
	vector<uint64_t> valid;
};

//! value_column of `table` per vertex of `csr`, keyed by key_column.  A vertex no row names, or whose value is NULL, has
//! no value; two rows of one key with different values are refused.
inline ValueColumn ValuesInVertexOrder(ClientContext &context, GGGraph &graph, gg_csr *csr, const string &table,
                                       const string &key_column, const string &value_column, const char *fn) {
	const auto rows = GGCollectKeyedValues(context, GGTableSource(context, table, {key_column, value_column}, false), fn,
	                                       "value_column");
	const idx_t n = rows.keys.size();
	vector<uint32_t> dense(n ? n : 1);
	uint64_t V = 0, kept = 0, dropped = 0;
	{
		lock_guard<mutex> guard(graph.lock);
		GGGraph::Check(gg_csr_info(csr, &V, &kept, &dropped), "gg_csr_info");
		if (n) {
			GGGraph::Check(gg_csr_lookup(graph.ctx, csr, rows.keys.data(), n, dense.data()), "gg_csr_lookup");
		}
	}
	ValueColumn out;
	out.values.assign(V ? V : 1, 0);
	out.valid.assign((V + 63) / 64 + 1, 0);
	vector<uint64_t> seen((V + 63) / 64 + 1, 0);
	for (idx_t i = 0; i < n; i++) {
		const uint32_t d = dense[i];
		if (d == UINT32_MAX) {
			continue; // (a key that is no vertex of the CSR: no row of the walk table can hold it)
		}
		const uint64_t bit = 1ull << (d & 63);
		if (seen[d >> 6] & bit) {
			const bool had = out.valid[d >> 6] & bit;
			if (had != (bool)rows.has[i] || (had && out.values[d] != rows.values[i])) {
				throw InvalidInputException(string(fn) + ": two rows of " + table + " share " + key_column + " = " +
				                            to_string(rows.keys[i]) + " and carry different values of " + value_column +
				                            "; a value per " + key_column + " cannot express that");
			}
			continue;
		}
		seen[d >> 6] |= bit;
		if (rows.has[i]) {
			out.valid[d >> 6] |= bit;
			out.values[d] = rows.values[i];
		}
	}
	return out;
}

//===--------------------------------------------------------------------===//
// Bind and registration
//===--------------------------------------------------------------------===//
//! What a function's bind is written as: the parts of the reference's bind signature a gg function uses, and which of
//! the functions that share the code this is (rows or count form, ...; 0 where there is one)
typedef unique_ptr<FunctionData> (*gg_bind_t)(ClientContext &context, vector<Value> &inputs,
                                              vector<LogicalType> &return_types, vector<string> &names, int kind);

//! The reference's table_function_bind_t over a gg_bind_t: GGScanFunction(name, types, GGBind<ExtendBind, COUNT>)
template <gg_bind_t BIND, int KIND = 0>
unique_ptr<FunctionData> GGBind(ClientContext &context, vector<Value> &inputs, unordered_map<string, Value> &named_parameters,
                                vector<LogicalType> &input_table_types, vector<string> &input_table_names,
                                vector<LogicalType> &return_types, vector<string> &names) {
	return BIND(context, inputs, return_types, names, KIND);
}

//! Creates the functions in the catalog (inside the caller's transaction)
inline void GGRegisterTableFunctions(ClientContext &context, vector<TableFunction> functions) {
	auto &catalog = Catalog::GetCatalog(context);
	for (auto &function : functions) {
		CreateTableFunctionInfo info(function);
		catalog.CreateTableFunction(context, &info);
	}
}

//===--------------------------------------------------------------------===//
// Sources
//===--------------------------------------------------------------------===//
//! The global state of a source whose rows are one table of one device result, drained by the pipeline's threads together
struct GGDrainState : public GlobalSourceState {
	idx_t MaxThreads() override {
		return max_threads;
	}
	GGResultDrain drain;   // the rows (count forms: none)
	idx_t max_threads = 1;
	bool counted = false;  // count forms: the one row went out (under drain.lock)
	idx_t next_rank = 0;   // ranked forms (one thread drains): the rank of the next row to leave
};
//! ... with the statistics of the device call that made the result
template <class STATS>
struct GGDrainStateOf : public GGDrainState {
	STATS stats {};
};

//! A source that hands device-resident rows to the pipeline's threads through GGResultSlab windows.  The helpers follow the
//! drain protocol written down at GGResultDrain (gg_operators.hpp): slab.Columns(n) is called inside the fetch.
class GGResultSource : public PhysicalOperator {
public:
	GGResultSource(vector<LogicalType> types, shared_ptr<GGGraph> graph_p)
	    : PhysicalOperator(PhysicalOperatorType::INVALID, move(types), 0), graph(move(graph_p)) {
	}

	shared_ptr<GGGraph> graph;

	unique_ptr<LocalSourceState> GetLocalSourceState(ExecutionContext &context, GlobalSourceState &gstate) const override {
		return make_unique<GGResultSlab>(graph);
	}

protected:
	static void PollInterrupt(ExecutionContext &context) {
		if (context.client.interrupted) {
			throw InterruptException();
		}
	}
	//! The one row of a count form, to the first thread that asks
	static void EmitCountRow(GGDrainState &state, DataChunk &chunk, std::initializer_list<uint64_t> values) {
		lock_guard<mutex> guard(state.drain.lock);
		if (state.counted) {
			return;
		}
		state.counted = true;
		idx_t c = 0;
		for (auto value : values) {
			FlatVector::GetData<int64_t>(chunk.data[c++])[0] = (int64_t)value;
		}
		chunk.SetCardinality(1);
	}
	//! The slab has rows to serve, after claiming and fetching the next ones of the state's one table where it had none;
	//! false: nothing is left.  fetch: a GGResultDrain::fetch_t
	template <class FETCH>
	static bool Refill(GGDrainState &state, GGResultSlab &slab, const FETCH &fetch) {
		return slab.pos < slab.rows || state.drain.Refill(slab, [] { return false; }, fetch); // (nothing to advance to)
	}
	//! Refill with the first `columns` id columns of the rows (gg_result_fetch)
	static bool FetchIds(GGDrainState &state, GGResultSlab &slab, idx_t columns) {
		return Refill(state, slab, [columns](gg_result *result, int table, idx_t offset, uint32_t want, GGResultSlab &slab) {
			uint32_t got = 0;
			GGGraph::Check(gg_result_fetch(result, table, offset, want, slab.Columns(columns), &got), "gg_result_fetch");
			return got;
		});
	}
	//! Refill with `ids` id columns, then `edges` edge columns (gg_result_fetch_edges); fn: for the message
	static bool FetchIdsAndEdges(GGDrainState &state, GGResultSlab &slab, idx_t ids, idx_t edges, const char *fn) {
		struct {
			idx_t ids, edges;
			const char *fn;
		} shape = {ids, edges, fn};
		auto at = &shape; // (one pointer: the closure stays within std::function's own storage)
		return Refill(state, slab, [at](gg_result *result, int table, idx_t offset, uint32_t want, GGResultSlab &slab) {
			uint32_t got = 0, got_edges = 0;
			auto columns = slab.Columns(at->ids + at->edges);
			GGGraph::Check(gg_result_fetch(result, table, offset, want, columns, &got), "gg_result_fetch");
			GGGraph::Check(gg_result_fetch_edges(result, table, offset, want, columns + at->ids, &got_edges),
			               "gg_result_fetch_edges");
			if (got_edges != got) {
				throw InternalException(string(at->fn) + ": id and edge columns of different lengths");
			}
			return got;
		});
	}
	//! Serves the next rows of a slab filled by FetchIdsAndEdges: the id columns into chunk.data[first ..], then the LAST
	//! edge column — the joined row's rowid; a walk carries no edge columns, the others hold -1 — behind them
	static idx_t EmitIdsAndRowid(GGResultSlab &slab, DataChunk &chunk, idx_t first, idx_t ids, idx_t edges) {
		const idx_t n = MinValue<idx_t>(STANDARD_VECTOR_SIZE, slab.rows - slab.pos);
		memcpy(FlatVector::GetData<int64_t>(chunk.data[first + ids]), slab.column[ids + edges - 1] + slab.pos,
		       n * sizeof(int64_t));
		return slab.Emit(chunk, first, ids);
	}
	//! chunk.data[0] of `count` rows just emitted: their ranks (one thread: the slabs are claimed and emitted in order)
	static void EmitRank(GGDrainState &state, DataChunk &chunk, idx_t count) {
		auto rank = FlatVector::GetData<int64_t>(chunk.data[0]);
		for (idx_t i = 0; i < count; i++) {
			rank[i] = (int64_t)(state.next_rank + i);
		}
		state.next_rank += count;
	}
};

//! A source over the `hops`-hop walks from `sources` (all_sources: from every vertex)
class GGWalkSource : public GGResultSource {
public:
	GGWalkSource(vector<LogicalType> types, shared_ptr<GGGraph> graph_p, int hops_p, vector<int64_t> sources_p,
	             bool all_sources_p)
	    : GGResultSource(move(types), move(graph_p)), hops(hops_p), sources(move(sources_p)), all_sources(all_sources_p) {
	}

	int hops;
	vector<int64_t> sources;
	bool all_sources;

protected:
	//! the sources as the C-ABI takes them: (ids, their number), null for every vertex
	const int64_t *SourceIds() const {
		return all_sources ? nullptr : GGSourceIds(sources);
	}
	uint64_t SourceCount() const {
		return all_sources ? 0 : sources.size();
	}
	//! The walk table, on the device.  Caller holds graph->lock.
	void ExpandWalks(GGResultPtr &out) const {
		GGExpandWalks(*graph, sources, all_sources, hops, out);
	}
	//! The walk table joined with the rows of graph->filter_csr on column from_col (gg_result_extend_edge, include/gg.h),
	//! the walk table freed before this returns.  out null: counted only.  Caller holds graph->lock.
	void ExpandExtended(int from_col, bool keep_ids, bool keep_edges, gg_extend_stats &stats, GGResultPtr *out) const {
		GGResultPtr walks;
		ExpandWalks(walks);
		GGGraph::Check(gg_result_extend_edge(graph->ctx, walks.get(), hops, graph->filter_csr, from_col, keep_ids ? 1 : 0,
		                                     keep_edges ? 1 : 0, &stats,
		                                     out ? static_cast<gg_result **>(GGResultOut(*out)) : nullptr),
		               "gg_result_extend_edge");
	}
};

} // namespace duckdb
