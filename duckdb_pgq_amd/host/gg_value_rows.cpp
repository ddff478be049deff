// gg_value_rows.cpp — walk rows joined with a second keyed table, then filtered by a value range and cut to the best n by
// that value, as three table functions over gg_khop_extend's arguments (gg_extend.cpp) and graph (GGBuildExtendGraph):
//
//   gg_khop_extend_filter(<gg_khop_extend's 11 arguments>, value_column VARCHAR, value_of BIGINT, lo BIGINT, hi BIGINT,
//                         negate BOOLEAN)
//        -> (v0 BIGINT, ..., v{hops} BIGINT, w BIGINT, ext_rowid BIGINT)  the joined rows whose value passes, in input order
//   gg_khop_extend_filter_count(same arguments)
//        -> (rows BIGINT, walks BIGINT, valued BIGINT)   one row: rows that pass, joined rows looked at, of those with a value
//   gg_khop_extend_top(<the same>, descending BOOLEAN, tie_col BIGINT, n BIGINT)
//        -> (rank BIGINT, v0 BIGINT, ..., v{hops} BIGINT, w BIGINT, ext_rowid BIGINT)   the best n of them, in rank order
//
// value_of names the column 0..hops + 1 of the joined row whose value is tested.  For hops + 1 (the column w)
// value_column is an integer column of ext_table, a property of the row's ext_next_col (m_creationdate of m_messageid);
// for 0..hops it is an integer column of vertex_table.  Either is read in the statement's own transaction and brought into
// the vertex order of its CSR through gg_csr_lookup.  A NULL value clears the vertex's valid bit: the row behaves as SQL's
// NULL under the comparison and passes nothing.  A NULL lo is INT64_MIN, a NULL hi INT64_MAX; negate keeps the valued rows
// outside [lo, hi].  Two rows of ext_table that share an ext_next_col and carry different values cannot be expressed per
// vertex: the statement is refused with an error that says so (m_messageid is a key in LDBC).  TIMESTAMP columns are out of
// scope: the caller casts.
// gg_khop_extend_top: ORDER BY value [DESC], v{tie_col} (NULL: no tie column), then by input row; n NULL: every row.  Rows
// leave in rank order and one thread drains them, as gg_khop_aggregate_top's do.
// What that stands for in the reference: the filter inside the scan of the payload's table and PhysicalTopN
// (src/execution/operator/order/physical_top_n.cpp:238-293, 421-454) above the last hash join —
// benchmark/ldbc/queries/interactive-complex-2.sql:5,8-9, interactive-complex-9.sql:16-18 (m_creationdate < :date ORDER BY
// m_creationdate DESC, m_messageid LIMIT 20), the date range of interactive-complex-4.sql:9,18.  No planner rule recognises
// these shapes.
// The walk table and the extended table are dropped before the first row leaves; only the answer's rows stay on the device.
#include "gg_table_function.hpp"

namespace duckdb {

namespace {

enum ValueRowsKind { FILTER, COUNT, TOP };

const char *FunctionName(int kind) {
	return kind == FILTER ? "gg_khop_extend_filter" : kind == COUNT ? "gg_khop_extend_filter_count" : "gg_khop_extend_top";
}

struct ValueRowsSpec {
	int kind; // ValueRowsKind
	int hops, from_col, value_of;
	int64_t lo, hi;
	bool negate, descending;
	int tie_col; // -1: none
	uint64_t n;  // TOP: UINT64_MAX: every row
};

class PhysicalGGValueRows : public GGWalkSource {
public:
	PhysicalGGValueRows(shared_ptr<GGGraph> graph_p, ValueRowsSpec spec_p, vector<int64_t> sources_p, bool all_sources_p,
	                    ValueColumn column_p)
	    : GGWalkSource(OutputTypes(spec_p), move(graph_p), spec_p.hops, move(sources_p), all_sources_p), spec(spec_p),
	      column(move(column_p)) {
	}
	static vector<LogicalType> OutputTypes(const ValueRowsSpec &spec) {
		const idx_t n = spec.kind == COUNT ? 3 : spec.hops + 3 + (spec.kind == TOP ? 1 : 0);
		return vector<LogicalType>(n, LogicalType::BIGINT);
	}
	typedef GGDrainStateOf<gg_value_filter_stats> State;

	ValueRowsSpec spec;
	ValueColumn column;

	unique_ptr<GlobalSourceState> GetGlobalSourceState(ClientContext &context) const override {
		auto state = make_unique<State>();
		lock_guard<mutex> guard(graph->lock);
		if (!graph->csr || !graph->filter_csr) {
			throw InternalException("GG_VALUE_ROWS scheduled before both CSRs were built");
		}
		const int out_hops = hops + 1;
		const gg_csr *value_csr = spec.value_of == out_hops ? graph->filter_csr : graph->csr;
		const int mode = spec.negate ? GG_VALUE_NOT_IN : GG_VALUE_IN;
		state->drain.Replace(context, out_hops, [&](idx_t &rows) {
			GGResultPtr owner, extended;
			gg_extend_stats extend_stats {};
			ExpandExtended(spec.from_col, true, true, extend_stats, &extended);
			if (spec.kind == TOP) {
				gg_value_top_stats top {};
				GGGraph::Check(gg_result_top_rows(graph->ctx, extended.get(), out_hops, spec.value_of, value_csr,
				                                  column.values.data(), column.valid.data(), spec.lo, spec.hi, mode,
				                                  spec.descending ? 1 : 0, spec.tie_col, spec.n, &top, GGResultOut(owner)),
				               "gg_result_top_rows");
				state->stats.rows_in = top.rows_in, state->stats.rows_valued = top.rows_valued;
				state->stats.rows_out = top.rows_out;
			} else {
				const bool count = spec.kind == COUNT;
				GGGraph::Check(gg_result_filter_value(graph->ctx, extended.get(), out_hops, spec.value_of, value_csr,
				                                      column.values.data(), column.valid.data(), spec.lo, spec.hi, mode,
				                                      count ? 0 : 1, &state->stats,
				                                      count ? nullptr : static_cast<gg_result **>(GGResultOut(owner))),
				               "gg_result_filter_value");
			}
			rows = spec.kind == COUNT ? 0 : state->stats.rows_out;
			return owner; // (the extended table goes back to the pool here: only the answer's rows stay in HBM)
		});
		if (spec.kind == FILTER) {
			state->max_threads = GGResultSlab::ThreadsFor(state->stats.rows_out);
		}
		return move(state);
	}

	void GetData(ExecutionContext &context, DataChunk &chunk, GlobalSourceState &gstate_p,
	             LocalSourceState &lstate) const override {
		auto &gstate = (State &)gstate_p;
		PollInterrupt(context);
		if (spec.kind == COUNT) {
			EmitCountRow(gstate, chunk, {gstate.stats.rows_out, gstate.stats.rows_in, gstate.stats.rows_valued});
			return;
		}
		// the slab: the id columns v0..v{hops}, w, then the edge columns e1..e{hops+1}, the last of which is ext_rowid
		auto &slab = (GGResultSlab &)lstate;
		const idx_t ids = (idx_t)hops + 2, edges = (idx_t)hops + 1;
		if (!FetchIdsAndEdges(gstate, slab, ids, edges, "gg_khop_extend_filter")) {
			return;
		}
		if (spec.kind == TOP) {
			EmitRank(gstate, chunk, EmitIdsAndRowid(slab, chunk, 1, ids, edges));
		} else {
			EmitIdsAndRowid(slab, chunk, 0, ids, edges);
		}
	}

	string GetName() const override {
		return "GG_VALUE_ROWS";
	}
};

unique_ptr<FunctionData> ValueRowsBind(ClientContext &context, vector<Value> &inputs, vector<LogicalType> &return_types,
                                       vector<string> &names, int kind) {
	const GGWalkArguments args(FunctionName(kind), inputs, GGWalkArguments::EXTENSION, {6, 7, 8, 9, 10, 11, 12},
	                           "hops, ext_table, ext_key_col, ext_next_col, from_col, value_column and value_of");
	const string &fn = args.fn;
	const auto hops = args.hops;
	const string value_column = inputs[11].ToString();
	const auto value_of = inputs[12].GetValue<int64_t>();
	if (value_of < 0 || value_of > hops + 1) {
		throw BinderException(fn + ": value_of must lie in 0.." + to_string(hops + 1));
	}
	ValueRowsSpec spec {};
	spec.kind = kind;
	spec.hops = (int)hops, spec.from_col = (int)args.from_col, spec.value_of = (int)value_of;
	spec.lo = inputs[13].is_null ? INT64_MIN : inputs[13].GetValue<int64_t>();
	spec.hi = inputs[14].is_null ? INT64_MAX : inputs[14].GetValue<int64_t>();
	spec.negate = !inputs[15].is_null && inputs[15].GetValue<bool>();
	spec.tie_col = -1;
	spec.n = UINT64_MAX;
	if (kind == TOP) {
		spec.descending = !inputs[16].is_null && inputs[16].GetValue<bool>();
		if (!inputs[17].is_null) {
			const auto tie = inputs[17].GetValue<int64_t>();
			if (tie < 0 || tie > hops + 1) {
				throw BinderException(fn + ": tie_col must be NULL or lie in 0.." + to_string(hops + 1));
			}
			spec.tie_col = (int)tie;
		}
		if (!inputs[18].is_null) {
			const auto n = inputs[18].GetValue<int64_t>();
			if (n < 0) {
				throw BinderException(fn + ": n must not be negative");
			}
			spec.n = (uint64_t)n;
		}
	}
	auto data = make_unique<GGFunctionData>();
	data->open = [=](ClientContext &ctx, GGOpened &opened) {
		opened.graph = args.BuildGraph(ctx);
		auto sources = args.Sources(ctx);
		const bool of_ext = value_of == args.hops + 1;
		auto column = ValuesInVertexOrder(ctx, *opened.graph, of_ext ? opened.graph->filter_csr : opened.graph->csr,
		                                  of_ext ? args.ext_table : args.vertex_table, of_ext ? args.ext_next : args.vertex_key,
		                                  value_column, args.fn.c_str());
		opened.source = make_unique<PhysicalGGValueRows>(opened.graph, spec, move(sources), args.AllSources(), move(column));
	};
	data->parallel_result = kind == FILTER; // (the top's rows leave in rank order)
	data->description = args.Describe() + ", " + value_column + " of column " + to_string(value_of) +
	                    (spec.negate ? " outside [" : " in [") + to_string(spec.lo) + ", " + to_string(spec.hi) + "]" +
	                    (kind == TOP ? string(", ordered") + (spec.descending ? " descending" : "") : string());
	return_types = PhysicalGGValueRows::OutputTypes(spec);
	if (kind == COUNT) {
		names = {"rows", "walks", "valued"};
	} else {
		GGWalkColumnNames(names, hops, true, kind == TOP);
	}
	return move(data);
}

} // namespace

void GGRegisterValueRowsFunctions(ClientContext &context) {
	auto args = GGWalkArguments::Types(true);
	args.insert(args.end(), {LogicalType::VARCHAR, LogicalType::BIGINT, LogicalType::BIGINT, LogicalType::BIGINT,
	                         LogicalType::BOOLEAN});
	auto top_args = args;
	top_args.insert(top_args.end(), {LogicalType::BOOLEAN, LogicalType::BIGINT, LogicalType::BIGINT});
	GGRegisterTableFunctions(context, {GGScanFunction("gg_khop_extend_filter", args, GGBind<ValueRowsBind, FILTER>),
	                                   GGScanFunction("gg_khop_extend_filter_count", args, GGBind<ValueRowsBind, COUNT>),
	                                   GGScanFunction("gg_khop_extend_top", top_args, GGBind<ValueRowsBind, TOP>)});
}

} // namespace duckdb
