"""The eight walk-row operators on calls that carry TWO faults at once: the status code is that of the check which comes
first in the entry point, so the order of the argument checks is behaviour.

The graph and the results are those of test_gpu_result_kinds.py: the walk table has the levels 1..2, the closure is one of
the five older kinds and the aggregate one of the kinds born with a refusal contract.  The expected codes below are
written from the entry points' source, check by check, not from a run:

  gg_result_filter_common_neighbour  one check: GG_ERR_INVALID_ARG for every fault, a shard included
  gg_result_filter_edge              handles, `materialise` without out_result (I) -> shard (S) -> kind (S) -> hops (I) ->
                                     columns (I) -> mode (I)
  gg_result_extend_edge              handles, `materialise` without out_result (I) -> shard (S) -> kind (S) -> hops (I) ->
                                     column (I) -> edge columns from a CSR without rowids (S)
  gg_result_group_by                 handles (I) -> neither stats nor out_result (I) -> shard (S) -> kind (S) -> hops (I) ->
                                     columns (I) -> weights without a weight column (I)
  gg_result_filter_value             handles, values (I) -> shard (S) -> kind (S) -> hops (I) -> column (I) -> mode (I) ->
                                     `materialise` without out_result (I)
  gg_result_top_rows                 the same checks -> no out_result (I) -> tie column (I)
  gg_result_distinct                 handles, cols (I) -> kind (expect_kind: I for an older kind, S for a younger one) ->
                                     `materialise` without out_result (I) -> neither (I) -> hops (I) -> columns (I)
  gg_result_group_tuples             handles, cols (I) -> kind (expect_kind) -> neither (I) -> hops (I) -> key columns (I) ->
                                     value column (I) -> value table, values (I) -> shard (S)

After its refusals every entry point serves a correct call, whose figures are checked against numpy on the fetched table."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_result_kinds import DST, ROWID, SEEDS, SRC, VID, make_results

pytestmark = pytest.mark.gpu

OK, I, S = 0, -1, -6  # GG_OK, GG_ERR_INVALID_ARG, GG_ERR_STATE
i64p, u64p, intp = C.POINTER(C.c_int64), C.POINTER(C.c_uint64), C.POINTER(C.c_int)
HOPS, HOPS_OUT, COL_OUT, MODE_BAD = 2, 3, 9, 7  # the walk table has the levels 1..2
VALUES = np.arange(VID.size, dtype=np.int64) * 3 - 4


def _p(a, t=i64p):
    return None if a is None else a.ctypes.data_as(t)


@pytest.fixture
def world(gg):
    """the graph's whole CSR, a shard of it, a CSR without edge rowids, one result of every kind, the walk table's rows"""
    assert SRC.size == DST.size == ROWID.size and SEEDS.size == 3
    gg.staging_clear()
    gg.append_vertices(VID)
    gg.append_edges(SRC, DST, ROWID)
    csrs, results = {}, {}
    try:
        csrs["whole"] = gg.build_csr()
        csrs["shard"] = gg.build_csr_shard(0, 2)
        gg.set_edge_rowid(False)
        csrs["plain"] = gg.build_csr()
        gg.set_edge_rowid(True)
        make_results(gg, csrs["whole"], results)
        n = C.c_uint64()
        assert gg.lib.gg_result_rows(results["walk"], HOPS, C.byref(n)) == OK and n.value > 3
        cols = [np.zeros(n.value, np.int64) for _ in range(HOPS + 1)]
        got = C.c_uint32()
        assert gg.lib.gg_result_fetch(results["walk"], HOPS, 0, n.value, (i64p * 3)(*[_p(c) for c in cols]),
                                      C.byref(got)) == OK and got.value == n.value
        yield gg, csrs, results, np.stack(cols, axis=1)
    finally:
        for res in results.values():
            gg.lib.gg_result_destroy(res)
        for csr in csrs.values():
            csr.close()


class Caller:
    """one entry point with a correct argument list; call(**faults) replaces arguments by name and returns the code (a
    result the call made is destroyed), stats holds the figures of the last call"""

    def __init__(self, gg, name, stats_at, **defaults):
        self.lib, self.ctx, self.fn = gg.lib, gg.ctx, getattr(gg.lib, name)
        self.name, self.stats_at, self.defaults = name, stats_at, defaults
        self.stats = None

    def call(self, **faults):
        unknown = set(faults) - set(self.defaults)
        assert not unknown, (self.name, unknown)
        a = dict(self.defaults, **faults)
        made = C.c_void_p()
        self.stats = None if self.stats_at is None else self.fn.argtypes[self.stats_at]._type_()
        args = []
        for key, v in a.items():
            if key == "out":
                args.append(C.byref(made) if v else None)
            elif key == "stats":
                args.append(C.byref(self.stats) if v else None)
            elif isinstance(v, np.ndarray):
                args.append(_p(v, {np.dtype(np.int64): i64p, np.dtype(np.uint64): u64p, np.dtype(np.int32): intp}[v.dtype]))
            else:
                args.append(v)
        try:
            return self.fn(self.ctx, *args)
        finally:
            if made.value is not None:
                self.lib.gg_result_destroy(made)


def refused(caller, cases):
    wrong = []
    for want, faults in cases:
        rc = caller.call(**faults)
        print(f"{caller.name}({', '.join(sorted(faults))}) = {rc}, the source says {want}")
        if rc != want:
            wrong.append((sorted(faults), rc, want))
    assert not wrong, (caller.name, wrong)


def test_common_neighbour_filter(world):
    gg, csrs, res, rows = world
    f = Caller(gg, "gg_result_filter_common_neighbour", None, res=res["walk"], hops=HOPS, filter=csrs["whole"].handle, out=True)
    shard = csrs["shard"].handle
    refused(f, [
        (I, dict(filter=shard)),  # (one fault: this entry point answers a shard with the code of its one check)
        (I, dict(filter=shard, res=res["closure"])),
        (I, dict(filter=shard, res=res["agg"])),
        (I, dict(filter=shard, hops=HOPS_OUT)),
        (I, dict(res=res["closure"], hops=HOPS_OUT)),
        (I, dict(res=res["agg"], hops=HOPS_OUT)),
        (I, dict(filter=shard, out=False)),
        (I, dict(res=None, filter=shard)),
    ])
    made = C.c_void_p()
    assert gg.lib.gg_result_filter_common_neighbour(gg.ctx, res["walk"], HOPS, csrs["whole"].handle, C.byref(made)) == OK
    try:
        n = C.c_uint64()
        assert gg.lib.gg_result_rows(made, HOPS + 1, C.byref(n)) == OK
        adj = {}
        for s, d in zip(SRC, DST):
            adj.setdefault(int(s), []).append(int(d))
        want = 0
        for row in rows:
            for w in adj.get(int(row[0]), []):
                m = 1
                for v in row[1:]:
                    m *= adj.get(int(v), []).count(w)
                want += m
        assert n.value == want
    finally:
        gg.lib.gg_result_destroy(made)


def test_edge_filter(world):
    gg, csrs, res, rows = world
    f = Caller(gg, "gg_result_filter_edge", 8, res=res["walk"], hops=HOPS, csr=csrs["whole"].handle, from_col=HOPS, to_col=0,
               mode=0, materialise=0, stats=True, out=True)
    shard = csrs["shard"].handle
    refused(f, [
        (S, dict(csr=shard)),
        (S, dict(csr=shard, res=res["closure"])),
        (S, dict(csr=shard, res=res["agg"])),
        (S, dict(csr=shard, hops=HOPS_OUT)),
        (S, dict(res=res["closure"], hops=HOPS_OUT)),
        (S, dict(res=res["agg"], hops=HOPS_OUT)),
        (I, dict(hops=HOPS_OUT, from_col=COL_OUT)),
        (I, dict(hops=HOPS_OUT, to_col=-1)),
        (I, dict(to_col=COL_OUT, mode=MODE_BAD)),
        (I, dict(materialise=1, out=False, csr=shard)),  # the first before the second
        (I, dict(res=None, csr=shard)),
        (I, dict(csr=None, res=res["agg"])),
        (S, dict(res=res["agg"], from_col=COL_OUT)),
    ])
    assert f.call() == OK
    edges = {}
    for s, d in zip(SRC, DST):
        edges[(int(s), int(d))] = edges.get((int(s), int(d)), 0) + 1
    m = [edges.get((int(r[HOPS]), int(r[0])), 0) for r in rows]
    assert (f.stats.rows_in, f.stats.rows_out, f.stats.matches) == (len(rows), sum(m), sum(m))
    assert f.call(mode=2) == OK and f.stats.rows_out == sum(1 for x in m if x == 0)


def test_extension(world):
    gg, csrs, res, rows = world
    f = Caller(gg, "gg_result_extend_edge", 7, res=res["walk"], hops=HOPS, csr=csrs["whole"].handle, from_col=HOPS,
               want_edges=0, materialise=0, stats=True, out=True)
    shard, plain = csrs["shard"].handle, csrs["plain"].handle
    refused(f, [
        (S, dict(csr=shard)),
        (S, dict(csr=shard, res=res["closure"])),
        (S, dict(csr=shard, res=res["agg"])),
        (S, dict(csr=shard, hops=HOPS_OUT)),
        (S, dict(res=res["closure"], hops=HOPS_OUT)),
        (S, dict(res=res["agg"], hops=HOPS_OUT)),
        (I, dict(hops=HOPS_OUT, from_col=COL_OUT)),
        (S, dict(csr=plain, want_edges=1)),
        (I, dict(csr=plain, want_edges=1, from_col=COL_OUT)),  # the column before the rowids
        (I, dict(csr=plain, want_edges=1, hops=HOPS_OUT)),
        (I, dict(materialise=1, out=False, csr=shard)),
        (I, dict(res=None, csr=shard)),
        (I, dict(csr=None, res=res["agg"])),
    ])
    assert f.call(csr=plain) == OK  # without edge columns a CSR without rowids serves
    deg = {}
    for s in SRC:
        deg[int(s)] = deg.get(int(s), 0) + 1
    d = [deg.get(int(r[HOPS]), 0) for r in rows]
    assert (f.stats.rows_in, f.stats.rows_out, f.stats.rows_matched) == (len(rows), sum(d), sum(1 for x in d if x))
    assert f.call(want_edges=1, materialise=1) == OK and f.stats.rows_out == sum(d)


def test_group_by(world):
    gg, csrs, res, rows = world
    whole, shard = csrs["whole"].handle, csrs["shard"].handle
    f = Caller(gg, "gg_result_group_by", 8, res=res["walk"], hops=HOPS, key_col=HOPS, key_csr=whole, weight_col=-1,
               weight_csr=None, weights=None, stats=True, out=True)
    refused(f, [
        (S, dict(key_csr=shard)),
        (S, dict(key_csr=shard, res=res["closure"])),
        (S, dict(key_csr=shard, res=res["agg"])),
        (S, dict(key_csr=shard, hops=HOPS_OUT)),
        (S, dict(weight_csr=shard, hops=HOPS_OUT)),
        (S, dict(res=res["closure"], hops=HOPS_OUT)),
        (S, dict(res=res["agg"], hops=HOPS_OUT)),
        (I, dict(hops=HOPS_OUT, key_col=COL_OUT)),
        (I, dict(stats=False, out=False, key_csr=shard)),  # "neither" before the shard
        (I, dict(weight_col=COL_OUT, weights=VALUES)),
        (I, dict(key_col=COL_OUT, weights=VALUES)),
        (I, dict(res=None, key_csr=shard)),
        (I, dict(key_csr=None, res=res["agg"])),
        (S, dict(res=res["agg"], key_col=COL_OUT)),
    ])
    assert f.call(weight_col=0, weights=VALUES) == OK
    assert (f.stats.rows_in, f.stats.rows_grouped, f.stats.groups) == (len(rows), len(rows), np.unique(rows[:, HOPS]).size)


def value_cases(res, shard):
    return [
        (S, dict(csr=shard)),
        (S, dict(csr=shard, res=res["closure"])),
        (S, dict(csr=shard, res=res["agg"])),
        (S, dict(csr=shard, hops=HOPS_OUT)),
        (S, dict(res=res["closure"], hops=HOPS_OUT)),
        (S, dict(res=res["agg"], hops=HOPS_OUT)),
        (I, dict(hops=HOPS_OUT, value_col=COL_OUT)),
        (I, dict(value_col=COL_OUT, mode=MODE_BAD)),
        (I, dict(values=None, csr=shard)),
        (I, dict(res=None, csr=shard)),
        (I, dict(csr=None, res=res["agg"])),
        (S, dict(res=res["agg"], mode=MODE_BAD)),
    ]


def row_values(rows, col):
    at = {int(v): i for i, v in enumerate(VID)}
    return np.array([VALUES[at[int(c)]] for c in rows[:, col]])


def test_value_filter(world):
    gg, csrs, res, rows = world
    f = Caller(gg, "gg_result_filter_value", 11, res=res["walk"], hops=HOPS, value_col=HOPS, csr=csrs["whole"].handle,
               values=VALUES, valid=None, lo=0, hi=15, mode=0, materialise=0, stats=True, out=True)
    shard = csrs["shard"].handle
    refused(f, value_cases(res, shard) + [
        (S, dict(materialise=1, out=False, csr=shard)),  # the second before the first
        (I, dict(materialise=1, out=False, mode=MODE_BAD)),
        (I, dict(materialise=1, out=False)),
    ])
    x = row_values(rows, HOPS)
    assert f.call(materialise=1) == OK
    assert (f.stats.rows_in, f.stats.rows_valued, f.stats.rows_out) == (len(rows), len(rows), int(((0 <= x) & (x <= 15)).sum()))


def test_top_rows(world):
    gg, csrs, res, rows = world
    f = Caller(gg, "gg_result_top_rows", 13, res=res["walk"], hops=HOPS, value_col=HOPS, csr=csrs["whole"].handle,
               values=VALUES, valid=None, lo=0, hi=15, mode=0, descending=1, tie_col=0, n=4, stats=True, out=True)
    shard = csrs["shard"].handle
    refused(f, value_cases(res, shard) + [
        (S, dict(out=False, csr=shard)),
        (S, dict(tie_col=COL_OUT, csr=shard)),
        (I, dict(tie_col=COL_OUT, out=False)),
        (I, dict(tie_col=COL_OUT, mode=MODE_BAD)),
    ])
    x = row_values(rows, HOPS)
    cand = int(((0 <= x) & (x <= 15)).sum())
    assert f.call() == OK
    assert (f.stats.rows_in, f.stats.candidates, f.stats.rows_out) == (len(rows), cand, min(4, cand))


def test_distinct(world):
    gg, csrs, res, rows = world
    cols = np.array([HOPS, 0], np.int32)
    f = Caller(gg, "gg_result_distinct", 6, res=res["walk"], hops=HOPS, cols=cols, n_cols=2, materialise=0, stats=True,
               out=True)
    refused(f, [
        (I, dict(res=res["closure"])),
        (S, dict(res=res["agg"])),
        (I, dict(res=res["closure"], hops=HOPS_OUT)),  # an older kind and a younger one answer differently
        (S, dict(res=res["agg"], hops=HOPS_OUT)),
        (S, dict(res=res["agg"], materialise=1, out=False)),
        (S, dict(res=res["agg"], stats=False, out=False)),
        (I, dict(res=res["agg"], cols=None)),  # the handles before the kind
        (I, dict(hops=HOPS_OUT, cols=np.array([COL_OUT, 0], np.int32))),
        (I, dict(hops=HOPS_OUT, n_cols=0)),
        (I, dict(cols=np.array([0, 0], np.int32), materialise=1, out=False)),
    ])
    assert f.call(materialise=1) == OK
    assert (f.stats.rows_in, f.stats.rows_out) == (len(rows), np.unique(rows[:, [HOPS, 0]], axis=0).shape[0])


def test_group_tuples(world):
    gg, csrs, res, rows = world
    cols = np.array([HOPS, 0], np.int32)
    whole, shard = csrs["whole"].handle, csrs["shard"].handle
    f = Caller(gg, "gg_result_group_tuples", 9, res=res["walk"], hops=HOPS, cols=cols, n_cols=2, value_col=1, value_csr=whole,
               values=VALUES, valid=None, stats=True, out=True)
    refused(f, [
        (S, dict(value_csr=shard)),
        (I, dict(value_csr=shard, res=res["closure"])),  # the kind before the shard: an older kind is GG_ERR_INVALID_ARG
        (S, dict(value_csr=shard, res=res["agg"])),
        (I, dict(value_csr=shard, hops=HOPS_OUT)),  # the level before the shard
        (I, dict(res=res["closure"], hops=HOPS_OUT)),
        (S, dict(res=res["agg"], hops=HOPS_OUT)),
        (I, dict(hops=HOPS_OUT, cols=np.array([COL_OUT, 0], np.int32))),
        (I, dict(value_col=COL_OUT, values=None)),
        (I, dict(value_col=COL_OUT, value_csr=shard)),
        (I, dict(values=None, value_csr=shard)),
        (I, dict(stats=False, out=False, value_csr=shard)),
        (I, dict(value_col=-1, value_csr=shard)),  # a value table without a value column
        (S, dict(res=res["agg"], stats=False, out=False)),
        (I, dict(res=res["agg"], cols=None)),
    ])
    assert f.call() == OK
    assert (f.stats.rows_in, f.stats.rows_valued, f.stats.groups) == (len(rows), len(rows),
                                                                     np.unique(rows[:, [HOPS, 0]], axis=0).shape[0])
