"""Every device operation on scratch memory that is not zero.

gg_ctx::dev_alloc recycles pool blocks as they are; a fresh hipMalloc block is in practice zero.  A context created with
GG_POOL_FILL=<byte> sets every block it hands out to that byte first (csrc/gg_runtime.hip), so what scratch holds when an
operation starts is an input of the test and no longer depends on which tests ran before.  Three contexts:

  0x00  the fresh-hipMalloc case, made explicit
  0xFF  the library's own "empty" sentinel (DST_EMPTY, INVALID_U32, the cost cells): a forgotten memset to 0 fails
  0xA5  neither: negative as a signed value, no valid small index: a forgotten memset to 0xFF fails

and the unfilled session context as the fourth.  Every operation runs through the check helper and the exact reference
its own module already has (the way tests/test_gpu_edge_ids.py reuses them), so every assertion those make holds here too;
every comparison is between integers and exact.  On top of that, `under` records what every fetch, export and digest of
the test returned and asserts that the record is the same on all four contexts: rows as multisets (a table that atomics
order is compared in order by its own check where an order is defined), everything else in call order.

COVERED maps every C entry point that runs on the device to the test here that runs it under the fills;
tests/test_pool_fill_cpu.py holds it against gg.SYMBOLS, so an operation added later fails there until it is listed."""
import contextlib
import ctypes
import hashlib
import os
import types

import numpy as np
import pytest

import duckdb_pgq_amd as pkg
from duckdb_pgq_amd import gg as ggmod
from duckdb_pgq_amd import sharding
from tests import all_shortest_paths_ref as AP
from tests import bfs_shapes
from tests import cheapest_paths_ref as PR
from tests import cheapest_ref as CR
from tests import edge_ids as EI
from tests import test_gpu_bfs_levels as t_bfs
from tests import test_gpu_build_forms as t_forms
from tests import test_gpu_cheapest as t_cheapest
from tests import test_gpu_cheapest_paths as t_cheapest_paths
from tests import test_gpu_deep_walks as t_deep
from tests import test_gpu_distinct as t_distinct
from tests import test_gpu_edge_ids as t_ids
from tests import test_gpu_extend as t_extend
from tests import test_gpu_group_tuples as t_tuples
from tests import test_gpu_khop_pair_counts as t_pairs
from tests import test_gpu_lazy_reverse_rows as t_lazy
from tests import test_gpu_level_sets as t_levels
from tests import test_gpu_mirrored_tables as t_mirrored
from tests import test_gpu_parity as t_parity
from tests import test_gpu_reach_closure as t_reach
from tests import test_gpu_result_kinds as t_kinds
from tests import test_gpu_scan_sort as t_scan
from tests import test_gpu_value_rows as t_value
from tests import test_gpu_walk_closure as t_walk
from tests.oracle_lib import sort_rows
from tests.test_gpu_derived_reverse import TILE, _ids, mirrored, reverse_reference

pytestmark = pytest.mark.gpu

FILLS = (0x00, 0xFF, 0xA5)
CONTEXTS = (None,) + FILLS  # None: the session's context, never filled
PLACEMENTS = ("wide", "dense_zero", "sparse")  # one per id dictionary (tests/edge_ids.py)
NO_LONG_ROWS = 0xFFFFFFFF

# C entry point -> the test below that runs it on the filled contexts
COVERED = {
    "gg_csr_build": "test_csr_builds",
    "gg_vertices_from_edges": "test_csr_builds",
    "gg_csr_export": "test_csr_builds",
    "gg_debug_csr_reverse": "test_csr_builds",
    "gg_csr_build_shard": "test_sharded_builds",
    "gg_csr_lookup": "test_lookup_and_join_probe",
    "gg_join_probe": "test_lookup_and_join_probe",
    "gg_expand_khop": "test_khop",
    "gg_khop_count": "test_khop",
    "gg_expand_khop_result": "test_khop",
    "gg_result_digest": "test_khop",
    "gg_expand_khop_edges": "test_khop",
    "gg_expand_khop_range": "test_khop",
    "gg_khop_partition": "test_khop",
    "gg_expand_khop_mid": "test_khop",
    "gg_khop_partition_mid": "test_khop",
    "gg_expand_khop_mid_result": "test_khop",
    "gg_expand_khop_dev": "test_khop",
    "gg_result_filter_common_neighbour": "test_same_neighbour_filter_at_five_hops",
    "gg_walk_endpoints": "test_consumers_of_every_build_form",
    "gg_bfs64": "test_bfs_levels_at_both_cell_widths",
    "gg_bfs64_pairs": "test_bfs_levels_at_both_cell_widths",
    "gg_bfs64_pairs_packed": "test_bfs_levels_at_both_cell_widths",
    "gg_bfs64_paths": "test_paths_at_both_cell_widths",
    "gg_bfs64_all_paths": "test_paths_at_both_cell_widths",
    "gg_bfs_sharded_begin": "test_consumers_of_every_build_form",
    "gg_bfs_sharded_expand": "test_consumers_of_every_build_form",
    "gg_bfs_sharded_words": "test_consumers_of_every_build_form",
    "gg_bfs_sharded_commit": "test_consumers_of_every_build_form",
    "gg_bfs_sharded_pairs": "test_consumers_of_every_build_form",
    "gg_bfs_sharded_levels": "test_consumers_of_every_build_form",
    "gg_walk_closure": "test_closures",
    "gg_reach_closure": "test_closures",
    "gg_level_sets": "test_closures",
    "gg_triangles": "test_triangles",
    "gg_triangles_edges": "test_triangles",
    "gg_khop_aggregate": "test_khop_aggregate",
    "gg_khop_aggregate_top": "test_khop_aggregate_top",
    "gg_khop_pair_counts": "test_khop_pair_counts",
    "gg_edge_weights_create": "test_cheapest",
    "gg_cheapest64": "test_cheapest",
    "gg_cheapest64_paths": "test_cheapest_paths",
    "gg_components": "test_components",
    "gg_result_filter_edge": "test_filter_edge",
    "gg_result_extend_edge": "test_extend_edge",
    "gg_result_group_by": "test_group_by",
    "gg_result_filter_value": "test_filter_value_and_top_rows",
    "gg_result_top_rows": "test_filter_value_and_top_rows",
    "gg_result_distinct": "test_distinct",
    "gg_result_group_tuples": "test_group_tuples",
    "gg_debug_scan": "test_scan_and_sort",
    "gg_debug_sort_pairs": "test_scan_and_sort",
}


# ---- contexts ----------------------------------------------------------------------------------------------------------
def _ctx_with_fill(fill):
    """a context created with GG_POOL_FILL set, the way test_gpu_mirrored_tables.gg_unpaired sets its variable"""
    old = os.environ.get("GG_POOL_FILL")
    os.environ["GG_POOL_FILL"] = fill if isinstance(fill, str) else hex(fill)
    try:
        g = pkg.GG(0)
    finally:
        if old is None:
            del os.environ["GG_POOL_FILL"]
        else:
            os.environ["GG_POOL_FILL"] = old
    return g


def test_the_variable_is_a_byte_in_decimal_or_hex_and_anything_else_is_off():
    for text, want in (("165", 0xA5), ("0xa5", 0xA5), ("0XFF", 0xFF), ("0", 0), ("0x0", 0), ("255", 255), ("256", -1),
                       ("0x100", -1), ("-1", -1), ("a5", -1), ("0x", -1), ("", -1), ("12 ", -1), (" 12", -1), ("1e2", -1)):
        g = _ctx_with_fill(text)
        try:
            assert g.pool_fill() == (want, 0, 0), text
        finally:
            g.close()


class Filled:
    def __init__(self, ctx, fill):
        self.ctx, self.fill = ctx, fill
        self.name = "session" if fill is None else f"{fill:#04x}"


@pytest.fixture(scope="module", params=CONTEXTS, ids=lambda f: "session" if f is None else f"fill_{f:02x}")
def filled(request, _gg_session):
    if request.param is None:
        yield Filled(_gg_session, None)
        return
    g = _ctx_with_fill(request.param)
    yield Filled(g, request.param)
    g.close()


# ---- what a test fetched, as one record per context --------------------------------------------------------------------
_RESULT_METHODS = ("fetch", "fetch_edges", "fetch_triangle_edges", "digest", "rows", "export", "export_reverse",
                   "export_reverse_index", "pairs", "words", "levels")
_RESULT_CLASSES = (ggmod.KhopResult, ggmod.KhopAggregate, ggmod.TupleGroups, ggmod.KhopPairCounts, ggmod.CheapestPaths,
                   ggmod.WalkClosure, ggmod.ReachClosure, ggmod.LevelSets, ggmod.Csr, ggmod.ShardedBfs)
# GG methods whose answer is no result of a device operation (state of the pool, timings, uninitialised host memory)
_NOT_RECORDED = {"pool", "pool_fill", "placement", "profile_get", "host_buffer", "staging_counts", "debug_bfs_steps",
                 "close", "profile", "profile_reset", "profile_select", "debug_reset"}
# the helpers through which the other modules' checks read whole tables (they call the C ABI themselves)
_MODULE_FETCHERS = ("fetch_all", "fetch_ids", "fetch_edges", "read_table")
_KEPT_KEYS = {"rows", "digest", "tables"}  # of a stats dictionary; arrays count under every key
# what a recorded call may return that is no data: handles, nothing, text, timings, flags
_NOT_DATA = _RESULT_CLASSES + (ggmod.DeviceWords, ggmod.EdgeWeights, type(None), str, bytes, float, bool, np.floating, np.bool_)
_M = np.uint64(0x9E3779B97F4A7C15)


def _row_hash(cols):
    """one uint64 per row of the columns (1-D integer arrays of one length)"""
    with np.errstate(over="ignore"):
        h = np.full(cols[0].size, 0x243F6A8885A308D3, np.uint64)
        for c in cols:
            c = np.ascontiguousarray(c)
            u = c.view(np.uint64) if c.dtype.itemsize == 8 else c.astype(np.int64).view(np.uint64)
            h = (h ^ u) * _M
            h ^= h >> np.uint64(29)
        return h


class Record:
    """rows: (where, columns) -> (how many, sum of their hashes mod 2^64); scalars: in call order"""

    def __init__(self):
        self.rows, self.scalars, self.tables = {}, [], 0

    def add(self, where, x):
        if isinstance(x, np.ndarray) and x.dtype.kind in "iub":
            cols = [x] if x.ndim == 1 else [x[:, c] for c in range(x.shape[1])] if x.ndim == 2 else [x.reshape(-1)]
            self._rows(where, cols)
        elif isinstance(x, (tuple, list)):
            arrays = [a for a in x if isinstance(a, np.ndarray) and a.ndim == 1 and a.dtype.kind in "iub"]
            if len(arrays) > 1 and len({a.size for a in arrays}) == 1:  # the columns of one table
                self._rows(where, arrays)
                x = [a for a in x if not any(a is b for b in arrays)]
            for i, a in enumerate(x):
                self.add(f"{where}[{i}]" if isinstance(a, np.ndarray) else where, a)
        elif isinstance(x, dict):
            for k in sorted(x, key=str):
                if k in _KEPT_KEYS or isinstance(x[k], (np.ndarray, dict)):
                    self.add(f"{where}.{k}", x[k])
        elif isinstance(x, (int, np.integer)) and not isinstance(x, bool):
            self.scalars.append((where, int(x)))
        elif isinstance(x, np.ndarray):  # (object or float cells: in order)
            self.scalars.append((where, repr(x.tolist())))
        elif not isinstance(x, _NOT_DATA):
            raise AssertionError(f"{where} returned a {type(x).__name__}: teach Record.add to record it or to leave it out")

    def _rows(self, where, cols):
        self.tables += 1
        key = (where, len(cols))
        n, s = self.rows.get(key, (0, 0))
        h = _row_hash(cols) if cols[0].size else np.zeros(0, np.uint64)
        self.rows[key] = (n + int(cols[0].size), (s + int(h.sum(dtype=np.uint64))) & ((1 << 64) - 1))

    def digest(self):
        return hashlib.sha1(repr((sorted(self.rows.items()), self.scalars)).encode()).hexdigest()


@contextlib.contextmanager
def recording(record):
    """every fetch, export and digest of the result classes and every answer of a GG method goes into `record`"""
    saved = []

    def wrap(cls, name):
        fn = vars(cls)[name]
        if not isinstance(fn, types.FunctionType):
            return
        label = f"{cls.__name__}.{name}"

        def hooked(*a, **kw):
            out = fn(*a, **kw)
            record.add(label, out)
            return out

        saved.append((cls, name, fn))
        setattr(cls, name, hooked)

    for cls in _RESULT_CLASSES:
        for name in _RESULT_METHODS:
            if name in cls.__dict__:
                wrap(cls, name)
    for name in list(ggmod.GG.__dict__):
        if not name.startswith("_") and name not in _NOT_RECORDED:
            wrap(ggmod.GG, name)
    modules = {m.__name__: m for holder in (globals(), vars(t_ids)) for m in holder.values()
               if isinstance(m, types.ModuleType) and m.__name__.startswith("tests.test_gpu_")}
    for module in modules.values():
        for name in _MODULE_FETCHERS:
            if name in vars(module):
                wrap(module, name)
    try:
        yield record
    finally:
        for cls, name, fn in saved:
            setattr(cls, name, fn)


_seen = {}  # test key -> {context name: Record}


@contextlib.contextmanager
def under(filled, key, tables=2):
    """The test's body on one context: the fill is the one asked for before, blocks were filled by the end, and what the
    body fetched is what it fetched on every context that ran it before."""
    ctx = filled.ctx
    ctx.debug_reset()
    fill, blocks_before, _ = ctx.pool_fill()
    assert fill == (-1 if filled.fill is None else filled.fill)
    record = Record()
    try:
        with recording(record):
            yield ctx
    finally:
        ctx.debug_reset()
        ctx.profile(False)
        ctx.staging_clear()
    fill, blocks, nbytes = ctx.pool_fill()
    assert fill == (-1 if filled.fill is None else filled.fill)  # gg_debug_reset leaves the mode alone
    if filled.fill is None:
        assert blocks == nbytes == 0
    else:
        assert blocks > blocks_before and nbytes >= 256 * blocks
    assert record.tables >= tables and (record.tables or record.scalars), (key, record.tables, tables)  # it fetched what it was to
    others = _seen.setdefault(key, {})
    for name, other in others.items():
        if other.digest() != record.digest():
            rows = {k: (v, other.rows.get(k)) for k, v in record.rows.items() if other.rows.get(k) != v}
            rows.update({k: (None, v) for k, v in other.rows.items() if k not in record.rows})
            scalars = [(a, b) for a, b in zip(record.scalars, other.scalars) if a != b][:8]
            raise AssertionError(f"{key}: context {filled.name} and context {name} fetched different bits: rows {rows}, "
                                 f"scalars {scalars} ({len(record.scalars)} / {len(other.scalars)})")
    others[filled.name] = record


# ---- graphs ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def placements(filled):
    """kind -> (the placement's graph, its references, its CSR on the context by the default build with rowids), built
    on first use and kept while the context is the module's"""
    made = {}

    def get(kind):
        if kind not in made:
            eg = EI.edge_graph(kind)
            ctx = filled.ctx
            ctx.debug_reset()
            csr = t_ids._build(ctx, eg.vid, eg.src, eg.dst)
            made[kind] = (eg, EI.references(eg), csr)
            for got, w in zip(csr.export(), AP.csr_of(eg.vid, eg.src, eg.dst)):
                assert np.array_equal(got, w)
            # the walk tables at hops 1 and 2: tail lanes and tail mask words exist
            counts = [csr.E, made[kind][1]["table"].shape[0]]
            assert all(n % 256 for n in counts) and any(n % 64 for n in counts), counts
            ctx.staging_clear()
        return made[kind]

    yield get
    for _, _, csr in made.values():
        csr.close()


def on(*kinds):
    """the placements a test runs under.  One per test where the module's wall time asks for it (every dictionary still
    serves a third of the operations, and the `placements` fixture builds and exports a CSR under each)."""
    return pytest.mark.parametrize("kind", kinds)


@pytest.fixture(scope="module")
def tables(orc):
    """tests/test_gpu_build_forms.py's tables, made once"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = t_forms.Table(orc, name)
        return made[name]

    yield get
    for t in made.values():
        t.close()


def _table(ctx, ref, csr):
    return t_ids._table(ctx, ref, csr)


HIP_MEMCPY_DEVICE_TO_HOST = 2  # hipMemcpyKind


def _hip():
    """the HIP runtime of libgg.so itself, for one device-to-host copy: a second copy of the runtime loaded beside it
    has no device.  (dlsym on a library's handle also searches what the library is linked against.)"""
    return ggmod.load_library()


# ---- CSR builds --------------------------------------------------------------------------------------------------------
def _check_exports(csr, vid, src, dst, rowid, legacy):
    off, nbr, eid, v2 = csr.export()
    want = AP.csr_of(vid, src, dst)
    assert np.array_equal(off, want[0]) and np.array_equal(nbr, want[1]) and np.array_equal(v2, want[3])
    assert np.array_equal(eid, want[2]) if rowid else np.all(eid == -1)
    want_rev = reverse_reference(want[3], src, dst, by_source=legacy)
    assert np.array_equal(csr.export_reverse_index(), want_rev[2])
    for name, a, b in zip(("roff", "rnbr", "rrow"), csr.export_reverse(), want_rev):
        assert np.array_equal(a, b), name


@pytest.mark.parametrize("kind", ["sparse"])
def test_csr_builds(filled, kind):
    """the default build, the multi-pass build and the edge-only build, rowids on and off, rank modes 1 and 2: export(),
    export_reverse_index() and export_reverse() against AP.csr_of and the numpy reverse"""
    eg = EI.edge_graph(kind)
    with under(filled, ("csr_builds", kind), tables=100) as ctx:
        for legacy in (False, True):
            for rowid in (True, False):
                for rank in (1, 2):
                    for edge_only in (False, True):
                        ctx.set_edge_rowid(rowid)
                        ctx.rank_mode(rank)
                        ctx.force_legacy_build(legacy)
                        vid = np.unique(np.concatenate([eg.src, eg.dst])) if edge_only else eg.vid
                        csr = t_mirrored._build(ctx, vid, eg.src, eg.dst, edge_only)
                        try:
                            _check_exports(csr, vid, eg.src, eg.dst, rowid, legacy)
                        finally:
                            csr.close()


def test_mirrored_table_builds(filled, orc):
    """a fully mirrored table: paired densification with and without rowids and from the edges alone
    (test_gpu_mirrored_tables.check); its derived reverse, whose rows the counting calls leave unwritten and the export
    writes (test_gpu_lazy_reverse_rows)"""
    rng = np.random.default_rng(2 * TILE + 1)
    vid = _ids("sparse", 3000, rng)
    src, dst = mirrored(vid, 2 * TILE + 1, rng, extras=True)
    with under(filled, "mirrored_builds") as ctx:
        for rowid in (False, True):
            for edge_only in (False, True):
                t_mirrored.check(ctx, ctx, orc, vid, src, dst, rowid, (1, 2), edge_only)
        src, dst = src[:-1], dst[:-1]  # an even number of rows: the reverse is derived
        rc, g = orc.csr_build(vid, src, dst)
        assert rc == 0
        try:
            want_rev = reverse_reference(g.arrays()[3], src, dst)
            r = {"khop12": g.khop(1, 2), "khop22": g.khop(2, 2)}
            csr = t_lazy._build(ctx, vid, src, dst)
            try:
                assert csr.reverse_derived == 1 and not csr.reverse_rows_ready
                got = t_lazy._counting(ctx, csr, g.V)
                assert not csr.reverse_rows_ready
                t_lazy._check_counting(got, r)
                assert np.array_equal(csr.export_reverse_index(), want_rev[2])
                for name, a, b in zip(("roff", "rnbr", "rrow"), csr.export_reverse(), want_rev):
                    assert np.array_equal(a, b), name
                assert csr.reverse_rows_ready and t_lazy._counting(ctx, csr, g.V) == got
            finally:
                csr.close()
        finally:
            g.close()


# form -> (dictionary kind, table) of tests/test_gpu_build_forms.py: every form once, every kind twice
FORMS = {"leaf_rowid": ("sparse", "a_plain"), "vertex_sorted": ("dense", "a_plain"), "derived": ("wide", "a_mirrored"),
         "mask_ranks": ("dense", "a_mirrored"), "multipass_rowid": ("wide", "a_mirrored"), "multipass": ("sparse", "a_plain")}
CONSUMERS = {
    "shortest_paths": t_forms.test_shortest_paths,
    "middle_vertex_two_hop": t_forms.test_middle_vertex_two_hop,
    "walk_counts_and_three_hops": t_forms.test_walk_counts_and_three_hop_expansion,
    "bfs_output_forms": t_forms.test_bfs_in_every_output_form,
    "endpoints_reach_and_level_sets": t_forms.test_seeded_endpoints_reach_closure_and_level_sets,
    "two_hop_walks_with_rowids": t_forms.test_two_hop_walks_with_edge_rowids,
}


# every consumer on a form with rowids and on one without, every form twice
CONSUMER_FORMS = {
    "shortest_paths": ("leaf_rowid", "derived"),
    "middle_vertex_two_hop": ("vertex_sorted", "multipass"),
    "walk_counts_and_three_hops": ("mask_ranks", "multipass_rowid"),
    "bfs_output_forms": ("derived", "multipass"),
    "endpoints_reach_and_level_sets": ("vertex_sorted", "multipass_rowid"),
    "two_hop_walks_with_rowids": ("leaf_rowid", "mask_ranks"),
}
assert sorted(CONSUMER_FORMS) == sorted(CONSUMERS) and {f for fs in CONSUMER_FORMS.values() for f in fs} == set(FORMS)


@pytest.mark.parametrize("consumer,form", [(c, f) for c in sorted(CONSUMER_FORMS) for f in CONSUMER_FORMS[c]])
def test_consumers_of_every_build_form(filled, tables, consumer, form):
    """tests/test_gpu_build_forms.py's consumers on a CSR of every form gg_csr_build makes: shortest paths, the
    middle-vertex 2-hop forms, khop_count and expand_khop with force_frontier off and on, bfs64 / pairs / packed pairs /
    the sharded BFS, walk_endpoints, reach_closure on both visited sets, level_sets on every set and order mode, walks
    with their edge rowids"""
    kind, name = FORMS[form]
    with under(filled, ("form", form, consumer)) as ctx:
        CONSUMERS[consumer](ctx, None, tables, form, kind, name)


def test_sharded_builds(filled, orc):
    with under(filled, "sharded_builds", tables=0) as ctx:
        t_parity.test_each_shard_matches_oracle_sharded_the_same_way(ctx, orc)


def test_lookup_and_join_probe(filled, orc):
    with under(filled, "lookup_join") as ctx:
        t_parity.test_csr_lookup_and_pinned_host_buffers(ctx, orc)
        t_parity.test_join_probe_returns_every_matching_build_row_per_probe_key(ctx, orc)


# ---- k-hop -------------------------------------------------------------------------------------------------------------
@on("wide")
def test_khop(filled, orc, placements, kind):
    """khop_count, expand_khop counted and materialised for 1..3 hops, expand_khop_result with its digest, expand_khop_edges,
    closed_walks, the range and the middle-vertex forms and the device-resident result words, with force_frontier off and
    on, against the C oracle"""
    eg, ref, csr = placed = placements(kind)
    S = ref["table_sources"]
    rc, g = orc.csr_build(eg.vid, eg.src, eg.dst)
    assert rc == 0
    try:
        dense = g.lookup(S)
        dense = dense[dense >= 0].astype(np.uint32)
        whole, listed = g.khop(1, 3), g.khop(1, 3, sources_dense=dense)
        with under(filled, ("khop", eg.kind), tables=20) as ctx:
            for knob in (0, 1):
                ctx.force_frontier(knob)
                assert ctx.khop_count(csr, 1, 3)[1:4] == whole["rows"][1:4]
                assert ctx.khop_count(csr, 1, 3, sources=S)[1:4] == listed["rows"][1:4]
                assert ctx.expand_khop(csr, 1, 3) == whole and ctx.expand_khop(csr, 1, 3, sources=S) == listed
                for k, sources, sd in ((1, None, None), (2, None, None), (1, S, dense), (2, S, dense), (3, S, dense)):
                    want = g.khop_rows(k, k, sources_dense=sd)[k]
                    counted = g.khop(k, k, sources_dense=sd)
                    res = ctx.expand_khop_result(csr, k, sources)
                    try:
                        assert res.digest(csr, k) == (counted["rows"][k], counted["digest"][k]) and res.rows(k) == want.shape[0]
                        assert np.array_equal(sort_rows(t_deep.read_table(res, k)), sort_rows(want)), (knob, k)
                    finally:
                        res.close()
                got = ctx.expand_khop(csr, 1, 3, sources=S, materialise=True)
                for h in (1, 2, 3):
                    assert np.array_equal(sort_rows(got["tables"][h]), sort_rows(g.khop_rows(h, h, sources_dense=dense)[h]))
            ctx.force_frontier(0)
            # walks with their edge rowids (append positions): edge j of every row is the table row (v_j-1, v_j)
            res = ctx.expand_khop_edges(csr, EI.TABLE_HOPS, S)
            try:
                v = t_extend.fetch_all(res, EI.TABLE_HOPS)
                e = t_extend.fetch_all(res, EI.TABLE_HOPS, edges=True)
                assert np.array_equal(sort_rows(v), sort_rows(ref["table"]))
                for j in range(EI.TABLE_HOPS):
                    assert np.array_equal(np.stack([eg.src[e[:, j]], eg.dst[e[:, j]]], axis=1), v[:, j:j + 2])
            finally:
                res.close()
            # closed 3-edge walks from the list = the 2-hop table filtered by an edge back to its start
            want_rows, want_st = ref["filter"][(2, 0, "inner")]
            st, res = ctx.closed_walks(csr, 3, S)
            try:
                assert st == want_st and np.array_equal(t_extend.fetch_all(res, 2), want_rows)
            finally:
                res.close()
            # source ranges and middle-vertex ranges partition the 1- and 2-hop result
            two = g.khop(1, 2)
            b = ctx.khop_partition(csr, 3)
            assert b[0] == 0 and b[-1] == csr.V
            for lo, hi in zip(b, b[1:]):
                assert ctx.expand_khop_range(csr, lo, hi, 1, 2) == g.khop(1, 2, lo=lo, hi=hi)
            b = ctx.khop_partition_mid(csr, 3)
            assert b[0] == 0 and b[-1] == csr.V
            rows, dig, mid_rows = [0, 0, 0], [0, 0, 0], []
            for lo, hi in zip(b, b[1:]):
                st = ctx.expand_khop_mid(csr, lo, hi)
                for h in (1, 2):
                    rows[h] += st["rows"][h]
                    dig[h] = t_parity.dsum(dig[h], st["digest"][h])
                res = ctx.expand_khop_mid_result(csr, lo, hi)
                try:
                    n, d = res.digest(csr, 2)
                    assert (n, d & 0xFFFFFFFF) == (st["rows"][2], st["digest"][2] & 0xFFFFFFFF)
                    mid_rows.append(t_deep.read_table(res, 2))
                finally:
                    res.close()
            assert rows[1:] == two["rows"][1:3] and dig[1:] == [x & 0xFFFFFFFF for x in two["digest"][1:3]]
            assert np.array_equal(sort_rows(np.concatenate(mid_rows)), sort_rows(g.khop_rows(2, 2)[2]))
            # the six result words left on the device.  Nothing waits for them and the library's stream is non-blocking: the
            # expand_khop call between the two reads its own counters back, which synchronises that stream before the copy
            words = ctx.expand_khop_dev(csr, 1)
            want = sharding.stats_to_vec(ctx.expand_khop(csr, 1, 2))
            vec = np.zeros(words.n, np.uint64)
            assert _hip().hipMemcpy(ctypes.c_void_p(vec.ctypes.data), ctypes.c_void_p(words.ptr), vec.nbytes, HIP_MEMCPY_DEVICE_TO_HOST) == 0
            got = [int(x) & 0xFFFFFFFF if i in sharding.LANEWISE else int(x) for i, x in enumerate(vec)]
            assert got == [w & 0xFFFFFFFF if i in sharding.LANEWISE else w for i, w in enumerate(want)]
    finally:
        g.close()


def test_deep_walks_at_five_hops(filled, orc):
    """the 5-hop tables of tests/deep_graphs.multigraph: all sources, a list and a range under both frontier knobs, and
    the walks with their edge rowids"""
    with under(filled, "deep_walks") as ctx:
        t_deep.test_deep_materialised_tables_and_their_digests(ctx, orc, "multigraph", 5, 5)
        t_deep.test_deep_walks_with_their_edge_rowids(ctx, orc, "multigraph", 5)


@pytest.mark.parametrize("form,kind", [("leaf_rowid", "sparse"), ("derived", "wide")])
def test_same_neighbour_filter_at_five_hops(filled, orc, form, kind):
    with under(filled, ("same_neighbour", form)) as ctx:
        t_forms.test_same_neighbour_filter_over_a_filter_csr_of_every_form(ctx, None, orc, form, kind)


# ---- paths -------------------------------------------------------------------------------------------------------------
def test_bfs_levels_at_both_cell_widths(filled):
    """bfs64 level by level (test_gpu_bfs_levels.check) on a push-and-pull shape with one-byte cells, and on the 333-level
    shape with two-byte cells in all 64 lanes, with its pairs and packed pairs"""
    with under(filled, "bfs_levels") as ctx:
        for name in ("transitions_push", "late_pull_6"):
            s = bfs_shapes.shape(name)
            csr = t_bfs.build(ctx, s)
            try:
                r, rd = t_bfs.check(ctx, csr, s, built_for=s.directions)
                assert rd["cell_bytes"] == 1
            finally:
                csr.close()
        t_bfs.test_two_byte_cells_in_all_64_lanes_with_pull_levels_past_254(ctx, bfs_shapes.shape("deep_all_lanes"))


@on("wide")
def test_paths_at_both_cell_widths(filled, placements, kind):
    """shortest_paths, all_shortest_paths, shortest_path_counts and the bfs64 pairs between edge ids (one-byte cells), and
    the paths traced off two-byte cells"""
    eg, ref, csr = placed = placements(kind)
    with under(filled, ("paths", eg.kind)) as ctx:
        t_ids.test_bfs_pairs_and_shortest_paths_between_edge_ids(ctx, placed)
        s, t = EI.path_pairs(eg)
        off, nbr, eid, vid = AP.csr_of(eg.vid, eg.src, eg.dst)
        for got, want in zip(ctx.shortest_path_counts(csr, s, t), AP.shortest_path_counts(off, nbr, vid, s, t)):
            assert got.dtype == want.dtype and np.array_equal(got, want)
        deep = bfs_shapes.shape("deep_all_lanes")
        t_bfs.test_paths_off_two_byte_cells(ctx, deep, True)
        t_bfs.test_all_paths_off_two_byte_cells(ctx, deep, False)


# ---- closures ----------------------------------------------------------------------------------------------------------
@on("sparse")
def test_closures(filled, placements, kind):
    """walk_closure (a forest 60 deep, and the edge-id graph bounded at two levels), reach_closure with the bitmap and the
    hash visited set, level_sets on every set and order mode"""
    eg, ref, csr = placed = placements(kind)
    seeds = eg.sources()
    classes = (np.arange(seeds.size) % 3).astype(np.uint32)
    seen = (np.arange(seeds.size) % 2).astype(bool)
    with under(filled, ("closures", eg.kind)) as ctx:
        t_walk.check(ctx, eg.src, eg.dst, seeds[:6], max_levels=2)
        src, dst, ids = t_walk.forest(np.random.default_rng(17), 3000, 30, 60)
        assert len(t_walk.check(ctx, src, dst, ids[:30])) >= 60
        t_reach.check(ctx, eg.src, eg.dst, seeds, classes, seen)
        t_levels.check(ctx, eg.src, eg.dst, seeds, classes, max_levels=4)


# ---- triangles ---------------------------------------------------------------------------------------------------------
@on("wide")
def test_triangles(filled, orc, placements, kind):
    """counts, rows and edge rows in both orders, from every vertex and from a list; with the small LDS tiles"""
    eg, ref, csr = placed = placements(kind)
    with under(filled, ("triangles", eg.kind)) as ctx:
        for tile in (0, 64, 4):
            for order in (0, 1):
                for which in ("all", "list"):
                    ctx.debug_triangle_tile(tile)
                    t_ids.test_triangles_count_and_rows(ctx, orc, placed, order, which)
                    t_ids.test_triangle_edges(ctx, placed, order, which)


# ---- aggregates over walks ---------------------------------------------------------------------------------------------
@on("dense_zero")
def test_khop_aggregate(filled, placements, kind):
    """by start and by end vertex; every in-row a long one, none, and the default threshold"""
    eg, ref, csr = placed = placements(kind)
    with under(filled, ("aggregate", eg.kind)) as ctx:
        for long_row in (0, 1, NO_LONG_ROWS):
            for group_by in t_ids.K.GROUPS:
                ctx.debug_aggregate_long_row(long_row)
                t_ids.test_khop_aggregate(ctx, placed, group_by)


@on("sparse")
def test_khop_aggregate_top(filled, placements, kind):
    """the LDS sort and the global one (the routes of gg_debug_aggregate_top), n below, at and above the group count"""
    eg, ref, csr = placed = placements(kind)
    with under(filled, ("aggregate_top", eg.kind)) as ctx:
        t_ids.test_khop_aggregate_top_when_the_id_alone_decides(ctx, placed, "end")
        t_ids.test_khop_aggregate_top_of_weighted_totals(ctx, placed)


PULL_KNOBS = [(1, 0), (NO_LONG_ROWS, 0), (0, 1)]  # (long-row threshold, gather mode) next to the default (0, 0)


@on("wide")
def test_khop_pair_counts(filled, placements, kind):
    """with a target list and without; every in-row a long one, none, and every row gathered"""
    eg, ref, csr = placed = placements(kind)
    with under(filled, ("pair_counts", eg.kind)) as ctx:
        for long_row, gather_mode in [(0, 0)] + PULL_KNOBS:
            ctx.debug_pair_counts(long_row, gather_mode)
            t_pairs.check(ctx, csr, eg.tri, 1, 2, ref["sources"], ref["pair_targets"], ref["pair_counts"],
                          gather_all=gather_mode == 1)
            t_pairs.check(ctx, csr, eg.tri, 1, 2, ref["sources"], None, ref["pair_counts_all"], gather_all=gather_mode == 1)


_weighted = {}


def _weighted_graph(eg, lo_hi):
    key = (eg.kind, lo_hi)
    if key not in _weighted:
        wt = CR.hashed_weights(eg.src.size, *lo_hi)
        _weighted[key] = (wt, CR.WeightedGraph(eg.vid, eg.src, eg.dst, wt), {})
    return _weighted[key]


@on("dense_zero")
def test_cheapest(filled, placements, kind):
    """tests/test_gpu_cheapest.py's edge-id case under both knobs of gg_debug_cheapest"""
    eg, ref, csr = placed = placements(kind)
    wt, g, memo = _weighted_graph(eg, ())
    S = np.concatenate([np.asarray(eg.named, np.int64), np.asarray(eg.wired, np.int64)[:20], [eg.hub], EI.LISTED])[:64]
    targets = np.concatenate([np.asarray(eg.named, np.int64), EI.LISTED])
    if "all" not in memo:
        memo["all"], memo["cut"] = CR.cheapest(g, S, -1, None), CR.cheapest(g, S, 2, targets)
    with under(filled, ("cheapest", eg.kind)) as ctx:
        w = ctx.edge_weights(csr, wt)
        try:
            for long_row, gather_mode in [(0, 0)] + PULL_KNOBS:
                ctx.debug_cheapest(long_row, gather_mode)
                got = t_cheapest.check(ctx, csr, w, g, S, -1, None, memo["all"], gather_all=gather_mode == 1)
                assert set(np.asarray(eg.named).tolist()) <= set(got[1].tolist())
                t_cheapest.check(ctx, csr, w, g, S, 2, targets, memo["cut"], gather_all=gather_mode == 1)
        finally:
            w.close()


@on("sparse")
def test_cheapest_paths(filled, placements, kind):
    """the traced paths of a 64-source batch to a target list, and of any number of pairs, under both knobs"""
    eg, ref, csr = placed = placements(kind)
    wt, g, memo = _weighted_graph(eg, (0, 3))
    S = np.concatenate([np.asarray(eg.named, np.int64), np.asarray(eg.wired, np.int64)[:20], [eg.hub], EI.LISTED])[:64]
    ends = np.concatenate([np.asarray(eg.named, np.int64), np.asarray(eg.wired, np.int64)[::3], [eg.hub], EI.LISTED])
    lanes, targets = t_cheapest_paths.all_pairs(S, ends)
    s, d = EI.path_pairs(eg)
    if "batch" not in memo:
        memo["batch"], memo["pairs"] = PR.paths(g, S, lanes, targets), PR.pair_paths(g, s, d)
    with under(filled, ("cheapest_paths", eg.kind)) as ctx:
        w = ctx.edge_weights(csr, wt)
        try:
            for long_row, gather_mode in [(0, 0), (1, 0), (0, 1)]:
                ctx.debug_cheapest(long_row, gather_mode)
                rows, pairs, st = t_cheapest_paths.check(ctx, csr, w, g, S, lanes, targets, want=memo["batch"],
                                                         gather_all=gather_mode == 1)
                assert st["rows"] > 0
                assert PR.same_rows(ctx.cheapest_paths(csr, w, s, d), memo["pairs"]["rows"])
        finally:
            w.close()


@on("wide")
def test_components(filled, placements, kind):
    """both init modes and both jump schedules (test_gpu_components.check), on one component and on many"""
    eg, ref, csr = placed = placements(kind)
    with under(filled, ("components", eg.kind)) as ctx:
        t_ids.test_components(ctx, placed)


# ---- row operators -----------------------------------------------------------------------------------------------------
@on("wide")
def test_filter_edge(filled, orc, placements, kind):
    eg, ref, csr = placed = placements(kind)
    with under(filled, ("filter_edge", eg.kind)) as ctx:
        t_ids.test_filter_edge(ctx, orc, placed)


@on("dense_zero")
def test_extend_edge(filled, placements, kind):
    """from every column, with and without edge columns; with the small tile"""
    eg, ref, csr = placed = placements(kind)
    with under(filled, ("extend_edge", eg.kind)) as ctx:
        for tile in (0, t_extend.SMALL_TILE):
            ctx.debug_extend(tile)
            t_ids.test_extend_edge(ctx, placed)


@on("sparse")
def test_group_by(filled, placements, kind):
    """the LDS route and the global one, every key and weight column"""
    eg, ref, csr = placed = placements(kind)
    with under(filled, ("group_by", eg.kind)) as ctx:
        t_ids.test_group_by_on_both_routes(ctx, placed)


@on("wide")
def test_filter_value_and_top_rows(filled, placements, kind):
    """tests/test_gpu_value_rows.py's edge-id case: filter_value in and not_in, top_rows on both sort routes"""
    eg, ref, csr = placed = placements(kind)
    with under(filled, ("value_rows", eg.kind)) as ctx:
        t_value.test_edge_case_ids_as_cells_and_as_tie_ids_under_every_dictionary(ctx, eg.kind)


@on("dense_zero")
def test_distinct(filled, placements, kind):
    """every column set with combine on and off; the slot count forced to its minimum"""
    eg, ref, csr = placed = placements(kind)
    with under(filled, ("distinct", eg.kind)) as ctx:
        t_distinct.test_edge_case_ids_under_both_csr_builds(ctx, eg.kind, False)
        t_distinct.test_slots_forced_to_the_minimum_and_around_the_default(ctx)


TUPLE_COLUMNS = [[0], [2], [0, 2], [2, 1, 0]]


@on("sparse")
def test_group_tuples(filled, placements, kind):
    """the count form and the valued forms (test_gpu_group_tuples.check_forms) with the groups in LDS and in global memory"""
    eg, ref, csr = placed = placements(kind)
    with under(filled, ("group_tuples", eg.kind)) as ctx:
        table = _table(ctx, ref, csr)
        try:
            for route in (1, 2):
                ctx.debug_group_tuples(route)
                for cols in TUPLE_COLUMNS:
                    t_tuples.check_forms(ctx, table, EI.TABLE_HOPS, ref["table"], cols, csr, eg.vid, ref["weights"],
                                         knob=(route, 0))
        finally:
            table.close()


# ---- primitives --------------------------------------------------------------------------------------------------------
def test_scan_and_sort(filled):
    """the chained scan over 66 and 130 tiles (two and three look-back trips), the radix sort over 66 tiles with two and
    four passes, and with keys that are no element"""
    with under(filled, "scan_sort") as ctx:
        for n in t_scan.SCAN_N[-2:]:
            for width in (4, 8):
                t_scan.test_scan_matches_cumsum(ctx, n, width)
        for key_bits in (9, 31):
            t_scan.test_sort_matches_stable_argsort(ctx, t_scan.SORT_N[-1], key_bits)
        t_scan.test_sort_drops_the_no_element_key(ctx, t_scan.SORT_N[-1], 17)


# ---- lifetime ----------------------------------------------------------------------------------------------------------
def _fetch_every_kind(lib, results):
    out = {}
    for name, kind, cols, total_of, call in t_kinds.FETCHERS:
        total = total_of(lib, results[kind])
        total = total[0] if isinstance(total, tuple) else total
        n, whole = t_kinds.fetch(lib, call, results[kind], cols, 0, total + 10)
        assert n == total >= 3, name
        out[name] = whole
    return out


def _same_fetches(a, b):
    assert sorted(a) == sorted(b)
    for name in a:
        for x, y in zip(a[name], b[name]):
            assert x.dtype == y.dtype and np.array_equal(x, y), name


def _churn(ctx, orc):
    """one call of every operation above on another graph, every result closed: their blocks go back to the pool and the
    next calls take them"""
    eg = EI.edge_graph("sparse")
    ref = EI.references(eg)
    S = ref["table_sources"]
    for legacy, edge_only in ((True, False), (False, True)):  # the multi-pass and the edge-only build, with their exports
        ctx.force_legacy_build(legacy)
        vid = np.unique(np.concatenate([eg.src, eg.dst])) if edge_only else eg.vid
        built = t_mirrored._build(ctx, vid, eg.src, eg.dst, edge_only)
        try:
            _check_exports(built, vid, eg.src, eg.dst, True, legacy)
        finally:
            built.close()
    ctx.force_legacy_build(False)
    csr = t_ids._build(ctx, eg.vid, eg.src, eg.dst)
    placed = (eg, ref, csr)
    try:
        t_ids.test_triangles_count_and_rows(ctx, orc, placed, 0, "all")
        t_ids.test_triangle_edges(ctx, placed, 1, "list")
        t_ids.test_khop_aggregate(ctx, placed, "end")
        t_ids.test_khop_aggregate_top_of_weighted_totals(ctx, placed)
        for long_row, gather_mode in [(0, 0)] + PULL_KNOBS:
            ctx.debug_pair_counts(long_row, gather_mode)
            t_pairs.check(ctx, csr, eg.tri, 1, 2, ref["sources"], ref["pair_targets"], ref["pair_counts"],
                          gather_all=gather_mode == 1)
        ctx.debug_pair_counts(0, 0)
        t_ids.test_components(ctx, placed)
        t_ids.test_bfs_pairs_and_shortest_paths_between_edge_ids(ctx, placed)
        t_ids.test_filter_edge(ctx, orc, placed)
        t_ids.test_extend_edge(ctx, placed)
        t_ids.test_group_by_on_both_routes(ctx, placed)
        t_walk.check(ctx, eg.src, eg.dst, eg.sources()[:6], max_levels=2)
        t_reach.check(ctx, eg.src, eg.dst, eg.sources())
        t_levels.check(ctx, eg.src, eg.dst, eg.sources(), max_levels=3)
        t_value.test_edge_case_ids_as_cells_and_as_tie_ids_under_every_dictionary(ctx, eg.kind)
        t_distinct.test_edge_case_ids_under_both_csr_builds(ctx, eg.kind, False)
        table = _table(ctx, ref, csr)
        try:
            t_tuples.check_forms(ctx, table, EI.TABLE_HOPS, ref["table"], [0, 2], csr, eg.vid, ref["weights"])
        finally:
            table.close()
        wt, g, memo = _weighted_graph(eg, ())
        sources = np.concatenate([np.asarray(eg.named, np.int64), np.asarray(eg.wired, np.int64)[:20], [eg.hub], EI.LISTED])[:64]
        if "all" not in memo:
            memo["all"] = CR.cheapest(g, sources, -1, None)
        w = ctx.edge_weights(csr, wt)
        try:
            for long_row, gather_mode in [(0, 0)] + PULL_KNOBS:
                ctx.debug_cheapest(long_row, gather_mode)
                t_cheapest.check(ctx, csr, w, g, sources, -1, None, memo["all"], gather_all=gather_mode == 1)
            ctx.debug_cheapest(0, 0)
            s, d = EI.path_pairs(eg)
            ctx.cheapest_paths(csr, w, s, d)
        finally:
            w.close()
        assert ctx.expand_khop(csr, 1, 3)["rows"][3] > 0 and ctx.khop_count(csr, 1, 3)[3] > 0
        ctx.expand_khop_edges(csr, 2, S).close()
        want_rows, want_st = ref["filter"][(2, 0, "inner")]
        st, res = ctx.closed_walks(csr, 3, S)
        try:
            assert st == want_st and np.array_equal(t_extend.fetch_all(res, 2), want_rows)
        finally:
            res.close()
        half = csr.V // 2
        whole = ctx.expand_khop(csr, 1, 2)
        for form in (ctx.expand_khop_range, ctx.expand_khop_mid):  # the range and the middle-vertex forms
            parts = [form(csr, 0, half, 1, 2), form(csr, half, csr.V, 1, 2)]
            assert [sum(p["rows"][h] for p in parts) for h in (1, 2)] == whole["rows"][1:3]
        res = ctx.expand_khop_mid_result(csr, 0, half)
        try:
            assert res.rows(2) == ctx.expand_khop_mid(csr, 0, half)["rows"][2]
        finally:
            res.close()
        assert ctx.connected_paths_same_neighbour(csr, csr, 2, S).shape[1] == 4  # rows (w, v0, v1, v2)
        shape = bfs_shapes.shape("transitions_push")
        levels = t_bfs.build(ctx, shape)
        try:
            t_bfs.check(ctx, levels, shape, built_for=shape.directions)
        finally:
            levels.close()
        ctx.debug_scan(np.ones(65 * t_scan.TILE + 1, np.uint32))
        ctx.debug_sort_pairs(np.arange(5000, dtype=np.uint32)[::-1] % 511, np.arange(5000, dtype=np.uint32), key_bits=9)
    finally:
        csr.close()
        ctx.debug_reset()


def _same_columns(got, want, what):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and np.array_equal(a, b), what


def test_results_and_lazy_csr_parts_outlive_the_calls_that_recycle_their_neighbours(filled, orc, _gg_session):
    """(What the 0xA5 context is for; the others run it too.)  Kept open across two rounds of churn:

      - one result of every kind of tests/test_gpu_result_kinds.py;
      - that graph's CSR (29 rows with rowids, not mirrored: its reverse rows and row index come from the build), with the
        reverse-by-source copy and its positions that the first shortest_paths call builds, read again by shortest_paths
        with edges and by the triangle edge rows;
      - a fully mirrored table's CSR whose build derived the reverse: its row index (ensure_reverse_index) and its reverse
        rows (ensure_reverse) are written on first use, here by the exports before the churn, and its own reverse-by-source
        copy by shortest_paths without edges.

    The churn is one call of every operation, its results closed.  After each round every kept result and every part of
    both CSRs is read again and compared bit for bit with its first read and with the reference — a column that never got
    ctx->keep() would hold the fill byte or a stranger's rows by now (and the pool's count of blocks in use says at once whether
    the two parts written on first use were kept).  Afterwards the pool has as many blocks in use as
    before."""
    V, S, D, R = t_kinds.VID, t_kinds.SRC, t_kinds.DST, t_kinds.ROWID
    # the reference: the same results on the unfilled session context
    base = _gg_session
    base.debug_reset()
    base.staging_clear()
    base.append_vertices(V)
    base.append_edges(S, D, R)
    csr0, results0 = base.build_csr(), {}
    try:
        t_kinds.make_results(base, csr0, results0)
        reference = _fetch_every_kind(base.lib, results0)
    finally:
        for res in results0.values():
            base.lib.gg_result_destroy(res)
        csr0.close()
        base.staging_clear()
    # the mirrored table: 2400 rows over 300 vertices, with self-loops, duplicate rows and dangling ids
    rng = np.random.default_rng(2400)
    m_vid = _ids("sparse", 300, rng)
    m_src, m_dst = mirrored(m_vid, 2400, rng, extras=True)
    rc, g = orc.csr_build(m_vid, m_src, m_dst)
    assert rc == 0
    try:
        m_arrays = g.arrays()
    finally:
        g.close()
    m_rev = reverse_reference(m_arrays[3], m_src, m_dst)
    ends = np.concatenate([m_vid[:12], [int(m_vid.max()) + 1]]).astype(np.int64)
    m_s, m_t = np.repeat(ends, ends.size), np.tile(ends, ends.size)
    m_paths = t_ids.SP.shortest_paths(m_arrays[0], m_arrays[1], m_arrays[2], m_arrays[3], m_s, m_t, -1, False)
    assert m_paths[0].size > 100
    # the small graph: every vertex to every vertex, and its triangle edge rows
    want_csr = AP.csr_of(V, S, D, R)
    want_rev = reverse_reference(want_csr[3], S, D)
    k_s, k_t = np.repeat(V, V.size), np.tile(V, V.size)
    k_paths = t_ids.SP.shortest_paths(*want_csr, k_s, k_t, -1, True)
    k_triangles = sort_rows(t_ids.E.rows(V, S, D, R, 0, None))
    assert k_paths[0].size > 50 and k_triangles.shape[0] == 18
    with under(filled, "lifetime", tables=40) as ctx:
        in_use = ctx.pool()[1]
        ctx.append_vertices(V)
        ctx.append_edges(S, D, R)
        csr, results, derived = ctx.build_csr(), {}, None
        try:
            derived = t_lazy._build(ctx, m_vid, m_src, m_dst)  # (no rowids, rank mode 1: the form that derives)
            ctx.debug_reset()
            assert derived.reverse_derived == 1 and not derived.reverse_rows_ready and not derived.reverse_index_ready
            assert not csr.reverse_derived and csr.reverse_rows_ready

            def read_again(first_time=False):
                for got, w in zip(csr.export(), want_csr):
                    assert np.array_equal(got, w)
                assert np.array_equal(csr.export_reverse_index(), want_rev[2])
                _same_columns(csr.export_reverse(), want_rev, "the small graph's reverse")
                _same_columns(ctx.shortest_paths(csr, k_s, k_t, -1, True), k_paths, "paths with edges")
                t_ids.t_tri_edges.check(ctx, csr, k_triangles, 0, None, R)
                off, nbr, eid, vid = derived.export()
                _same_columns((off, nbr, vid), (m_arrays[0], m_arrays[1], m_arrays[3]), "the mirrored table's forward rows")
                assert np.all(eid == -1)
                held = ctx.pool()[1]
                assert np.array_equal(derived.export_reverse_index(), m_rev[2])
                assert derived.reverse_index_ready and (derived.reverse_rows_ready or first_time)
                # the row index written on first use stays handed out when its call has ended: one block more, kept
                assert ctx.pool()[1] == held + (1 if first_time else 0)
                _same_columns(derived.export_reverse(), m_rev, "the derived reverse, written on first use")
                assert derived.reverse_rows_ready
                assert ctx.pool()[1] == held + (2 if first_time else 0)  # and the rotated reverse rows
                _same_columns(ctx.shortest_paths(derived, m_s, m_t, -1, False), m_paths, "paths over the derived reverse")

            read_again(first_time=True)
            t_kinds.make_results(ctx, csr, results)
            first = _fetch_every_kind(ctx.lib, results)
            _same_fetches(first, reference)
            for _ in range(2):
                _churn(ctx, orc)
                _same_fetches(_fetch_every_kind(ctx.lib, results), first)
                read_again()
        finally:
            for res in results.values():
                ctx.lib.gg_result_destroy(res)
            csr.close()
            if derived is not None:
                derived.close()
        ctx.staging_clear()
        assert ctx.pool()[1] == in_use
