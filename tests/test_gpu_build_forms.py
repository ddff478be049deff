"""Every consumer of a CSR on every form gg_csr_build makes, under every id dictionary.

gg_csr_build takes one of six routes (FORMS below); the other GPU tests prove that all of them export the same
off / nbr / vid, and then run nearly everything else on the first one with sparse ids.  Here each consumer that reads
state the routes fill differently (epos / eid, row, rrow / rnbr and who wrote them, the lazily built reverse-by-source
copy, the lazily built 16-byte id table) runs on each route and each dictionary kind, against the C oracle and the numpy
restatements the suite already has.  Everything is integer: every comparison is exact.

build_form() proves that the build took the route it names -- from the kernels the profiler saw, reverse_derived and
the exported rowids -- so a knob that stops selecting its route fails here instead of repeating another form's test.

The tables live in position space (vertex = its position in the vertex table, which is its dense index on every
route): one oracle CSR and one set of references per table serve the three dictionary kinds, whose ids are put on
afterwards.  As every form of a table is compared with the same reference object, equal rows across the forms follow;
the shortest-path test checks it directly as well."""
import hashlib

import numpy as np
import pytest

from duckdb_pgq_amd import GGError
from tests import deep_graphs
from tests import shortest_path_ref as ref
from tests.oracle_lib import endpoint_sets, exact_walk_counts, sort_rows
from tests.test_gpu_deep_walks import launched, read_table
from tests.test_gpu_derived_reverse import TILE, _ctx_with_env, _ids, mirrored
from tests.test_gpu_level_sets import COMBINATIONS, exact_levels
from tests.test_gpu_parity import dsum
from tests.test_gpu_reach_closure import exact_reach
from tests.test_gpu_walk_closure import exact_closure, forest

pytestmark = pytest.mark.gpu

GG_ERR_STATE = -6

# (1) bucketed leaf geometry with edge rowids, (2) vertex-sorted, (3) vertex-sorted with the derived reverse, (4) bucketed
# with match-mask ranks and no rowids, (5) the multi-pass build with and without rowids; (6) LEAF_BIG has its own test
FORMS = ["leaf_rowid", "vertex_sorted", "derived", "mask_ranks", "multipass_rowid", "multipass"]
LEAF_BIG = "leaf_big"
HAS_ROWID = {"leaf_rowid", "multipass_rowid"}
KEEPS_ROW = {"multipass_rowid", "multipass"}  # csr->row: gg_bfs64_paths need not rebuild it (path_entry_rows)
KINDS = ["dense", "sparse", "wide"]


@pytest.fixture(scope="module")
def _gg_sorted_module():
    """A second context that never derives (GG_MIRROR_REVERSE=0 at its creation): the vertex-sorted form of a fully
    mirrored table exists only there."""
    g = _ctx_with_env("GG_MIRROR_REVERSE")
    yield g
    g.close()


@pytest.fixture
def gg_sorted(_gg_sorted_module):
    g = _gg_sorted_module
    g.debug_reset()
    yield g
    g.debug_reset()
    g.profile(False)
    g.staging_clear()


# ---- forms -------------------------------------------------------------------------------------------------------------
def _knobs(ctx, form):
    ctx.debug_reset()
    ctx.set_edge_rowid(form in HAS_ROWID)
    ctx.rank_mode(2 if form == "mask_ranks" else 1 if form in ("vertex_sorted", "derived") else 0)
    ctx.force_legacy_build(form in KEEPS_ROW)


def _build(ctx, form, vid, src, dst, rowid):
    _knobs(ctx, form)
    ctx.staging_clear()
    ctx.append_vertices(vid)
    ctx.append_edges(src, dst, rowid)
    return launched(ctx, ctx.build_csr)


def build_form(gg, form, vid, src, dst, rowid=None, sorted_ctx=None):
    """Set the knobs of `form`, build, and prove that the build took that route; returns (context, csr).  The context is
    gg, except for the vertex-sorted form of a table that gg derives the reverse of: that one is built on sorted_ctx.

    What tells the routes apart (gg_csr_fast.hip, csr_build_fast): the multi-pass build launches densify_hist and no
    partition_dual; of the bucketed builds only the vertex-sorted one can try the derivation, and on a table of an even
    number of rows it then launches both forms of its rows step, the plain one as leaf_rows_plain; reverse_derived says
    whether the derivation held; gg_csr_export reports -1 for every rowid exactly when the build kept none."""
    src = np.asarray(src, np.int64)
    assert src.size and src.size % 2 == 0, "an odd table never tries the derivation: the proof below needs an even one"
    csr, names = _build(gg, form, vid, src, dst, rowid)
    ctx = gg
    if form == "vertex_sorted":
        assert "leaf_rows_plain" in names, names  # on gg, that is: the witness that these knobs give the sorted form
        if csr.reverse_derived:
            csr.close()
            assert sorted_ctx is not None, "a fully mirrored table: pass the context that never derives"
            ctx = sorted_ctx
            csr, names = _build(ctx, form, vid, src, dst, rowid)
            assert "leaf_rows_plain" not in names and "partition_dual_plain" not in names, names
    try:
        bucketed, multipass = "partition_dual" in names, "densify_hist" in names
        assert bucketed != multipass, names
        assert multipass == (form in KEEPS_ROW), (form, names)
        if bucketed:
            assert "leaf_rows" in names or "leaf_rows_plain" in names, names
        if form in ("leaf_rowid", "mask_ranks", LEAF_BIG):
            assert "leaf_rows_plain" not in names and "sub_totals_plain" not in names, (form, names)
        if form == "derived":
            assert {"leaf_rows", "leaf_rows_plain", "partition_dual_plain"} <= names, names
        assert csr.reverse_derived == (1 if form == "derived" else 0), form
        assert csr.E > 0
        eid = csr.export()[2]
        assert bool(np.all(eid == -1)) == (form not in HAS_ROWID), form
        if form in HAS_ROWID:
            assert not np.any(eid == -1), form
            assert ("gather_rowid" in names) == (rowid is not None), names
    except BaseException:
        csr.close()
        raise
    return ctx, csr


def first_paths_call(ctx, form, fn):
    """fn(), the first gg_bfs64_paths call on a CSR: it rebuilds the entries' sources exactly where the build kept none"""
    out, names = launched(ctx, fn)
    assert ("path_entry_rows" in names) == (form not in KEEPS_ROW), (form, names)
    return out


def refused(ctx, fn):
    with pytest.raises(GGError) as e:
        fn()
    assert e.value.code == GG_ERR_STATE, e.value


# ---- tables ------------------------------------------------------------------------------------------------------------
def _positions(name):
    """(V, src, dst) in position space; the id V is no vertex."""
    shape, variant = name.split("_")
    rng = np.random.default_rng(sum(map(ord, shape)))
    if shape == "a":    # partial tiles; self loops, duplicate rows, ids that are no vertex
        V = 3000
        src, dst = mirrored(np.arange(V, dtype=np.int64), 2 * (2 * TILE + 99), rng, extras=True)
    elif shape == "b":  # many buckets, the direct-store path of k_vrows
        V = 70_000
        src, dst = mirrored(np.arange(V, dtype=np.int64), 600_000, rng, extras=True)
    elif shape == "c":  # the hub is the source of every first-half row
        V = 3000
        leaves = np.delete(np.arange(V, dtype=np.int64), HUB)[:2500]
        d = leaves[rng.integers(0, leaves.size, TILE + 100)]
        s = np.full(d.size, HUB, np.int64)
        src, dst = np.concatenate([s, d]), np.concatenate([d, s])
    else:
        raise AssertionError(name)
    if variant == "plain":  # the same rows shuffled: no row i + E/2 mirrors row i any more
        p = rng.permutation(src.size)
        src, dst = src[p], dst[p]
    else:
        assert variant == "mirrored"
    return V, src, dst


HUB = 17
TABLES = ["a_mirrored", "a_plain", "b_mirrored", "b_plain", "c_mirrored", "c_plain"]


class Table:
    """One table in position space, its oracle CSR and the references of the consumers, each computed on first use."""

    def __init__(self, orc, name):
        self.name = name
        self.V, self.src, self.dst = _positions(name)
        self.pos = np.arange(self.V, dtype=np.int64)
        rc, self.g = orc.csr_build(self.pos, self.src, self.dst)
        assert rc == 0
        self.off, self.nbr, self.eid, o_vid = self.g.arrays()
        assert np.array_equal(o_vid, self.pos)
        keep = (self.src < self.V) & (self.dst < self.V)
        self.ksrc, self.kdst = self.src[keep], self.dst[keep]
        rng = np.random.default_rng(len(name))
        self.sources = rng.choice(self.V, 64, replace=False).astype(np.int64)
        if name[0] == "c":
            self.sources[5] = HUB if HUB not in self.sources else self.sources[5]
        self.targets = self.pos if self.V <= 3000 else np.sort(rng.choice(self.V, 300, replace=False)).astype(np.int64)
        self._memo = {}

    def memo(self, key, fn):
        if key not in self._memo:
            self._memo[key] = fn()
        return self._memo[key]

    def ids(self, kind):
        """(vid, idmap): the vertex ids of a dictionary kind and the map position -> id with idmap[V] no vertex"""
        def make():
            vid = _ids(kind, self.V, np.random.default_rng(self.V + len(kind)))
            bad = np.int64(int(vid.max()) + 1) if int(vid.max()) < np.iinfo(np.int64).max else np.int64(int(vid.min()) - 1)
            return vid, np.append(vid, bad)
        return self.memo(("ids", kind), make)

    def pairs(self):
        return np.repeat(self.sources, self.targets.size), np.tile(self.targets, self.sources.size)

    def bfs(self, max_hops):
        return self.memo(("bfs", max_hops), lambda: self.g.bfs64(self.sources, max_hops))

    def paths(self, max_hops):
        """ref.shortest_paths of every (source, target) pair, with the oracle's distances; vertex column: positions"""
        def make():
            dist = self.bfs(max_hops)[0]
            if max_hops >= 0 and np.array_equal(dist, self.bfs(-1)[0]):
                return self.paths(-1)  # (the relation is a function of the CSR and the distances)
            lane = {int(s): i for i, s in enumerate(self.sources)}
            s, t = self.pairs()
            return ref.shortest_paths(self.off, self.nbr, self.eid, self.pos, s, t, max_hops, True,
                                      dist_of=lambda v: dist[lane[v]])
        return self.memo(("paths", max_hops), make)

    def khop(self, k_min, k_max, **sel):
        key = tuple(sorted((k, np.asarray(v).tobytes()) for k, v in sel.items()))
        return self.memo(("khop", k_min, k_max, key), lambda: self.g.khop(k_min, k_max, **sel))

    def rows2(self):
        return self.memo("rows2", lambda: self.g.khop_rows(2, 2)[2])

    def close(self):
        self.g.close()


@pytest.fixture(scope="module")
def tables(orc):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Table(orc, name)
        return made[name]

    yield get
    for t in made.values():
        t.close()


def cases(shapes, forms=FORMS):
    """form x dictionary kind x table; the derived form takes the mirrored variants only"""
    out = []
    for form in forms:
        for kind in KINDS:
            for shape in shapes:
                for variant in ("mirrored", "plain"):
                    if form == "derived" and variant == "plain":
                        continue
                    out.append(pytest.param(form, kind, f"{shape}_{variant}", id=f"{form}-{kind}-{shape}_{variant}"))
    return out


def build_table(gg, gg_sorted, form, t, kind, rowid=None):
    """the table under the ids of `kind`, built in `form`; the exported arrays are the oracle's"""
    vid, idmap = t.ids(kind)
    ctx, csr = build_form(gg, form, vid, idmap[t.src], idmap[t.dst], rowid, sorted_ctx=gg_sorted)
    try:
        assert (csr.V, csr.E, csr.dropped) == (t.g.V, t.g.E, t.g.dropped)
        off, nbr, eid, v2 = csr.export()
        assert np.array_equal(off, t.off) and np.array_equal(nbr, t.nbr) and np.array_equal(v2, vid)
        if form in HAS_ROWID:
            assert np.array_equal(eid, t.eid if rowid is None else rowid[t.eid])
    except BaseException:
        csr.close()
        raise
    return ctx, csr, vid, idmap


def id_list(t, idmap, n, seed):
    """positions of n vertices, some of them twice, and the id that is no vertex in between; their ids"""
    rng = np.random.default_rng(seed)
    p = rng.choice(t.V, n, replace=False).astype(np.int64)
    p = np.concatenate([p[: n // 2], [t.V], p[: n // 4], p[n // 2:], [t.V]])
    return p, idmap[p]


# ---- 1. shortest paths -------------------------------------------------------------------------------------------------
_path_rows = {}  # (table, kind, max_hops) -> (form that ran first, digest of its pair / step / vertex columns)


def _same(got, want, names=("pair", "step", "vertex", "edge")):
    for name, g, w in zip(names, got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), name


@pytest.mark.parametrize("form,kind,name", cases("abc"))
def test_shortest_paths(gg, gg_sorted, tables, form, kind, name):
    """64 sources x every vertex (a, c) or 300 targets (b), max_hops -1 and 2, row for row against ref.shortest_paths:
    without edges on every form, twice on one CSR (the reverse-by-source copy fresh, then kept); with edges -- append
    positions and explicit rowids -- where the form keeps rowids, refused with GG_ERR_STATE where it keeps none.  The
    pair / step / vertex columns are the same on every form of a table."""
    t = tables(name)
    s_pos, t_pos = t.pairs()
    explicit = np.arange(t.src.size, dtype=np.int64)[::-1] * 3 + 1000
    for rowid in ((None, explicit) if form in HAS_ROWID else (None,)):
        ctx, csr, vid, idmap = build_table(gg, gg_sorted, form, t, kind, rowid)
        try:
            s, d = vid[s_pos], vid[t_pos]
            for n_call, max_hops in enumerate((-1, 2)):
                pair, step, vpos, edge = t.paths(max_hops)
                want = (pair, step, vid[vpos], np.full(edge.size, -1, np.int64))
                call = lambda: ctx.shortest_paths(csr, s, d, max_hops, edges=False)  # noqa: E731
                got = first_paths_call(ctx, form, call) if n_call == 0 else call()
                _same(got, want)
                h = hashlib.sha1(b"".join(np.ascontiguousarray(c).tobytes() for c in got[:3])).hexdigest()
                first = _path_rows.setdefault((name, kind, max_hops), (form, h))
                assert first[1] == h, (first[0], form)
                if form in HAS_ROWID:
                    hop = edge >= 0
                    w_edge = edge if rowid is None else np.where(hop, rowid[np.where(hop, edge, 0)], -1)
                    _same(ctx.shortest_paths(csr, s, d, max_hops, edges=True), want[:3] + (w_edge,))
                else:
                    refused(ctx, lambda: ctx.shortest_paths(csr, s[:100], d[:100], max_hops, edges=True))
                    _same(ctx.shortest_paths(csr, s, d, max_hops, edges=False), want)  # the context is usable
        finally:
            csr.close()


# ---- 2. middle-vertex 2-hop --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,kind,name", cases("ab"))
def test_middle_vertex_two_hop(gg, gg_sorted, tables, form, kind, name):
    """The middle-vertex ranges of khop_partition_mid: their counts and digests add up to the oracle's, and their
    materialised rows are the oracle's 2-hop rows (table b, 5 * 10^6 rows: their number and their digest read where they
    lie)."""
    t = tables(name)
    ctx, csr, vid, idmap = build_table(gg, gg_sorted, form, t, kind)
    try:
        whole, second = t.khop(1, 2), t.khop(2, 2)
        want = sort_rows(vid[t.rows2()]) if name[0] == "a" else None
        for n in (1, 3, 8):
            b = ctx.khop_partition_mid(csr, n)
            assert b[0] == 0 and b[-1] == csr.V and all(x <= y for x, y in zip(b, b[1:]))
            rows, dig, rows22, dig22, got, n_mat, d_mat = [0, 0, 0], [0, 0, 0], 0, 0, [], 0, 0
            for lo, hi in zip(b, b[1:]):
                st = ctx.expand_khop_mid(csr, lo, hi)
                for h in (1, 2):
                    rows[h] += st["rows"][h]
                    dig[h] = dsum(dig[h], st["digest"][h])
                st = ctx.expand_khop_mid(csr, lo, hi, 2, 2)
                rows22, dig22 = rows22 + st["rows"][2], dsum(dig22, st["digest"][2])
                res = ctx.expand_khop_mid_result(csr, lo, hi)
                try:
                    n_part, d_part = res.digest(csr, 2)
                    assert n_part == res.rows(2)
                    n_mat, d_mat = n_mat + n_part, dsum(d_mat, d_part)
                    if want is not None:
                        got.append(read_table(res, 2))
                finally:
                    res.close()
            assert rows[1:] == whole["rows"][1:3] and dig[1:] == [x & 0xFFFFFFFF for x in whole["digest"][1:3]], n
            assert (rows22, dig22) == (second["rows"][2], second["digest"][2] & 0xFFFFFFFF), n
            assert (n_mat, d_mat) == (whole["rows"][2], whole["digest"][2] & 0xFFFFFFFF), n
            if want is not None:
                assert np.array_equal(sort_rows(np.concatenate(got)), want), n
    finally:
        csr.close()


# ---- 3. counting and product kernels -----------------------------------------------------------------------------------
@pytest.mark.parametrize("form,kind,name", cases("ac"))
def test_walk_counts_and_three_hop_expansion(gg, gg_sorted, tables, form, kind, name):
    """khop_count up to 4 hops against exact_walk_counts and expand_khop(1, 3) against the oracle, from every vertex and
    from a source list, with the product kernels and with the frontier kernels only."""
    t = tables(name)
    ctx, csr, vid, idmap = build_table(gg, gg_sorted, form, t, kind)
    try:
        p, listed = id_list(t, idmap, 40, 7)
        if name[0] == "c":
            p[0], listed[0] = HUB, vid[HUB]
        for sources, sel, osel in ((None, None, {}), (listed, p, {"sources_dense": p[p < t.V].astype(np.uint32)})):
            exact = t.memo(("exact", sel is None), lambda: exact_walk_counts(t.pos, t.src, t.dst, 4, sources=sel)[1])
            want = t.khop(1, 3, **osel)
            assert want["rows"][1:4] == exact[1:4]
            for knob in (0, 1):
                ctx.force_frontier(knob)
                assert ctx.khop_count(csr, 1, 4, sources=sources)[1:5] == exact[1:5], knob
                assert ctx.expand_khop(csr, 1, 3, sources=sources) == want, knob
            ctx.force_frontier(0)
    finally:
        csr.close()


# ---- 4. BFS ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,kind,name", cases("a"))
def test_bfs_in_every_output_form(gg, gg_sorted, tables, form, kind, name):
    """gg_bfs64 with a target list, gg_bfs64_pairs, gg_bfs64_pairs_packed and the 1-rank sharded BFS stepped to its end
    on the whole CSR: all the oracle's distances."""
    t = tables(name)
    ctx, csr, vid, idmap = build_table(gg, gg_sorted, form, t, kind)
    try:
        sources = vid[t.sources]
        tp, targets = id_list(t, idmap, 200, 3)
        for max_hops in (-1, 3):
            dist, stats = t.bfs(max_hops)
            got, _ = ctx.bfs64(csr, sources, max_hops, targets=targets)
            assert ctx.bfs64(csr, sources, max_hops, fetch=False)[1] == stats
            assert np.array_equal(got, np.where(tp < t.V, dist[:, np.minimum(tp, t.V - 1)], -1))
            lane, v = np.nonzero(dist >= 0)
            want = sort_rows(np.stack([sources[lane], vid[v], dist[lane, v].astype(np.int64)], axis=1))
            rows, st = ctx.bfs64_pairs(csr, sources, max_hops)
            assert st == stats and np.array_equal(sort_rows(rows), want)
            words = ctx.bfs64_pairs_packed(csr, sources, max_hops)
            w_lane = (words >> np.uint64(58)).astype(np.int64)
            w_dist = ((words >> np.uint64(32)) & np.uint64(0x3FFFFFF)).astype(np.int64)
            w_v = (words & np.uint64(0xFFFFFFFF)).astype(np.int64)
            assert np.array_equal(sort_rows(np.stack([sources[w_lane], vid[w_v], w_dist], axis=1)), want)
            rows, levels = ctx.bfs_sharded_emulated([csr], sources, max_hops)
            assert np.array_equal(sort_rows(rows), want)
            assert levels == int(dist.max())
    finally:
        csr.close()


# ---- 5. seeded closures ------------------------------------------------------------------------------------------------
def _fetch(res):
    try:
        got = res.fetch()
        assert sum(res.rows()) == got[0].size
        return got
    finally:
        res.close()


@pytest.mark.parametrize("form,kind,name", cases("a"))
def test_seeded_endpoints_reach_closure_and_level_sets(gg, gg_sorted, tables, form, kind, name):
    """walk_endpoints, reach_closure (both visited sets) and level_sets (every set and order combination), seeded with
    ids that repeat and ids that are no vertex: the seeds pass through the id table that ensure_ht fills on first use."""
    t = tables(name)
    ctx, csr, vid, idmap = build_table(gg, gg_sorted, form, t, kind)
    try:
        p, seeds = id_list(t, idmap, 12, 5)
        dense = np.unique(p[p < t.V])
        masks = t.memo("endpoints", lambda: endpoint_sets(t.off, t.nbr, dense, 4))
        ids, got = ctx.walk_endpoints(csr, seeds, 4)
        keep = np.flatnonzero(masks)
        assert np.array_equal(ids, vid[keep]) and np.array_equal(got, masks[keep])

        classes = (np.arange(p.size) % 3).astype(np.uint32)
        seen = (np.arange(p.size) % 2).astype(bool)
        e_cls, e_pos, e_lev = t.memo("reach", lambda: exact_reach(t.ksrc, t.kdst, t.pos, p, classes, seen))
        for mode in (1, 2):
            ctx.debug_reach_visited(mode, 0)
            cls, v, lev = _fetch(ctx.reach_closure(csr, seeds, classes, seen))
            assert np.array_equal(lev, e_lev) and np.array_equal(cls, e_cls) and np.array_equal(v, vid[e_pos]), mode
        ctx.debug_reach_visited(0, 0)

        l_cls, l_pos, l_lev = t.memo("levels", lambda: exact_levels(t.ksrc, t.kdst, t.pos, p, classes, 3))
        for combination in COMBINATIONS:
            ctx.debug_level_sets(*combination)
            cls, v, lev = _fetch(ctx.level_sets(csr, seeds, classes, max_levels=3))
            assert np.array_equal(lev, l_lev) and np.array_equal(cls, l_cls) and np.array_equal(v, vid[l_pos]), combination
        ctx.debug_level_sets(0, 0)
    finally:
        ctx.debug_reach_visited(0, 0)
        ctx.debug_level_sets(0, 0)
        csr.close()


_forest = {}


def forest_positions():
    """test_gpu_walk_closure's reply forest (3000 messages, 30 roots, a chain of 60 replies) in position space"""
    if not _forest:
        src, dst, ids = forest(np.random.default_rng(17), 3000, 30, 60)
        order = np.argsort(ids)
        _forest["V"] = ids.size
        _forest["src"] = order[np.searchsorted(ids, src, sorter=order)].astype(np.int64)
        _forest["dst"] = order[np.searchsorted(ids, dst, sorter=order)].astype(np.int64)
        assert _forest["src"].size % 2 == 0
    return _forest["V"], _forest["src"], _forest["dst"]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", KINDS)
def test_walk_closure_on_a_deep_forest(gg, gg_sorted, form, kind):
    """gg_walk_closure over a forest with a chain 60 deep.  Where the form keeps rowids (append positions and explicit
    ones): every row against exact_closure, in order.  Where it keeps none, include/gg.h promises GG_ERR_STATE and a
    usable context: the reachability closure of the same CSR then runs, against exact_reach.  The derived form takes
    the forest with every edge mirrored; unbounded walks over it would meet a cycle, but it is refused before that."""
    V, s, d = forest_positions()
    if form == "derived":
        s, d = np.concatenate([s, d]), np.concatenate([d, s])
    rng = np.random.default_rng(V + len(kind))
    vid = _ids(kind, V, rng)
    bad = np.int64(int(vid.max()) + 1) if int(vid.max()) < np.iinfo(np.int64).max else np.int64(int(vid.min()) - 1)
    src, dst = vid[s], vid[d]
    seeds = np.concatenate([vid[:30], [bad], vid[:5], vid[1000:1010], [bad]])
    explicit = np.arange(src.size, dtype=np.int64)[::-1] * 5 + 77
    for rowid in ((None, explicit) if form in HAS_ROWID else (None,)):
        ctx, csr = build_form(gg, form, vid, src, dst, rowid, sorted_ctx=gg_sorted)
        try:
            if form in HAS_ROWID:
                res = ctx.walk_closure(csr, seeds)
                per_level = res.rows()
                got = _fetch(res)
                want = exact_closure(src, dst, np.arange(src.size, dtype=np.int64) if rowid is None else rowid, seeds)
                for g, w in zip(got, want):
                    assert g.dtype == w.dtype and np.array_equal(g, w)
                assert len(per_level) >= 60 and sum(per_level) == want[0].size
            else:
                refused(ctx, lambda: ctx.walk_closure(csr, seeds))
                refused(ctx, lambda: ctx.walk_closure(csr, seeds, 3))
                classes = np.zeros(seeds.size, np.uint32)
                seen = np.ones(seeds.size, bool)
                e_cls, e_vid, e_lev = exact_reach(src, dst, vid, seeds, classes, seen)
                cls, v, lev = _fetch(ctx.reach_closure(csr, seeds, classes, seen))
                assert np.array_equal(lev, e_lev) and np.array_equal(cls, e_cls) and np.array_equal(v, e_vid)
                assert form == "derived" or int(lev.max()) >= 60
        finally:
            csr.close()


# ---- 6. same-neighbour filter ------------------------------------------------------------------------------------------
_filter = {}


def filter_case():
    """deep_graphs' multigraph and a sensor table over it, in position space (the three sensors after the vertices), and
    the 5-hop rows the filter must give: for every path row and every sensor w, the row (w, v0..v5) comes
    prod_c mult(v_c, w) times -- the restatement of test_gpu_deep_walks.test_same_neighbour_filter_at_depth."""
    if _filter:
        return _filter
    vid, src, dst = deep_graphs.shape("multigraph")
    V = vid.size
    order = np.argsort(vid)

    def position(ids):  # V + 3: no vertex
        at = np.minimum(np.searchsorted(vid, ids, sorter=order), V - 1)
        return np.where(vid[order[at]] == ids, order[at], V + 3).astype(np.int64)

    rng = np.random.default_rng(91)
    m_src, m_dst = [], []
    for v in range(V):
        r = rng.random()
        for w in ([0] if r < 0.75 else [0, 0] if r < 0.85 else [0, 1] if r < 0.93 else [1] if r < 0.97 else []):
            m_src.append(v)
            m_dst.append(V + w)
    if len(m_src) % 2:
        m_src.append(m_src[0])
        m_dst.append(m_dst[0])
    mult = {}
    for a, b in zip(m_src, m_dst):
        mult[(a, b)] = mult.get((a, b), 0) + 1
    _filter.update(V=V, src=position(src), dst=position(dst), m_src=np.array(m_src, np.int64),
                   m_dst=np.array(m_dst, np.int64), mult=mult)
    return _filter


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", KINDS)
def test_same_neighbour_filter_over_a_filter_csr_of_every_form(gg, gg_sorted, orc, form, kind):
    """connected_paths_same_neighbour at 5 hops; the filter CSR (vertex -> sensor rows; for the derived form with their
    mirror, which adds no common neighbour: a sensor's neighbours are vertices, and no vertex neighbours a vertex) is
    built in the form, the path CSR by the default build of the same context."""
    c = filter_case()
    V = c["V"]
    vid = _ids(kind, V + 3, np.random.default_rng(V + len(kind)))
    bad = np.int64(int(vid.max()) + 1) if int(vid.max()) < np.iinfo(np.int64).max else np.int64(int(vid.min()) - 1)
    idmap = np.append(vid, bad)
    if "want" not in c:
        rc, g = orc.csr_build(np.arange(V + 3, dtype=np.int64), c["src"], c["dst"])
        assert rc == 0
        want = []
        for r in g.khop_rows(5, 5)[5].tolist():
            for w in (V, V + 1, V + 2):
                want += [[w] + r] * int(np.prod([c["mult"].get((v, w), 0) for v in r]))
        g.close()
        c["want"] = np.array(want, np.int64).reshape(-1, 7)
        assert 100 < c["want"].shape[0] < 100_000
    m_src, m_dst = c["m_src"], c["m_dst"]
    if form == "derived":
        m_src, m_dst = np.concatenate([m_src, m_dst]), np.concatenate([m_dst, m_src])
    ctx, filter_csr = build_form(gg, form, vid, idmap[m_src], idmap[m_dst], sorted_ctx=gg_sorted)
    path_csr = None
    try:
        assert ctx is gg
        ctx.debug_reset()
        ctx.staging_clear()
        ctx.append_vertices(vid)
        ctx.append_edges(idmap[c["src"]], idmap[c["dst"]])
        path_csr = ctx.build_csr()
        got, names = launched(ctx, lambda: ctx.connected_paths_same_neighbour(path_csr, filter_csr, 5))
        assert np.array_equal(sort_rows(got), sort_rows(vid[c["want"]]))
        assert "filter_fill" in names, names
    finally:
        filter_csr.close()
        if path_csr is not None:
            path_csr.close()


# ---- 7. walks with their edge rowids -----------------------------------------------------------------------------------
@pytest.mark.parametrize("form,kind,name", cases("a"))
def test_two_hop_walks_with_edge_rowids(gg, gg_sorted, tables, form, kind, name):
    """expand_khop_edges at 2 hops where the form keeps rowids (append positions and explicit ones): the rows
    (v0, v1, v2, e1, e2) are exactly the pairs of consecutive entries of the oracle's CSR with its rowids; refused with
    GG_ERR_STATE where the form keeps none."""
    t = tables(name)
    if form not in HAS_ROWID:
        ctx, csr, vid, idmap = build_table(gg, gg_sorted, form, t, kind)
        try:
            refused(ctx, lambda: ctx.expand_khop_edges(csr, 2))
            refused(ctx, lambda: ctx.expand_khop_edges(csr, 2, sources=vid[:3]))
            assert ctx.expand_khop(csr, 1, 2) == t.khop(1, 2)  # the context is usable
        finally:
            csr.close()
        return

    def entry_pairs():  # entry i = (u -> v) followed by every entry j of v's row
        row = np.repeat(t.pos, np.diff(t.off))
        lens = (t.off[1:] - t.off[:-1])[t.nbr]
        i = np.repeat(np.arange(t.nbr.size, dtype=np.int64), lens)
        j = t.off[t.nbr[i]] + np.arange(i.size, dtype=np.int64) - np.repeat(np.cumsum(lens) - lens, lens)
        return row[i], t.nbr[i], t.nbr[j], t.eid[i], t.eid[j]

    v0, v1, v2, e1, e2 = t.memo("entry_pairs", entry_pairs)
    assert v0.size == t.khop(1, 2)["rows"][2]
    assert np.array_equal(sort_rows(np.stack([v0, v1, v2], axis=1)), sort_rows(t.rows2()))
    explicit = np.arange(t.src.size, dtype=np.int64)[::-1] * 3 + 1000
    for rowid in (None, explicit):
        ctx, csr, vid, idmap = build_table(gg, gg_sorted, form, t, kind, rowid)
        try:
            res = ctx.expand_khop_edges(csr, 2)
            try:
                n = res.rows(2)
                assert n == v0.size
                v = read_table(res, 2)
                e = np.concatenate([res.fetch_edges(2, o) for o in range(0, n, 1024)])
            finally:
                res.close()
            m = (lambda x: x) if rowid is None else (lambda x: rowid[x])
            want = np.stack([vid[v0], vid[v1], vid[v2], m(e1), m(e2)], axis=1)
            assert np.array_equal(sort_rows(np.concatenate([v, e], axis=1)), sort_rows(want))
        finally:
            csr.close()


# ---- form 6 ------------------------------------------------------------------------------------------------------------
def test_more_than_2_to_the_20_vertices_without_rowids(gg, orc):
    """V = 2^20 + 1 contiguous ids, 2 * 10^6 mirrored rows, no rowids: the vertex-sorted form is refused and the leaf
    geometry taken, without epos.  Shortest paths of 64 sources x 50 targets, the middle-vertex ranges and khop_count.
    Left out as too slow at this size: the materialised 2-hop rows (their number and digest are read where they lie),
    every vertex as a target, khop_count past 3 hops and exact_walk_counts (Python integers over 10^6 vertices: the
    oracle's khop rows are the reference of the counts here)."""
    V = (1 << 20) + 1
    rng = np.random.default_rng(6)
    pos = np.arange(V, dtype=np.int64)
    vid = (pos + 1000)[rng.permutation(V)]
    s, d = mirrored(pos, 2_000_000, rng, extras=True)
    idmap = np.append(vid, np.int64(999))
    rc, g = orc.csr_build(pos, s, d)
    assert rc == 0
    gg.debug_reset()
    ctx, csr = build_form(gg, LEAF_BIG, vid, idmap[s], idmap[d])
    try:
        off, nbr, eid, o_vid = g.arrays()
        got = csr.export()
        assert np.array_equal(got[0], off) and np.array_equal(got[1], nbr) and np.array_equal(got[3], vid)
        sources = rng.choice(V, 64, replace=False).astype(np.int64)
        targets = nbr[off[sources[0]]:off[sources[0]] + 1].tolist() + rng.choice(V, 49, replace=False).tolist()
        sp, tp = np.repeat(sources, len(targets)), np.tile(np.array(targets, np.int64), 64)
        for max_hops in (-1, 2):
            dist = g.bfs64(sources, max_hops)[0]
            lane = {int(x): i for i, x in enumerate(sources)}
            pair, step, vpos, edge = ref.shortest_paths(off, nbr, eid, pos, sp, tp, max_hops, False,
                                                        dist_of=lambda v: dist[lane[v]])
            call = lambda: ctx.shortest_paths(csr, vid[sp], vid[tp], max_hops, edges=False)  # noqa: E731
            _same(first_paths_call(ctx, LEAF_BIG, call) if max_hops < 0 else call(), (pair, step, vid[vpos], edge))
        refused(ctx, lambda: ctx.shortest_paths(csr, vid[sp[:10]], vid[tp[:10]], -1, edges=True))
        whole = g.khop(1, 3)
        assert ctx.khop_count(csr, 1, 3)[1:4] == whole["rows"][1:4]
        p = np.concatenate([sources, sources[:5], [V]])
        listed = g.khop(1, 3, sources_dense=p[p < V].astype(np.uint32))
        assert ctx.khop_count(csr, 1, 3, sources=idmap[p])[1:4] == listed["rows"][1:4]
        for n in (1, 3, 8):
            b = ctx.khop_partition_mid(csr, n)
            rows, dig, n_mat, d_mat = [0, 0, 0], [0, 0, 0], 0, 0
            for lo, hi in zip(b, b[1:]):
                st = ctx.expand_khop_mid(csr, lo, hi)
                for h in (1, 2):
                    rows[h] += st["rows"][h]
                    dig[h] = dsum(dig[h], st["digest"][h])
                res = ctx.expand_khop_mid_result(csr, lo, hi)
                try:
                    n_part, d_part = res.digest(csr, 2)
                    n_mat, d_mat = n_mat + n_part, dsum(d_mat, d_part)
                finally:
                    res.close()
            assert rows[1:] == whole["rows"][1:3] and dig[1:] == [x & 0xFFFFFFFF for x in whole["digest"][1:3]], n
            assert (n_mat, d_mat) == (whole["rows"][2], whole["digest"][2] & 0xFFFFFFFF), n
    finally:
        csr.close()
        g.close()
