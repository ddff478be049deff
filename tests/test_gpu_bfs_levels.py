"""The 64-lane BFS (csrc/gg_bfs.hip) per level, direction and distance-cell width.

Every other BFS test compares final distances and four totals.  Here each search is compared with the level-by-level
reference (tests/bfs_levels_ref.py) on graphs that steer every level's direction by construction (tests/bfs_shapes.py):
the distances, the four totals, and gg_debug_bfs_steps -- the per-level n_active / te / reached the kernels counted and
`cur`, the buffer each level left its frontier in, which a pull flips and a push keeps: the device's own record of the
direction every level took.  That record must equal the sequence the shape was built for, so a pull or push body that is
never reached, or a moved threshold, fails here.  All comparisons are exact (integers)."""
import numpy as np
import pytest

from duckdb_pgq_amd import GGError
from tests import all_shortest_paths_ref as all_ref
from tests import bfs_shapes as shapes
from tests import shortest_path_ref as path_ref
from tests.bfs_levels_ref import PULL, PUSH, bfs_levels
from tests.test_gpu_build_forms import FORMS, _gg_sorted_module, build_form, gg_sorted  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

GG_ERR_TOO_LARGE = -5
_refs = {}


def build(gg, s):
    gg.staging_clear()
    gg.append_vertices(s.vid)
    gg.append_edges(s.src, s.dst)
    return gg.build_csr()


def reference(gg, s, sources, max_hops):
    factor = gg.debug_bfs_steps()["pull_factor"]  # the compiled threshold, not a copy of it
    key = (s.name, np.asarray(sources, np.int64).tobytes(), max_hops, factor)
    if key not in _refs:
        _refs[key] = bfs_levels(s.V, s.src, s.dst, sources, max_hops, factor)
    return _refs[key]


def directions_of(steps):
    """what the device recorded: level l pulled iff it flipped cur"""
    cur = steps[:, 3].astype(np.int64)
    assert set(cur.tolist()) <= {0, 1}
    return [PULL if a != b else PUSH for a, b in zip(cur[:-1], cur[1:])]


def check(gg, csr, s, sources=None, max_hops=-1, built_for=None, seen=None):
    """one gg_bfs64 against the reference; returns (the reference, the readout)"""
    sources = s.sources if sources is None else np.asarray(sources, np.int64)
    r = reference(gg, s, sources, max_hops)
    dist, st = gg.bfs64(csr, sources, max_hops)
    rd = gg.debug_bfs_steps()
    assert csr.V == s.V and csr.E == r.E
    assert np.array_equal(dist, r.dist), np.argwhere(dist != r.dist)[:8].tolist()
    assert st == r.totals
    assert rd["levels"] == r.levels
    assert rd["steps"].tolist() == r.steps.tolist()  # n_active, te, reached and cur of every entry, the seed included
    took = directions_of(rd["steps"])
    assert took == r.directions
    if built_for is not None:
        assert took == built_for[:r.levels], (s.name, max_hops)
    if seen is not None:
        seen.update((rd["cell_bytes"], d, l + 1) for l, d in enumerate(took))
    return r, rd


# ---- every shape, unbounded -------------------------------------------------------------------------------------------------
SHAPES = sorted(n for n in shapes.BUILDERS if n != "deep_all_lanes" and not n.startswith("long_chain_"))  # (own tests below)


@pytest.mark.parametrize("name", SHAPES)
def test_shape_runs_the_directions_it_was_built_for(gg, name):
    s = shapes.shape(name)
    csr = build(gg, s)
    try:
        if name.startswith("pull_rows_") and not s.symmetric:
            roff, rnbr, _ = csr.export_reverse()
            if name == "pull_rows_a":  # sources chosen from the library's own row order: the last entry of every row
                s = shapes.pull_rows("a", reverse=(roff, rnbr))
                srcs = set(s.sources.tolist())
                for t in range(2, 2 + len(shapes.IN_DEGREES)):
                    row = rnbr[roff[t]:roff[t + 1]].tolist()
                    assert not row or (row[-1] in srcs and not set(row[:-1]) & srcs), t
            elif name == "pull_rows_b":  # X leads every row
                for t in range(2, 2 + len(shapes.IN_DEGREES)):
                    assert roff[t] == roff[t + 1] or rnbr[roff[t]] == 1, t
            else:  # position p of every row is the source of lane p mod 64
                for t in range(64, s.V):
                    n = int(roff[t + 1] - roff[t])
                    assert rnbr[roff[t]:roff[t + 1]].tolist() == [p % 64 for p in range(n)], t
        r, rd = check(gg, csr, s, built_for=s.directions)
        assert r.levels == len(s.directions) and rd["cell_bytes"] == (2 if r.levels > 254 else 1)
        if name == "pull_rows_c":  # an 8-entry row: exactly 8 bits; 64 entries and more: all 64
            dist, _ = gg.bfs64(csr, s.sources, -1)
            indeg = np.bincount(s.dst, minlength=s.V)
            for t in range(64, s.V):
                assert np.flatnonzero(dist[:, t] == 1).tolist() == list(range(min(int(indeg[t]), 64))), t
    finally:
        csr.close()


# ---- level counts around the read-back chunk ----------------------------------------------------------------------------------
CHUNKED = [f"chain_{e}" for e in shapes.ECCENTRICITIES] + [f"layered_{e}" for e in shapes.ECCENTRICITIES] + [
    "late_pull_6", "late_pull_7"]


@pytest.mark.parametrize("name", CHUNKED)
def test_searches_that_end_at_before_and_after_a_chunk_of_levels(gg, name):
    """the host reads the levels' records back every 6 levels: searches that end, or are cut by max_hops, one before, at
    and one after that boundary, with a frontier left or not"""
    s = shapes.shape(name)
    csr = build(gg, s)
    try:
        for max_hops in shapes.HOP_BOUNDS:
            r, _ = check(gg, csr, s, max_hops=max_hops, built_for=s.directions)
            assert r.levels == (len(s.directions) if max_hops < 0 else min(max_hops, len(s.directions)))
    finally:
        csr.close()


# ---- targets, seeds -----------------------------------------------------------------------------------------------------------
def test_target_list_with_a_repeat_the_last_vertex_and_a_stranger(gg):
    s = shapes.shape("transitions_push")
    csr = build(gg, s)
    try:
        r = reference(gg, s, s.sources, -1)
        targets = np.array([70, s.V - 1, 70, s.V + 3, 0, -1, s.V - 1], np.int64)
        dist, st = gg.bfs64(csr, s.sources, -1, targets=targets)
        want = np.stack([r.dist[:, t] if 0 <= t < s.V else np.full(64, -1, np.int32) for t in targets], axis=1)
        assert np.array_equal(dist, want) and st == r.totals
        assert gg.debug_bfs_steps()["steps"].tolist() == r.steps.tolist()
    finally:
        csr.close()


@pytest.mark.parametrize("name", ["transitions_push", "late_pull_6", "star_pull_V65"])
def test_seed_patterns(gg, name):
    """64 lanes on one vertex, lanes alternating between two vertices, strangers in lanes 0 and 63, 1 / 2 / 63 / 64 lanes"""
    s = shapes.shape(name)
    a, b = int(s.sources[0]), int(s.sources[-1])
    stranger = s.sources.copy() if s.sources.size == 64 else np.resize(s.sources, 64)
    stranger[0], stranger[63] = s.V + 7, -3
    patterns = [np.full(64, a), np.array([a, b] * 32), stranger, np.array([b]), np.array([b, a]),
                np.resize(s.sources, 63), np.resize(s.sources, 64)]
    csr = build(gg, s)
    try:
        for sources in patterns:
            check(gg, csr, s, sources=sources)
    finally:
        csr.close()


# ---- build forms --------------------------------------------------------------------------------------------------------------
PLAIN_FORMS = [f for f in FORMS if f != "derived"]


@pytest.mark.parametrize("form,name", [(f, n) for n in ("pull_rows_c", "transitions_push", "star_push_V65", "late_pull_6")
                                       for f in PLAIN_FORMS] +
                         [(f, n) for n in ("pull_rows_c_mirrored", "funnel_mirrored") for f in FORMS])
def test_every_build_form(gg, gg_sorted, form, name):
    """the same levels on every route gg_csr_build takes; on the derived form the first pull level reads reverse rows that
    were written (rotated) on first use"""
    s = shapes.shape(name)
    ctx, csr = build_form(gg, form, s.vid, s.src, s.dst, sorted_ctx=gg_sorted)
    try:
        if form == "derived":
            assert not csr.reverse_rows_ready
        check(ctx, csr, s, built_for=s.directions)
        assert csr.reverse_rows_ready
        check(ctx, csr, s, built_for=s.directions)
    finally:
        csr.close()
        ctx.staging_clear()


# ---- repeatability --------------------------------------------------------------------------------------------------------------
def test_two_shapes_of_one_size_take_turns_on_one_context(gg):
    """a push-only search, then a pull search over as many vertices, twice: the pool hands the second the first's blocks,
    and a word or cell left behind would show"""
    a = shapes.shape("star_push_V65")
    b = shapes.star_pull(a.V)
    assert b.V == a.V
    ca, cb = build(gg, a), build(gg, b)
    try:
        for _ in range(2):
            check(gg, ca, a, built_for=[PUSH, PUSH])
            check(gg, cb, b, built_for=[PULL, PUSH])
    finally:
        ca.close()
        cb.close()


# ---- two-byte cells ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def deep():
    return shapes.shape("deep_all_lanes")


def test_two_byte_cells_in_all_64_lanes_with_pull_levels_past_254(gg, deep):
    s = deep
    csr = build(gg, s)
    try:
        r, rd = check(gg, csr, s, built_for=s.directions)
        assert rd["cell_bytes"] == 2 and r.levels == 333
        assert directions_of(rd["steps"])[267:332] == [PULL] * 65  # levels 268 .. 332
        assert np.all(r.dist.max(axis=1) > 255)  # every lane, hence every 8-byte word of a vertex's 64 cells
        want = {(int(s.sources[l]), int(v), int(r.dist[l, v])) for l, v in zip(*np.nonzero(r.dist >= 0))}
        pairs, st = gg.bfs64_pairs(csr, s.sources, -1)
        assert st == r.totals and pairs.shape[0] == len(want)
        assert {tuple(row) for row in pairs.tolist()} == want
        packed = gg.bfs64_pairs_packed(csr, s.sources, -1)
        assert packed.size == len(want)
        lane, d, v = packed >> np.uint64(58), (packed >> np.uint64(32)) & np.uint64(0x3FFFFFF), packed & np.uint64(0xFFFFFFFF)
        assert {(int(s.sources[a]), int(c), int(b)) for a, b, c in zip(lane, d, v)} == want
        assert int(d.max()) == 332 and int(d[lane == 63].max()) == 269 and int((d > 255).sum()) > 64 * 64
        assert gg.debug_bfs_steps()["cell_bytes"] == 2
        # bounded inside the one-byte range: the same graph answers with one-byte cells
        r8, rd8 = check(gg, csr, s, max_hops=254, built_for=s.directions)
        assert rd8["cell_bytes"] == 1 and r8.levels == 254
        r16, rd16 = check(gg, csr, s, max_hops=300, built_for=s.directions)
        assert rd16["cell_bytes"] == 2 and r16.levels == 300
    finally:
        csr.close()


PATH_LANES = [0, 1, 7, 8, 15, 16, 31, 32, 62, 63]


def _deep_pairs(s):
    """per lane: the lane's own source, chain vertices below and beyond distance 255, the chain's end, one vertex of each layer"""
    dsts = [None, 100, 300, 329, 330, 362 + 5, 394 + 31]
    lane, dst = [], []
    for l in PATH_LANES:
        for t in dsts:
            lane.append(l)
            dst.append(l if t is None else t)
        lane.append(l)
        dst.append(0 if l else s.V + 9)  # unreachable (behind the source) / no vertex
    return np.array(lane, np.uint32), np.array(dst, np.int64)


@pytest.mark.parametrize("edges", [True, False])
def test_paths_off_two_byte_cells(gg, deep, edges):
    s = deep
    gg.set_edge_rowid(True)
    csr = build(gg, s)
    try:
        off, nbr, eid, vid = csr.export()
        lane, dst = _deep_pairs(s)
        r = reference(gg, s, s.sources, -1)
        assert {int(r.dist[l, t]) > 255 for l, t in zip(lane, dst) if 0 <= t < s.V} == {True, False}
        want = path_ref.shortest_paths(off, nbr, eid, vid, s.sources[lane], dst, -1, edges)
        got, st = gg.bfs64_paths(csr, s.sources, lane, dst, -1, edges)
        for name, g, w in zip(("pair", "step", "vertex", "edge"), got, want):
            assert g.dtype == w.dtype and np.array_equal(g, w), name
        assert st == r.totals and int(got[1].max()) == 332
        assert gg.debug_bfs_steps()["cell_bytes"] == 2
    finally:
        csr.close()


@pytest.mark.parametrize("edges", [True, False])
def test_all_paths_off_two_byte_cells(gg, deep, edges):
    s = deep
    gg.set_edge_rowid(True)
    csr = build(gg, s)
    try:
        off, nbr, eid, vid = csr.export()
        lane, dst = _deep_pairs(s)
        batch = all_ref.make_batch(off, nbr, vid, s.sources)
        # the last layer is reached by 32 * 32 paths of 270 steps and more: keep three of each pair
        want0, want1, want_st = all_ref.batch_tables(off, nbr, eid, vid, s.sources, lane, dst, -1, 3, edges, True, batch=batch)
        got0, got1, st = gg.bfs64_all_paths(csr, s.sources, lane, dst, -1, 3, edges, True)
        for g, w in zip(got0 + got1, want0 + want1):
            assert g.dtype == w.dtype and np.array_equal(g, w)
        bfs = st.pop("bfs")
        assert st == want_st and bfs == reference(gg, s, s.sources, -1).totals
        assert int(got0[1].max()) == 332 and int(got0[2].max()) == 1024
        assert gg.debug_bfs_steps()["cell_bytes"] == 2
        if not edges:
            src_ids = s.sources[lane]
            got = gg.shortest_path_counts(csr, src_ids, dst)
            want = all_ref.shortest_path_counts(off, nbr, vid, src_ids, dst)
            for g, w in zip(got, want):
                assert g.dtype == w.dtype and np.array_equal(g, w)
    finally:
        csr.close()


def test_the_one_byte_boundary(gg):
    """eccentricity 253: 254 levels, the last finds nothing, one-byte cells.  255: rerun with two-byte cells.  At exactly 254
    the 254th level reaches the last vertex, whose empty row leaves a frontier at the deepest level a byte records: the
    code may rerun (it does, needlessly) or not, so only the answer is asserted."""
    for n, cell in ((254, 1), (255, None), (256, 2)):
        s = shapes.shape(f"long_chain_{n}")
        csr = build(gg, s)
        try:
            if cell is None:
                r = reference(gg, s, s.sources, -1)
                dist, st = gg.bfs64(csr, s.sources, -1)
                assert np.array_equal(dist, r.dist) and st == r.totals and int(dist.max()) == 254
            else:
                r, rd = check(gg, csr, s, built_for=s.directions)
                assert rd["cell_bytes"] == cell and int(r.dist.max()) == n - 1
        finally:
            csr.close()


# ---- the 16-bit limit -----------------------------------------------------------------------------------------------------------
def _chain_steps(n_vertices, lanes, levels):
    """the readout of a chain from its head in closed form (tests/test_bfs_levels_ref_cpu.py holds it to the reference)"""
    steps = np.zeros((levels + 1, 4), np.uint64)
    m = min(levels + 1, n_vertices)
    steps[:m, 0], steps[:m, 2] = 1, lanes
    steps[:min(m, n_vertices - 1), 1] = 1
    return steps


@pytest.mark.parametrize("n_vertices,max_hops", [(65_535, -1), (65_537, 65_534), (65_537, -1)])
def test_the_deepest_search_two_byte_cells_record(gg, n_vertices, max_hops):
    """65 534 is the last distance a two-byte cell holds: a chain that ends there is answered, a longer one is answered
    when the caller bounds the search there and refused when it does not -- and the context works on"""
    s = shapes.long_chain(n_vertices, lanes=2)
    csr = build(gg, s)
    try:
        if n_vertices == 65_537 and max_hops < 0:
            with pytest.raises(GGError) as e:
                gg.bfs64(csr, s.sources, -1)
            assert e.value.code == GG_ERR_TOO_LARGE and "deeper than 65534 levels" in str(e.value)
            small = shapes.shape("late_pull_6")
            c2 = build(gg, small)
            try:
                check(gg, c2, small, built_for=small.directions)
            finally:
                c2.close()
            return
        dist, st = gg.bfs64(csr, s.sources, max_hops)
        want = np.arange(n_vertices, dtype=np.int32)
        want[65_535:] = -1
        assert np.array_equal(dist, np.stack([want, want]))
        assert st == {"levels": 65_534, "traversed_edges": 65_534, "active_vertices": 65_534,
                      "reached_pairs": 2 * 65_535}
        rd = gg.debug_bfs_steps()
        assert rd["cell_bytes"] == 2 and rd["levels"] == 65_534
        assert np.array_equal(rd["steps"], _chain_steps(n_vertices, 2, 65_534))
    finally:
        csr.close()


# ---- the readout itself -----------------------------------------------------------------------------------------------------------
def test_both_directions_ran_with_both_cell_widths_and_a_pull_as_level_one(gg, deep):
    seen = set()
    for s in (shapes.shape("transitions_pull"), shapes.shape("transitions_push"), deep):
        csr = build(gg, s)
        try:
            check(gg, csr, s, built_for=s.directions, seen=seen)
        finally:
            csr.close()
    for cell in (1, 2):
        for d in (PUSH, PULL):
            assert any(c == cell and m == d for c, m, _ in seen), (cell, d)
    assert (1, PULL, 1) in seen


def test_readout_is_empty_before_a_search_and_after_a_reset(gg):
    gg.debug_reset()
    rd = gg.debug_bfs_steps()
    assert rd["steps"].shape == (0, 4) and rd["levels"] == -1 and rd["cell_bytes"] == 0 and rd["pull_factor"] == shapes.FACTOR
    s = shapes.shape("chain_5")
    csr = build(gg, s)
    try:
        gg.bfs64(csr, s.sources, 0)
        rd = gg.debug_bfs_steps()
        assert rd["steps"].tolist() == [[1, 1, 3, 0]] and rd["levels"] == 0 and rd["cell_bytes"] == 1
        gg.bfs64(csr, [], -1)  # no sources: no level, no entry
        assert gg.debug_bfs_steps()["steps"].shape == (0, 4)
        gg.bfs64(csr, s.sources, -1, fetch=False)
        assert gg.debug_bfs_steps()["levels"] == 6
        gg.debug_reset()
        assert gg.debug_bfs_steps()["steps"].shape == (0, 4) and gg.debug_bfs_steps()["cell_bytes"] == 0
    finally:
        csr.close()
