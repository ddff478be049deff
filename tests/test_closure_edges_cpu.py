"""tests/closure_edges.py without a GPU: the model of the closures' shared step against np.repeat on every case, every
case named for a branch shown to take it (from the model's branch output), claim()'s hash slot against constants, the
three exact references against each other on forests — and the inputs of the three older closure test files replayed
through the model, which shows which of them reach locate_entry's global search (the reply forests do)."""
import numpy as np
import pytest

from tests import closure_edges as CE

CASES = CE.all_cases()


def _frontiers(case):
    if not hasattr(case, "_frontiers"):
        case._frontiers = {op: CE.frontiers(case, op) for op in case.ops}
    return case._frontiers


def _model_is_exact(deg, global_search=True):
    got = CE.locate(deg, global_search)
    entry, k = CE.repeat_reference(deg)
    return np.array_equal(got["entry"], entry) and np.array_equal(got["k"], k)


@pytest.mark.parametrize("name", list(CASES))
def test_model_equals_repeat_on_every_frontier(name):
    case = CASES[name]
    expanded = 0
    for op, levels in _frontiers(case).items():
        for L, deg in enumerate(levels):
            assert _model_is_exact(deg), (op, L)
            expanded += int(deg.sum()) > 0
    assert expanded  # every case expands something


def _named_level(case, op):
    return _frontiers(case)[op][case.expect["level"] - 1]


@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("zero_run_")])
def test_zero_runs_take_the_branch_they_are_named_for(name):
    case, e = CASES[name], CASES[name].expect
    for op in case.ops:
        deg = _named_level(case, op)
        m = CE.locate(deg)
        r = int(name.split("_")[2])
        assert (deg[1:1 + r] == 0).all() and deg[0] > 0  # [A, run, ...] in this operator's frontier order
        took_global = m["branch"] == CE.GLOBAL
        assert took_global.any() == e["global"], op
        if e["b_entry"] is not None:
            assert deg.size == r + 2 and deg[e["b_entry"]] == 300
        else:
            assert deg.size == r + 1
        if e["global"]:
            # exactly B's children in tile 0 lie behind the window of A.  The model without the branch gets them wrong
            # from r = 256 on; at r = 255 B is entry i0 + 256, which is also what the window's last offset stands for
            in_b = m["entry"] == e["b_entry"]
            first_tile = np.arange(m["M"]) < CE.XT
            np.testing.assert_array_equal(took_global, in_b & first_tile)
            assert _model_is_exact(deg, global_search=False) == (r == 255)
        else:
            assert _model_is_exact(deg, global_search=False)
        if e["b_starts_tile"] is not None:  # the run and B start on a tile border: the tile's first entry is B
            assert deg[0] == CE.XT and m["tile_entry"][e["b_starts_tile"]] == e["b_entry"]
            assert m["tile_entry"][0] == 0
        if e["b_entry"] is None:  # the run ends the frontier: A's last tile starts in A and its window passes the end
            assert m["tile_entry"].tolist() == [0, 0]
            assert (CE.load_window(np.concatenate([[0], np.cumsum(deg)]).astype(np.uint64), deg.size, 0)[-1]
                    == CE.PAST_THE_END) == (deg.size < CE.XT)


def test_zero_run_threshold_is_255_entries():
    """B behind A and r entries without children is window entry r + 1: with r = 254 the window's last pair of offsets
    is B's, with r = 255 B's start is the window's last offset and the search leaves the window"""
    for r, expect in ((CE.ZERO_RUN_CONTROL, False), (255, True)):
        deg = np.array([10] + [0] * r + [300])
        assert (CE.locate(deg)["branch"] == CE.GLOBAL).any() == expect


def test_tile_border_cases_have_their_totals_and_spans():
    for name, case in CASES.items():
        totals = case.expect.get("totals")
        if totals is None:
            continue
        for op in case.ops:
            got = [int(d.sum()) for d in _frontiers(case)[op][:len(totals)]]
            if name.startswith("wave_") and op == CE.REACH:
                assert got[0] == totals[0]
            else:
                assert got == totals, (name, op)
    for T in CE.TOTALS:  # level 2 of total_T: T parents of degree 1
        for op in CE.ALL_OPS:
            assert (_frontiers(CASES[f"total_{T}"])[op][1] == 1).all()
    for n in (256, 257):
        m = CE.locate(_frontiers(CASES[f"degree_one_{n}"])[CE.WALK][0])
        assert m["tile_entry"].tolist() == [0, 256][:len(m["tile_entry"])] and len(m["tile_entry"]) == (n + 255) // 256
    for L in (1, 2):
        case = CASES[f"long_parent_L{L}"]
        entry, first, end = case.expect["spans"]
        for op in case.ops:
            m = CE.locate(_named_level(case, op))
            at = np.flatnonzero(m["entry"] == entry)
            assert (at[0], at[-1] + 1) == (first, end)
            assert m["tile_entry"].tolist() == [0, 1, 1, 1]  # three tiles start inside the long parent
    m = CE.locate(_frontiers(CASES["hub_773"])[CE.WALK][0])
    assert m["tile_entry"].tolist() == [0, 0, 0, 0] and m["k"][-1] == 3 * CE.XT + 4


@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("wave_")])
def test_wave_patterns_have_their_winners(name):
    """position p of level 1 is seed p's only child: lane p % 64 of wave p / 64.  From the exact reference: which seeds'
    children are new, so which lanes can win."""
    case, e = CASES[name], CASES[name].expect
    n = e["parents"]
    deg = _frontiers(case)[CE.REACH][0]
    assert deg.tolist() == [1] * n
    cls, v, lev = CE.exact_rows(case, CE.REACH)
    level_1 = v[lev == 1]
    assert level_1.size == e["reach_level_1"]
    child = dict(zip(case.src.tolist(), case.dst.tolist()))  # one row per seed
    new = np.array([child[s] in set(level_1.tolist()) for s in case.seeds.tolist()])
    pattern = name.split("_")[2]
    if pattern == "distinct":
        assert new.all() and np.unique(level_1).size == n  # every lane of every wave wins
    elif pattern == "same":
        assert new.all() and level_1.size == 1  # n lanes claim one pair: one wins
    else:
        assert np.flatnonzero(new).tolist() == [e["winner"]]
        assert e["winner"] % 64 == {"first": 0, "32nd": 31, "lane63": 63, "last": (n - 1) % 64}[pattern]
    if n % 64:
        assert n // 64 * 64 + n % 64 == n and n % 64 < 64  # the last wave has lanes past M
    assert (n > CE.XT) == (CE.locate(deg)["tile_entry"].size == 2)


def test_fmix64_and_home_slot_constants():
    # by hand: 0 stays 0 through every xor-shift and multiplication
    assert CE.fmix64(0) == 0 and CE.home_slot(0, 0, 1024) == 0
    # x = 1: x ^= x >> 33 leaves 1; x *= c1 gives c1; and so on, each step written out
    c1, c2, m = 0xFF51AFD7ED558CCD, 0xC4CEB9FE1A85EC53, (1 << 64) - 1
    x = c1
    x ^= x >> 33
    assert x == 0xFF51AFD7ED558CCD ^ 0x7FA8D7EB
    x = (x * c2) & m
    x ^= x >> 33
    assert CE.fmix64(1) == x == 0xB456BCFC34C2CB2C
    # the multiply-high reduction: a power of two takes the top bits, any capacity takes floor(h * cap / 2^64)
    for c, v in ((0, 1), (5, 7), ((1 << 32) - 2, (1 << 32) - 2)):
        h = CE.fmix64((c << 32) | v)
        assert CE.home_slot(c, v, 64) == h >> 58 and CE.home_slot(c, v, 1024) == h >> 54
        assert CE.home_slot(c, v, 3) == h * 3 // (1 << 64) < 3
    assert CE.home_slot(0, 1, 64) == 0xB456BCFC34C2CB2C >> 58 == 45


@pytest.mark.parametrize("name", ["hash_homes_64", "hash_homes_1024"])
def test_hash_home_cases_fill_the_last_slot(name):
    case, e = CASES[name], CASES[name].expect
    cap = e["cap"]
    position = {int(v): i for i, v in enumerate(case.vertices.tolist())}
    cls, v, lev = CE.exact_rows(case, CE.REACH)
    homes = [CE.home_slot(c, position[w], cap) for c, w in zip(cls[lev == 1].tolist(), v[lev == 1].tolist())]
    assert homes.count(cap - 1) >= e["home_last"] and homes.count(cap - 2) >= e["home_before"]
    assert len(set(zip(cls[lev == 1].tolist(), v[lev == 1].tolist()))) == len(homes)  # distinct pairs
    # the growth rule leaves the forced slots alone, and the level sets' hash form has 1024 slots
    visited = int(case.seen.sum())
    for L, deg in enumerate(_frontiers(case)[CE.REACH]):
        M = int(deg.sum())
        assert 2 * (visited + M) <= cap
        visited += int((lev == L + 1).sum())
    assert max(int(d.sum()) for d in _frontiers(case)[CE.LEVELS]) <= 512
    assert case.n_classes > 4 * case.classes.size  # sparse class values: most classes of the class sort are empty


def test_growth_boundary_bounds():
    case = CASES["growth_boundary"]
    cls, v, lev = CE.exact_rows(case, CE.REACH)
    visited, bounds = int(case.seen.sum()), []
    for L, deg in enumerate(_frontiers(case)[CE.REACH]):
        if deg.sum():
            bounds.append(2 * (visited + int(deg.sum())))
        visited += int((lev == L + 1).sum())
    assert bounds == case.expect["bounds"] and bounds[-1] == CE.GROWTH_BOUND
    assert [slots for _, slots in case.reach_forms] == [32, 33, 31]


def test_class_width_cases_use_the_top_classes():
    for n in CE.CLASS_COUNTS:
        case = CASES[f"classes_{n}"]
        assert case.n_classes == n and int(case.classes.max()) == n - 1
        assert n == 1 or int(case.classes.min()) == n - 2
        assert case.expect["bitmap"] == (n <= 65537)
        cls = CE.exact_rows(case, CE.LEVELS)[0]
        assert set(cls.tolist()) == set(case.classes.tolist())
    bits_for = lambda n: max(1, (n - 1).bit_length())  # noqa: E731
    assert bits_for(1 << 31) == 31 and bits_for((1 << 31) + 1) == 32 == bits_for((1 << 32) - 1)


def test_route_switch_threshold_and_levels():
    assert CE.levels_compact_threshold(CE.ROUTE_V, CE.ROUTE_CLASSES) == 34191
    case = CE.route_switch()
    children = [int(d.sum()) for d in CE.frontiers(case, CE.LEVELS)]
    assert children[:3] == case.expect["children"] and children[3:] == [0]
    t = CE.levels_compact_threshold(CE.ROUTE_V, CE.ROUTE_CLASSES)
    assert [m >= t for m in children[:3]] == [False, True, False]
    assert CE.levels_compact_threshold(8, 1) == 0  # a small map is always read off in order


def test_exact_references_agree_on_forests():
    """on a forest whose seeds are distinct roots every (class, vertex) is reached along one walk, at one level: the
    reach closure's rows are the level sets' rows, and the walk closure's end vertices per level are the same vertices"""
    names = [n for n in CASES if n.endswith("_sink") or n.startswith(("total_", "degree_one_", "long_parent_", "hub_"))]
    cases = [CASES[n] for n in names] + [CE.unequal_levels()]
    assert len(cases) > 40
    for case in cases:
        assert np.unique(case.dst).size == case.dst.size and not np.isin(case.seeds, case.dst).any()  # a forest, roots
        walk, reach, levels = (CE.exact_rows(case, op) for op in CE.ALL_OPS)
        for a, b in zip(reach, levels):
            np.testing.assert_array_equal(a, b)
        ends = case.dst[walk[1]]
        assert sorted(zip(walk[2].tolist(), ends.tolist())) == sorted(zip(reach[2].tolist(), reach[1].tolist()))
        root_class = dict(zip(case.seeds.tolist(), case.classes.tolist()))  # a walk's seed gives its end's class
        class_at = dict(zip(zip(reach[2].tolist(), reach[1].tolist()), reach[0].tolist()))
        assert all(root_class[s] == class_at[(L, w)]
                   for s, L, w in zip(case.seeds[walk[0]].tolist(), walk[2].tolist(), ends.tolist()))
    assert [int((CE.exact_rows(cases[-1], CE.WALK)[2] == L).sum()) for L in range(1, 6)] == [3, 7, 2, 5, 1]


# ---- the inputs of the three older test files, replayed through the model ---------------------------------------------
class _Result:
    def __init__(self, cols):
        self.cols = cols

    def levels(self):
        return int(self.cols[2].max()) if self.cols[2].size else 0

    def rows(self, level=None):
        per_level = [int((self.cols[2] == L).sum()) for L in range(1, self.levels() + 1)]
        if level is None:
            return per_level
        return per_level[level - 1] if 1 <= level <= len(per_level) else 0

    def fetch(self):
        return self.cols

    def close(self):
        pass


class _Csr:
    def __init__(self, vertices, src, dst, rowid):
        keep = np.isin(src, vertices) & np.isin(dst, vertices)
        self.vertices, self.src, self.dst, self.rowid, self.V = vertices, src[keep], dst[keep], rowid[keep], vertices.size

    def export(self):
        return None, None, None, self.vertices

    def close(self):
        pass


class RecordingGG:
    """What the older tests need of a GG, answered by the exact references; every frontier an operator would expand is
    kept in `frontiers`.  vertices_from_edges gives the distinct endpoint ids ascending (include/gg.h)."""

    def __init__(self):
        from duckdb_pgq_amd import GGError

        self.error, self.frontiers, self._memo = GGError, [], {}
        self.staging_clear()

    def staging_clear(self):
        self.vertices, self.rows = np.empty(0, np.int64), []

    def append_vertices(self, ids):
        self.vertices = np.concatenate([self.vertices, np.asarray(ids, np.int64)])

    def append_edges(self, src, dst, rowid=None):
        self.rows.append((np.asarray(src, np.int64), np.asarray(dst, np.int64),
                          None if rowid is None else np.asarray(rowid, np.int64)))

    def _table(self):
        src, dst = (np.concatenate([r[i] for r in self.rows]) for i in (0, 1))
        rowid = self.rows[0][2] if len(self.rows) == 1 and self.rows[0][2] is not None else np.arange(src.size)
        return src, dst, rowid

    def vertices_from_edges(self):
        src, dst, _ = self._table()
        self.vertices = np.unique(np.concatenate([src, dst]))

    def build_csr(self):
        return _Csr(self.vertices, *self._table())

    def _run(self, op, csr, seeds, classes, seen, bound):
        seeds = np.asarray(seeds, np.int64)
        classes = np.zeros(seeds.size, np.uint32) if classes is None else np.asarray(classes, np.uint32)
        seen = np.zeros(seeds.size, bool) if seen is None else np.asarray(seen, bool)
        key = (id(csr), op, seeds.tobytes(), classes.tobytes(), seen.tobytes(), bound)
        if key not in self._memo:
            unbounded = bound is None or bound < 0
            case = CE.Case("replay", csr.vertices, csr.src, csr.dst, seeds, classes, seen,
                           bound=csr.V + 1 if unbounded and op != CE.REACH else (-1 if unbounded else bound))
            rows = CE.exact_rows(case, op)
            cyclic = unbounded and op != CE.REACH and rows[2].size and int(rows[2].max()) > csr.V
            if not cyclic:
                self.frontiers += [(op, deg) for deg in CE.frontiers(case, op, rows)]
            self._memo[key] = (csr, rows, cyclic)  # (the CSR is kept: its id is part of the key)
        _, rows, cyclic = self._memo[key]
        if cyclic:
            raise self.error(-6, "a cycle is reachable from a seed")
        return rows

    def walk_closure(self, csr, seeds, max_levels=None):
        seed, position, lev = self._run(CE.WALK, csr, seeds, None, None, max_levels)
        return _Result((seed, csr.rowid[position], lev))

    def reach_closure(self, csr, seeds, classes, seen=None, n_classes=None):
        classes = np.asarray(classes, np.uint32)
        if n_classes is not None and classes.size and int(classes.max()) >= n_classes:
            raise self.error(-1, "class out of range")
        return _Result(self._run(CE.REACH, csr, seeds, classes, seen, None))

    def level_sets(self, csr, seeds, classes, n_classes=None, max_levels=-1):
        classes = np.asarray(classes, np.uint32)
        if n_classes is not None and classes.size and int(classes.max()) >= n_classes:
            raise self.error(-1, "class out of range")
        return _Result(self._run(CE.LEVELS, csr, seeds, classes, None, max_levels))

    def debug_reach_visited(self, mode=0, slots=0):
        if not 0 <= mode <= 2:
            raise self.error(-1, "mode")

    def debug_level_sets(self, set_mode=0, order_mode=0):
        if not (0 <= set_mode <= 2 and 0 <= order_mode <= 2) or (set_mode, order_mode) == (2, 2):
            raise self.error(-1, "mode")


# these three only look at kernel names or at the C entry points' refusals, over graphs of three or four vertices
NOT_REPLAYED = {"test_kernels_are_launched", "test_other_results_refuse_the_level_set_calls"}


def _older_tests():
    from tests import test_gpu_level_sets, test_gpu_reach_closure, test_gpu_walk_closure

    out = []
    for module in (test_gpu_walk_closure, test_gpu_reach_closure, test_gpu_level_sets):
        for name in sorted(vars(module)):
            fn = getattr(module, name)
            if not name.startswith("test_") or not callable(fn) or name in NOT_REPLAYED:
                continue
            marks = [m for m in getattr(fn, "pytestmark", []) if m.name == "parametrize"]
            if marks:
                out += [(f"{module.__name__}.{name}[{value}]", fn, {marks[0].args[0]: value}) for value in marks[0].args[1]]
            else:
                out.append((f"{module.__name__}.{name}", fn, {}))
    return out


def test_which_inputs_reach_the_global_search():
    """Every test of the three older files runs against the exact references (and passes: the recorder computes what
    the device must); the frontiers they expand go through the model.

    What this shows is not what the cases were first built on.  A position leaves its window whenever its tile spans
    more than 256 entries, which takes 256 entries without children anywhere in the tile, not a run of them: the reply
    forests of the older files, where most messages have no reply, reach locate_entry's global search in all three
    operators, and the model with that branch deleted is wrong on them.  So the branch was covered before.  What the
    zero-run cases add is its edge: a run of exactly 254 entries stays in the window, 255 leaves it for the entry the
    window's last offset already names, 256 and more need the search's own answer; a run that starts on a tile border
    is skipped by the partition; a run at the very end leaves nothing to find."""
    reached = {op: 0 for op in CE.ALL_OPS}
    broken_older, replayed, n_frontiers = 0, 0, 0
    for label, fn, kwargs in _older_tests():
        gg = RecordingGG()
        fn(gg, **kwargs)
        replayed += 1
        for op, deg in gg.frontiers:
            if not deg.sum():
                continue
            n_frontiers += 1
            assert _model_is_exact(deg), label
            took = bool((CE.locate(deg)["branch"] == CE.GLOBAL).any())
            reached[op] += took
            exact_without = _model_is_exact(deg, global_search=False)
            assert took or exact_without
            broken_older += not exact_without
    assert replayed >= 35 and n_frontiers > 300
    assert all(n > 0 for n in reached.values()), reached
    assert broken_older > 0
    broken = [n for n, c in CASES.items() if c.expect.get("global")
              and all(not _model_is_exact(_named_level(c, op), global_search=False) for op in c.ops)]
    assert len(broken) == 3 * 3  # r = 256, 257, 600 behind a tile's first entry, three builds each
