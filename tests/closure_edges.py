"""The numpy / Python-int model of the step the three closure operators share (gg_internal.h: load_window and
locate_entry; gg_khop.hip: k_tile_partition; claim's hash slot), and the inputs built to reach its edges.

A level's frontier has n entries; entry i owns the child positions [foff[i], foff[i + 1]) of the exclusive prefix foff of
the entries' out-degrees.  A workgroup takes the tile of XT = 256 consecutive positions [256 t, 256 t + 256):
  k_tile_partition   i0 = the LAST entry with foff[i0] <= 256 t (entries without children that start there are skipped)
  load_window        the 257 offsets foff[i0 .. i0 + 256], 2^64 - 1 where i0 + j > n ("past the end")
  locate_entry       a binary search for the first window offset above p; if all 257 are <= p (the window is used up by
                     entries without children) the search goes on in global memory over foff[i0 + 256 .. n)
locate() restates the three with the kernels' own shapes and says, for every child position, the entry, the position
inside the entry and the branch (WINDOW or GLOBAL) that found it.  global_search=False is the model with the second
branch deleted: what a kernel without it would compute.

fmix64 / home_slot restate claim()'s slot, __umul64hi(fmix64(class << 32 | vertex index), cap), so that a case can choose
its keys by their home slot.

The case builders return Case objects: an edge table, the vertex table in the dense order the case needs (staged with
append_vertices: the dense index of a vertex is its position there, which the GPU tests assert from csr.export()[3]),
seeds, classes, seen flags and a bound.  Level 1's frontier is the seed list in its order (a seed that is no vertex has
degree 0); in the walk closure level 2's frontier is level 1's rows (parent order, then the append order inside a row); in
reach and level sets it is level 1's rows ascending by (class, dense index).  frontiers() gives the out-degrees of every
level's frontier in that order, from the exact references of the three operators' own test files.

Used by tests/test_closure_edges_cpu.py (the model against np.repeat; every case named for a branch takes it) and by
tests/test_gpu_closure_edges.py (the device against the exact references on every case)."""
from dataclasses import dataclass, field

import numpy as np

XT = 256
PAST_THE_END = (1 << 64) - 1
WINDOW, GLOBAL = 0, 1
M64 = (1 << 64) - 1


# ---- the shared step -------------------------------------------------------------------------------------------------
def tile_entries(foff, n, n_tiles):
    """k_tile_partition: per tile the last entry in [0, n) whose offset is <= 256 t (foff[0] == 0)"""
    out = np.empty(n_tiles, np.int64)
    for t in range(n_tiles):
        target = int(foff[0]) + t * XT
        lo, hi = 0, n  # first idx in [0, n] with foff[idx] > target
        while lo < hi:
            mid = (lo + hi) >> 1
            if int(foff[mid]) <= target:
                lo = mid + 1
            else:
                hi = mid
        out[t] = lo - 1
    return out


def load_window(foff, n, i0):
    """the 257 offsets a workgroup holds: foff[i0 + t] for i0 + t <= n, else 2^64 - 1"""
    gi = i0 + np.arange(XT + 1, dtype=np.int64)
    inside = gi <= n
    return np.where(inside, foff[np.where(inside, gi, 0)], np.uint64(PAST_THE_END)).astype(np.uint64)


def locate(deg, global_search=True):
    """Every child position of a frontier with out-degrees `deg` through the tile partition, the window and
    locate_entry.  Returns a dict: entry, k (position inside the entry), branch (WINDOW / GLOBAL) per position;
    tile_entry per tile; M."""
    deg = np.asarray(deg, np.int64)
    n = deg.size
    foff = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint64)
    M = int(foff[-1])
    n_tiles = (M + XT - 1) // XT
    te = tile_entries(foff, n, n_tiles)
    entry, k, branch = (np.empty(M, np.int64) for _ in range(3))
    for t in range(n_tiles):
        i0 = int(te[t])
        s_foff = load_window(foff, n, i0)
        p = np.arange(t * XT, min(M, (t + 1) * XT), dtype=np.uint64)
        lo = np.zeros(p.size, np.int64)
        hi = np.full(p.size, XT + 1, np.int64)  # first idx in [0, XT + 1) with s_foff[idx] > p
        while (lo < hi).any():
            live = lo < hi
            mid = (lo + hi) >> 1
            le = s_foff[np.minimum(mid, XT)] <= p
            lo = np.where(live & le, mid + 1, lo)
            hi = np.where(live & ~le, mid, hi)
        assert (lo >= 1).all()  # s_foff[0] = foff[i0] <= 256 t <= p
        idx = i0 + lo - 1
        start = s_foff[lo - 1]
        br = np.full(p.size, WINDOW, np.int64)
        if global_search:
            for j in np.flatnonzero(lo == XT + 1):  # window exhausted by zero-degree entries
                glo, ghi = i0 + XT, n
                while glo < ghi:
                    mid = (glo + ghi) >> 1
                    if foff[mid] <= p[j]:
                        glo = mid + 1
                    else:
                        ghi = mid
                idx[j] = glo - 1
                start[j] = foff[glo - 1]
                br[j] = GLOBAL
        sl = slice(t * XT, t * XT + p.size)
        entry[sl], k[sl], branch[sl] = idx, (p - start).astype(np.int64), br
    return {"entry": entry, "k": k, "branch": branch, "tile_entry": te, "M": M}


def repeat_reference(deg):
    """(entry, k) of every child position, by np.repeat"""
    deg = np.asarray(deg, np.int64)
    entry = np.repeat(np.arange(deg.size, dtype=np.int64), deg)
    k = np.arange(entry.size, dtype=np.int64) - np.repeat(np.cumsum(deg) - deg, deg)
    return entry, k


# ---- claim()'s slot --------------------------------------------------------------------------------------------------
def fmix64(x):
    x &= M64
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) & M64
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) & M64
    x ^= x >> 33
    return x


def home_slot(cls, vertex_index, cap):
    """the first slot claim() probes for (class, dense vertex index) in a table of `cap` slots"""
    return (fmix64((int(cls) << 32) | int(vertex_index)) * int(cap)) >> 64


# ---- cases -------------------------------------------------------------------------------------------------------------
WALK, REACH, LEVELS = "walk", "reach", "levels"
ALL_OPS = (WALK, REACH, LEVELS)
REACH_FORMS = ((1, 0), (2, 0))  # (visited mode, first hash slots): bitmap, hash set


@dataclass
class Case:
    name: str
    vertices: np.ndarray        # the vertex table; position = dense index
    src: np.ndarray
    dst: np.ndarray
    seeds: np.ndarray
    classes: np.ndarray
    seen: np.ndarray
    bound: int = -1             # max_levels of the walk closure and the level sets (< 0: none; reach takes none)
    ops: tuple = ALL_OPS
    n_classes: int = None       # None: max(classes) + 1
    reach_forms: tuple = REACH_FORMS
    levels_forms: tuple = None  # None: test_gpu_level_sets.COMBINATIONS
    expect: dict = field(default_factory=dict)  # what the CPU test asserts of the model on it
    staged: tuple = None        # (src, dst, positions): the table to stage where it has rows that are dropped; src / dst
    #                             above are then its rows at `positions`, which are their rowids

    def __post_init__(self):
        self.vertices, self.src, self.dst, self.seeds = (np.asarray(a, np.int64) for a in
                                                         (self.vertices, self.src, self.dst, self.seeds))
        self.classes = np.asarray(self.classes, np.uint32)
        self.seen = np.asarray(self.seen, bool)
        assert self.src.size == self.dst.size and self.seeds.size == self.classes.size == self.seen.size
        assert np.unique(self.vertices).size == self.vertices.size
        assert np.isin(self.src, self.vertices).all() and np.isin(self.dst, self.vertices).all()  # no row is dropped
        if self.n_classes is None:
            self.n_classes = int(self.classes.max()) + 1 if self.classes.size else 0


def vid(i):
    """the id of the vertex staged at position i (ascending, so the id order is the dense order as well)"""
    return 1000 + 3 * np.asarray(i, np.int64)


def no_vertex(j):
    return -7 - 2 * np.asarray(j, np.int64)


class _Graph:
    """vertices numbered in the order they are asked for; rows in the order they are added"""

    def __init__(self):
        self.n, self.src, self.dst = 0, [], []

    def new(self, count=None):
        first = self.n
        self.n += 1 if count is None else count
        return first if count is None else list(range(first, first + count))

    def edge(self, a, b):
        self.src.append(a), self.dst.append(b)

    def fan(self, a, count):
        """`count` new sink vertices under a"""
        kids = self.new(count)
        for w in kids:
            self.edge(a, w)
        return kids

    def case(self, name, seeds, classes=None, seen=None, **kw):
        seeds = np.asarray(seeds, np.int64)  # ids, not positions
        classes = np.zeros(seeds.size, np.uint32) if classes is None else classes
        seen = np.ones(seeds.size, bool) if seen is None else seen
        return Case(name, vid(np.arange(self.n)), vid(self.src), vid(self.dst), seeds, classes, seen, **kw)


ZERO_RUNS = (255, 256, 257, 600)
ZERO_RUN_CONTROL = 254  # one entry short: the window still holds B's offset pair


def zero_run(r, place, level, zeros="sink"):
    """A frontier [A, r entries without children, B] at `level`.
    place "first":  A (10 children) is tile 0's first entry, so B's children in tile 0 lie behind the whole window
          "border": A has exactly 256 children: the run and B start on the border of tile 1, whose first entry must be B
          "end":    the run ends the frontier (no B): the window of A's last tile runs past the end
    Level 1: the seeds are [A, run, B], the run non-vertex ids or sink vertices.  Level 2: one seed, a hub whose row is
    [A, sinks ..., B] in append order and in dense order."""
    assert place in ("first", "border", "end") and level in (1, 2) and (level == 1 or zeros == "sink")
    g = _Graph()
    hub = g.new() if level == 2 else None
    a = g.new()
    run = g.new(r) if zeros == "sink" else []
    b = g.new() if place != "end" else None
    members = [a] + run + ([b] if b is not None else [])
    if level == 2:
        for m in members:
            g.edge(hub, m)
    g.fan(a, {"first": 10, "border": 256, "end": 300}[place])
    if b is not None:
        g.fan(b, 300)
    if level == 2:
        seeds = vid([hub])
    elif zeros == "sink":
        seeds = vid(members)
    else:
        seeds = np.concatenate([vid([a]), no_vertex(np.arange(r)), vid([b]) if b is not None else np.empty(0, np.int64)])
    expect = {"level": level, "global": place == "first" and r >= 255, "b_entry": r + 1 if b is not None else None,
              "b_starts_tile": 1 if place == "border" else None}
    return g.case(f"zero_run_{r}_{place}_L{level}_{zeros}", seeds, expect=expect)


def zero_run_cases():
    out = []
    for r in ZERO_RUNS + (ZERO_RUN_CONTROL,):
        for place in ("first", "border", "end"):
            out.append(zero_run(r, place, 1, "novertex"))
            out.append(zero_run(r, place, 1, "sink"))
            out.append(zero_run(r, place, 2, "sink"))
    return out


TOTALS = (1, 255, 256, 257, 511, 512, 513)


def total_children(T):
    """Level 1: three parents, the middle one a sink, T children together.  Every child has one child of its own, so
    level 2 is T parents of degree 1 and level 3 T sinks."""
    g = _Graph()
    p, q, s = g.new(), g.new(), g.new()
    kids = g.fan(p, T // 3) + g.fan(s, T - T // 3)
    for w in kids:
        g.fan(w, 1)
    return g.case(f"total_{T}", vid([p, q, s]), classes=[0, 1, 1], expect={"totals": [T, T]})


def degree_one_parents(n):
    """n seeds with one child each: a tile of exactly 256 degree-1 parents, or of 257"""
    g = _Graph()
    parents = g.new(n)
    for p in parents:
        g.fan(p, 1)
    return g.case(f"degree_one_{n}", vid(parents), expect={"totals": [n]})


def long_parent(level):
    """a parent of 600 children that starts at position 200 of a tile: it ends in the fourth tile"""
    g = _Graph()
    hub = g.new() if level == 2 else None
    p, q, s = g.new(), g.new(), g.new()
    if level == 2:
        for m in (p, q, s):
            g.edge(hub, m)
    g.fan(p, 200), g.fan(q, 600), g.fan(s, 50)
    seeds = vid([hub]) if level == 2 else vid([p, q, s])
    return g.case(f"long_parent_L{level}", seeds, expect={"level": level, "spans": (1, 200, 800)})


def hub_three_tiles():
    """a hub of 3 x 256 + 5 children; every seventh child has a child"""
    g = _Graph()
    hub = g.new()
    kids = g.fan(hub, 3 * XT + 5)
    for w in kids[::7]:
        g.fan(w, 1)
    return g.case("hub_773", vid([hub]), expect={"totals": [3 * XT + 5, len(kids[::7])]})


def tile_border_cases():
    return ([total_children(T) for T in TOTALS] + [degree_one_parents(256), degree_one_parents(257)]
            + [long_parent(1), long_parent(2), hub_three_tiles()])


WAVE_PARENTS = (64, 64 + 1, 256 + 63)
WAVE_PATTERNS = ("distinct", "same", "first", "32nd", "lane63", "last")


def wave_pattern(n, pattern):
    """n level-1 seeds of one class, seen, one child each: lane p % 64 of wave p / 64 of k_reach_expand claims the child
    of seed p.  distinct: n new vertices, every lane wins.  same: one new vertex, one of n claimers wins.  first / 32nd
    / lane63 / last: only that seed's child is new, every other seed points at the next seed, which is seen.  The seeds
    form a cycle then, so the walk closure and the level sets run under a bound."""
    g = _Graph()
    parents = g.new(n)
    single = {"first": 0, "32nd": 31, "lane63": 63, "last": n - 1}.get(pattern)
    if pattern == "distinct":
        for p in parents:
            g.fan(p, 1)
    elif pattern == "same":
        x = g.new()
        for p in parents:
            g.edge(p, x)
    else:
        x = g.new()
        for i, p in enumerate(parents):
            g.edge(p, x if i == single else parents[(i + 1) % n])
    new = {"distinct": n, "same": 1}.get(pattern, 1)
    return g.case(f"wave_{n}_{pattern}", vid(parents), bound=3,
                  expect={"totals": [n], "reach_level_1": new, "winner": single, "parents": n})


def wave_cases():
    return [wave_pattern(n, pattern) for n in WAVE_PARENTS for pattern in WAVE_PATTERNS]


def hash_homes(cap, fanout, class_limit=1 << 14):
    """Seeds of one vertex s with `fanout` children, in classes chosen so that at least three (class, child) pairs home
    in slot cap - 1 and one in cap - 2: the claims of level 1 probe past the last slot and wrap to slot 0.  The seeds are
    not seen, so level 1 inserts into an empty set; reach runs with `cap` forced first slots, which the growth rule
    leaves alone (visited + M <= cap / 2 at every level), and the level sets' hash form has cap = 1024 for M <= 512."""
    g = _Graph()
    s = g.new()
    kids = g.fan(s, fanout)  # dense indices 1 .. fanout
    last, before = [], []
    for c in range(class_limit):
        homes = [home_slot(c, w, cap) for w in kids]
        if homes.count(cap - 1) and sum(n for _, n in last) < 3:
            last.append((c, homes.count(cap - 1)))
        elif homes.count(cap - 2) and not before and not homes.count(cap - 1):
            before.append((c, homes.count(cap - 2)))
        if sum(n for _, n in last) >= 3 and before:
            break
    classes = sorted(c for c, _ in last + before)
    assert sum(n for _, n in last) >= 3 and before, (cap, fanout)
    M = fanout * len(classes)
    assert 2 * M <= cap and M <= 512
    return g.case(f"hash_homes_{cap}", vid([s] * len(classes)), classes=classes, seen=np.zeros(len(classes), bool),
                  reach_forms=((1, 0), (2, cap)),
                  expect={"cap": cap, "kids": kids, "home_last": 3, "home_before": 1})


def hash_home_cases():
    return [hash_homes(64, 4), hash_homes(1024, 8)]


GROWTH_BOUND = 32  # 2 * (visited + M) before level 2 of growth_boundary()


def growth_boundary():
    """One seen seed with 3 children and 12 grandchildren: before level 1 the rule's bound 2 * (visited + M) is
    2 * (1 + 3) = 8, before level 2 it is 2 * (4 + 12) = 32.  Forced first slots of 32 and 33 are left alone; 31 < 32
    must grow, by a rebuild that inserts the seen seeds and level 1 again (two more reach_insert launches)."""
    g = _Graph()
    s = g.new()
    for w in g.fan(s, 3):
        g.fan(w, 4)
    return g.case("growth_boundary", vid([s]), ops=(REACH,),
                  reach_forms=tuple((2, GROWTH_BOUND + d) for d in (0, 1, -1)),
                  expect={"bounds": [8, GROWTH_BOUND]})


CLASS_COUNTS = (1, 2, 255, 256, 257, 65536, 65537, 1 << 31, (1 << 31) + 1, (1 << 32) - 1)
BITMAP_MAX_BITS = 1 << 33


def class_width(n_classes):
    """A handful of seeds in the top classes n_classes - 1 and n_classes - 2 over a graph of 7 vertices.  The hash forms
    of both operators run on every width; the bitmap forms where n_classes x V is within the budget of 2^33 bits."""
    g = _Graph()
    s0, s1 = g.new(), g.new()
    w = g.new(3)
    g.edge(s0, w[0]), g.edge(s0, w[1]), g.edge(s1, w[2]), g.edge(s1, w[1])
    x = g.fan(w[1], 2)
    g.edge(w[2], x[0])
    top = n_classes - 1
    low = max(top - 1, 0)
    seeds, classes = vid([s1, s0, s0, s1, s0]), [top, top, low, low, top]
    seen = [True, False, True, True, False]
    bitmap = n_classes * g.n <= BITMAP_MAX_BITS
    return g.case(f"classes_{n_classes}", seeds, classes=classes, seen=seen, n_classes=n_classes, ops=(REACH, LEVELS),
                  reach_forms=((1, 0), (2, 0), (0, 0)) if bitmap else ((2, 0), (0, 0)),
                  levels_forms=None if bitmap else ((2, 1), (0, 0)), expect={"bitmap": bitmap})


def class_width_cases():
    return [class_width(n) for n in CLASS_COUNTS]


def all_cases():
    """every case that goes through the operators whole, by name"""
    cases = (zero_run_cases() + tile_border_cases() + wave_cases() + hash_home_cases() + [growth_boundary()]
             + class_width_cases())
    out = {c.name: c for c in cases}
    assert len(out) == len(cases)
    return out


# ---- the frontiers of a case -----------------------------------------------------------------------------------------
def exact_rows(case, op):
    """(column 0, column 1, level) of the operator's exact reference on the case"""
    from tests.test_gpu_level_sets import exact_levels
    from tests.test_gpu_reach_closure import exact_reach
    from tests.test_gpu_walk_closure import exact_closure

    if op == WALK:
        rowid = np.arange(case.src.size, dtype=np.int64)
        return exact_closure(case.src, case.dst, rowid, case.seeds, None if case.bound < 0 else case.bound)
    if op == REACH:
        return exact_reach(case.src, case.dst, case.vertices, case.seeds, case.classes, case.seen)
    return exact_levels(case.src, case.dst, case.vertices, case.seeds, case.classes, case.bound)


def frontiers(case, op, rows=None):
    """The out-degrees of every frontier the operator expands on the case, in frontier order: [0] the seeds, [L] the
    rows of level L (the walk closure's: the end vertex of the row's edge)."""
    degree = dict(zip(*np.unique(case.src, return_counts=True)))
    is_vertex = set(case.vertices.tolist())
    deg_of = lambda ids: np.array([int(degree.get(v, 0)) if v in is_vertex else 0 for v in np.asarray(ids).tolist()],  # noqa: E731
                                  np.int64)
    col0, col1, lev = exact_rows(case, op) if rows is None else rows
    out = [deg_of(case.seeds)]
    for L in range(1, (int(lev.max()) if lev.size else 0) + 1):
        ends = case.dst[col1[lev == L]] if op == WALK else col1[lev == L]
        out.append(deg_of(ends))
    return out


# ---- the larger inputs of tests/test_gpu_closure_edges.py ------------------------------------------------------------
BIG_V = BIG_CLASSES = 70001  # 4.90e9 bits: past 2^32, inside the 2^33 budget
BIG_SEED_CLASSES = (0, 61355, 61356, 70000)


def bits_past_2_32():
    """70 001 vertices and as many classes.  Bit class * V + vertex passes 2^32 inside class 61 355 (at vertex index
    55 941) and stays above it from class 61 356 on.  Every class is seeded at the root (index 0), whose children have the
    indices 5, 14 059, 14 065 and V - 1 = 70 000: modulo 2^32 the bits of (61 356, 5) and (0, 14 065) are the same bit, as
    are those of (61 355, 70 000) and (0, 14 059) — an index cut to 32 bits loses a row of level 1."""
    V = BIG_V
    assert 61355 * V < 1 << 32 < 61355 * V + V - 1 and 61356 * V > 1 << 32
    assert (61356 * V + 5) % (1 << 32) == 14065 and (61355 * V + V - 1) % (1 << 32) == 14059
    edges = [(0, 5), (0, 14059), (0, 14065), (0, V - 1), (5, V - 1), (5, 1), (14065, 1), (14065, 2), (V - 1, 0),
             (V - 1, 55940), (V - 1, 55941), (14059, 55941), (55941, 55942), (55940, V - 2), (1, 3), (2, 3), (3, 0),
             (V - 2, V - 1), (55942, 4), (4, 14060), (14060, 14058), (1, 14058), (2, 69999), (69999, 6), (6, 7)]
    src, dst = (vid([e[i] for e in edges]) for i in (0, 1))
    seeds = vid([0] * len(BIG_SEED_CLASSES) + [V - 1])
    classes = list(BIG_SEED_CLASSES) + [61355]
    return Case("bits_past_2_32", vid(np.arange(V)), src, dst, seeds, classes, np.zeros(len(classes), bool), bound=3,
                ops=(REACH, LEVELS), n_classes=BIG_CLASSES, reach_forms=((1, 0),), levels_forms=((1, 1), (1, 2)))


ROUTE_V = ROUTE_CLASSES = 20000
LEVELS_SORT_FIXED_BYTES = 128 << 20  # gg_levels.hip


def levels_compact_threshold(V, n_classes):
    """the smallest level estimate at which gg_level_sets' byte model takes the compact route over a bitmap:
    11 W <= 24 p n + LEVELS_SORT_FIXED_BYTES (gg_levels.hip), W words in whole groups of four, p radix passes of 8 bits"""
    bits_for = lambda n: max(1, (n - 1).bit_length())  # noqa: E731
    words = 4 * max((V * n_classes + 127) // 128, 1)
    passes = (bits_for(V) + 7) // 8 + ((bits_for(n_classes) + 7) // 8 if n_classes > 1 else 0)
    need = 11 * words - LEVELS_SORT_FIXED_BYTES
    return max(0, -(-need // (24 * passes)))


def route_switch():
    """20 000 vertices x 20 000 classes (a 50 MB bitmap).  Three seeds of one vertex in three classes; level 1 has 3
    children (sort), level 2 a hub's 15 000 children in each class, 45 000 (compact), level 3 six (sort again)."""
    g = _Graph()
    s, hub = g.new(), g.new()
    g.edge(s, hub)
    kids = g.fan(hub, 15000)
    g.fan(kids[10], 1), g.fan(kids[14000], 1)
    g.new(ROUTE_V - g.n)
    classes = [0, 9999, ROUTE_CLASSES - 1]
    return g.case("route_switch", vid([s] * 3), classes=classes, seen=np.zeros(3, bool), n_classes=ROUTE_CLASSES,
                  ops=(LEVELS,), levels_forms=((0, 0),), expect={"children": [3, 45000, 6]})


def memset_cheaper():
    """a 16-byte bitmap: from level 2 on the frontier's 8 n bytes are no less than the whole map's 4 W = 16"""
    g = _Graph()
    a, b = g.new(), g.new()
    for _ in range(3):
        c, d = g.new(), g.new()
        g.edge(a, c), g.edge(b, d)
        a, b = c, d
    return g.case("memset_cheaper", vid([0, 1]), ops=(LEVELS,), levels_forms=((0, 0),))


def hub_65536():
    """a hub of 65 536 children: seeded 65 536 times, level 1 has 2^32 children"""
    g = _Graph()
    hub = g.new()
    g.fan(hub, 1 << 16)
    return g.case("hub_65536", np.full(1 << 16, vid(hub), np.int64))


def unequal_levels():
    """levels of 3, 7, 2, 5 and 1 rows in all three operators (a tree, every seed its own class)"""
    g = _Graph()
    level = [g.new()]
    for width in (3, 7, 2, 5, 1):
        kids = []
        for i in range(width):
            kids += g.fan(level[i % len(level)], 1)
        level = kids
    return g.case("unequal_levels", vid([0]), seen=[False], expect={"levels": [3, 7, 2, 5, 1]})
