"""Small graphs that steer the direction of every level of the 64-lane BFS by construction (tests/test_gpu_bfs_levels.py).

A level pulls when the frontier it starts from has more than E / factor edges (factor = 8, GG_BFS_PULL_FACTOR), so the
direction is steered through E and nothing else:

  ballast   a block of vertices no source can reach, holding at least 8 x the edges of the part under test: every
            frontier then has te * 8 <= E and every level pushes;
  no slack  all edges start in the frontier: a one-level star whose rows all start at a source has te_0 = E, complete
            bipartite layers seeded with the whole first layer have te = E / layers (at most 7 layers): every level pulls.
            A level whose frontier has no out-edge at all (te = 0) pushes, and finds nothing.

Every builder returns a Shape with the direction sequence it was built for; tests/test_bfs_levels_ref_cpu.py holds each
sequence to the reference, so a shape that stops steering fails there and not on the device.  Vertices are dense indices
(the vertex table is 0..V-1 in order); ids >= V and negative ids are no vertices."""
import numpy as np

PUSH, PULL = "push", "pull"
FACTOR = 8


class Shape:
    def __init__(self, name, V, src, dst, sources, directions, symmetric=False):
        self.name, self.V = name, int(V)
        self.src, self.dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
        self.sources = np.asarray(sources, np.int64)
        self.directions = list(directions)
        self.symmetric = symmetric  # rows i and i + E/2 mirror each other (the derived-reverse build forms)
        self.vid = np.arange(self.V, dtype=np.int64)

    def mirrored(self, directions):
        """the same graph with every row also reversed (row i + E/2 = row i swapped), and the sequence THAT graph is built for"""
        return Shape(self.name + "_mirrored", self.V, np.concatenate([self.src, self.dst]),
                     np.concatenate([self.dst, self.src]), self.sources, directions, symmetric=True)


def _cat(parts):
    parts = [np.asarray(p, np.int64).reshape(-1) for p in parts]
    return np.concatenate(parts) if parts else np.empty(0, np.int64)


def ballast(min_edges, base, multiple=1):
    """(number of vertices, src, dst): vertices base .. base + n - 1, each with 32 out-edges inside the block"""
    n = max(64, -(-min_edges // 32))
    n = -(-n // multiple) * multiple
    v = np.arange(n, dtype=np.int64)
    src = np.repeat(v, 32)
    dst = (src + np.tile(np.arange(1, 33, dtype=np.int64), n)) % n
    return n, src + base, dst + base


def full(a, b):
    """every vertex of a -> every vertex of b"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    return np.repeat(a, b.size), np.tile(b, a.size)


# ---- push rows ---------------------------------------------------------------------------------------------------------
HUB_DEGREES = [0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025]  # around the push walk's 64-entry step and 256-entry trip


def push_rows(layout="front"):
    """12 hub sources on their own lanes; the spokes of neighbouring hubs overlap, so several lanes OR into one word.
    layout "front": hubs, spokes, ballast.  layout "corners": the same graph relabelled so that hubs sit at dense indices 0,
    63, 64 and V - 1 (the last one reads off[V])."""
    n_spokes = 1100
    hubs = np.arange(12, dtype=np.int64)
    spokes = 12 + np.arange(n_spokes, dtype=np.int64)
    s, d = [], []
    for j, deg in enumerate(HUB_DEGREES):
        s.append(np.full(deg, hubs[j]))
        d.append(spokes[(j * 37 + np.arange(deg)) % n_spokes])
    nb, bs, bd = ballast(8 * sum(HUB_DEGREES), 12 + n_spokes)
    V = 12 + n_spokes + nb
    src, dst = _cat(s + [bs]), _cat(d + [bd])
    sources = hubs.copy()
    if layout == "corners":
        label = np.arange(V, dtype=np.int64)
        for hub, at in ((11, V - 1), (10, 64), (9, 63), (8, 0)):  # degrees 1025, 513, 512, 511
            a, b = int(label[hub]), at
            ia, ib = np.flatnonzero(label == a)[0], np.flatnonzero(label == b)[0]
            label[ia], label[ib] = b, a
        src, dst, sources = label[src], label[dst], label[sources]
    else:
        assert layout == "front"
    # level 1 walks the hubs' rows, level 2 starts from spokes without out-edges and finds nothing
    return Shape("push_rows_" + layout, V, src, dst, sources, [PUSH, PUSH])


# ---- pull rows ---------------------------------------------------------------------------------------------------------
IN_DEGREES = [0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 257]  # around the pull walk's 8-entry trip


def reverse_rows(V, src, dst):
    """(roff, rnbr) in edge-row order, the order the default build keeps; the GPU tests pass what export_reverse returns"""
    keep = (src >= 0) & (src < V) & (dst >= 0) & (dst < V)
    s, d = src[keep], dst[keep]
    order = np.argsort(d, kind="stable")
    return np.concatenate([[0], np.cumsum(np.bincount(d, minlength=V))]), s[order]


def pull_rows(variant, reverse=None):
    """Targets with the in-degrees above; every in-neighbour is a vertex of its own (variants a, b) with that one out-edge.

    a  only the in-neighbour in the LAST position of a target's reverse row is a source (it carries the lanes l with
       l mod 11 = the target's number; lane 0 sits on the heavy vertex): the walk cannot stop early and must read its tail.
    b  the in-neighbour in the FIRST position of every row is one vertex X that carries all 64 lanes: every row is
       complete after its first trip.
    c  position p of a row is the source of lane p mod 64 (64 shared source vertices, parallel rows past 64): an 8-entry
       row must come out with exactly 8 distinct bits, a 64-entry row with all 64 -- the lane-group OR -- and the
       targets lie at dense indices 8j + g for every slot g of a wavefront's 8 groups.
    The positions are those of `reverse` = (roff, rnbr), the library's own reverse rows of this graph (the graph does not
    depend on it, only the choice of sources in variant a); without it, edge-row order.  In a and b a heavy source with 200
    rows of its own takes te_0 * 8 past E.  Level 1 pulls; level 2 starts from targets without out-edges."""
    s, d = [], []
    if variant == "c":
        lanes = np.arange(64, dtype=np.int64)           # lane k starts at vertex k
        targets = 64 + np.arange(96, dtype=np.int64)    # 64 = 8 * 8: target i sits in group slot i % 8
        degs = [IN_DEGREES[(i // 8 + i % 8) % 12] for i in range(96)]
        for t, deg in zip(targets, degs):
            s.append(lanes[np.arange(deg) % 64])
            d.append(np.full(deg, t))
        V = 64 + 96
        return Shape("pull_rows_c", V, _cat(s), _cat(d), lanes, [PULL, PUSH])
    n_t = len(IN_DEGREES)
    heavy, x = 0, 1
    targets = 2 + np.arange(n_t, dtype=np.int64)
    sinks = 2 + n_t + np.arange(200, dtype=np.int64)
    nxt = 2 + n_t + 200
    if variant == "b":
        for t, deg in zip(targets, IN_DEGREES):  # X's rows first: X leads every reverse row in edge-row order
            if deg:
                s.append([x])
                d.append([t])
    for t, deg in zip(targets, IN_DEGREES):
        own = deg - (1 if variant == "b" and deg else 0)
        s.append(nxt + np.arange(own))
        d.append(np.full(own, t))
        nxt += own
    s.append(np.full(200, x if variant == "b" else heavy))  # (b: X itself is the heavy one, te_0 = 211 of E = 722)
    d.append(sinks)
    V = nxt
    src, dst = _cat(s), _cat(d)
    if variant == "b":
        return Shape("pull_rows_b", V, src, dst, np.full(64, x, np.int64), [PULL, PUSH])
    assert variant == "a"
    roff, rnbr = reverse if reverse is not None else reverse_rows(V, src, dst)
    last = [int(rnbr[roff[t + 1] - 1]) for t, deg in zip(targets, IN_DEGREES) if deg]
    sources = np.array([heavy] + [last[(l - 1) % len(last)] for l in range(1, 64)], np.int64)
    return Shape("pull_rows_a", V, src, dst, sources, [PULL, PUSH])


def complete_target():
    """X carries all 64 lanes from the seed on and lies in its own reverse row and in Y's: pull levels skip it (every lane
    seen) and must write an empty word for it.  X -> X, X -> Y, Y -> X, Y -> Z."""
    return Shape("complete_target", 3, [0, 0, 1, 1], [0, 1, 0, 2], [0] * 64, [PULL, PULL, PUSH])


# ---- V around the push chunk (64 words a wavefront) and the pull group (8 vertices a wavefront) ---------------------------
V_EDGES = [1, 7, 8, 9, 63, 64, 65, 127, 129]


def _star(V, base=0):
    """min(64, V // 2) sources (the LAST vertices when V is odd, so V - 1 is a source, else the first), each with a row to
    every other vertex; V = 1: a self loop"""
    if V == 1:
        return np.array([base]), np.array([base]), np.array([base])
    k = min(64, V // 2)
    v = np.arange(V, dtype=np.int64) + base
    srcs, rest = (v[V - k:], v[:V - k]) if V % 2 else (v[:k], v[k:])
    a, b = full(srcs, rest)
    return a, b, srcs


def star_pull(V, lanes=None):
    """one-level star of V vertices, no ballast: te_0 = E.  V = 1: `lanes` lanes on the self loop (the vertex is never new
    again: level 1 pulls and finds nothing)"""
    src, dst, srcs = _star(V)
    if V == 1:
        return Shape(f"star_pull_V1_{lanes}", 1, src, dst, np.full(lanes, 0), [PULL])
    return Shape(f"star_pull_V{V}", V, src, dst, srcs, [PULL, PUSH])


def star_push(V):
    """the same star behind a ballast block of a multiple of 128 vertices: the star ends the vertex array, at a length
    that is V modulo 64 and modulo 8"""
    _, _, probe = _star(V)
    n_probe = max(1, (V - probe.size) * probe.size)
    nb, bs, bd = ballast(8 * n_probe, 0, multiple=128)
    src, dst, srcs = _star(V, base=nb)
    return Shape(f"star_push_V{V}", nb + V, _cat([bs, src]), _cat([bd, dst]), srcs, [PUSH] if V == 1 else [PUSH, PUSH])


# ---- transitions -------------------------------------------------------------------------------------------------------
def _layers(widths, start=0):
    out = []
    for w in widths:
        out.append(np.arange(start, start + w, dtype=np.int64))
        start += w
    return out, start


def transitions(start="push"):
    """64 parallel chains into a bipartite block and out again: H =1:1=> A =full=> B =full=> C =1:1=> D =full=> F =1:1=> G, all
    64 wide, lane i seeded at H_i (start "push") or at A_i (start "pull").  E = 3 * 4096 + 3 * 64 (less 64 without H): a
    64-vertex frontier of 1:1 rows pushes (512 <= E), one of full rows pulls (32768 > E); G has no out-edges.
    cur runs 0,0,1,0,0,1,1,1: every push after a pull reads the buffer the pull wrote and needs `fnext` clean."""
    (H, A, B, C, D, F, G), V = _layers([64] * 7)
    parts = [(A, B, True), (B, C, True), (C, D, False), (D, F, True), (F, G, False)]
    dirs = [PULL, PULL, PUSH, PULL, PUSH, PUSH]
    if start == "push":
        parts, dirs = [(H, A, False)] + parts, [PUSH] + dirs
    s, d = [], []
    for a, b, is_full in parts:
        x, y = full(a, b) if is_full else (a, b)
        s.append(x)
        d.append(y)
    return Shape("transitions_" + start, V, _cat(s), _cat(d), H if start == "push" else A, dirs)


def funnel_mirrored():
    """The transitions of an undirected graph, where a wide layer's back edges keep it heavy and lanes that travel apart
    would flow back: all 64 lanes start at h and move in step.  h - a =all= B(64) =full= C(64) =all= n - m =all= G(64) =full=
    K(64), every row mirrored.  E = 2 * 8386, a level pulls above 2096 edges; te: h 1 and a 65 (push), B and C 64 * 65
    (pull), n and m 65 (push), G 64 * 65 (pull), K 4096 (a pull that finds nothing).  cur runs 0,0,0,1,0,0,0,1,0."""
    (h, a, B, C, n, m, G, K), V = _layers([1, 1, 64, 64, 1, 1, 64, 64])
    s, d = [], []
    for p, q in ((h, a), (a, B), (B, C), (C, n), (n, m), (m, G), (G, K)):
        x, y = full(p, q)
        s.append(x)
        d.append(y)
    return Shape("funnel", V, _cat(s), _cat(d), np.full(64, h[0]), []).mirrored(
        [PUSH, PUSH, PULL, PULL, PUSH, PUSH, PULL, PULL])


def pull_rows_c_mirrored():
    """pull_rows("c") undirected (E = 8352, the targets' rows sum to 4176): sources and targets take turns as the frontier
    and every frontier holds half the edges, until (level 4) the targets of fewer than 64 rows are the last to gain
    lanes: 1088 edges, 8704 > 8352, a pull that finds every row complete."""
    return pull_rows("c").mirrored([PULL, PULL, PULL, PULL])


# ---- level counts around the host's read-back chunk (6 levels) -------------------------------------------------------------
ECCENTRICITIES = [5, 6, 7, 11, 12, 13]
HOP_BOUNDS = [0, 1, 5, 6, 7, 11, 12, 13, -1]


def chain(ecc, lanes=3):
    """ecc + 1 vertices in a row, `lanes` lanes at the head: te = 1, so the levels pull while 8 > E = ecc and push from
    ecc = 8 on; the level after the last vertex has te = 0"""
    v = np.arange(ecc + 1, dtype=np.int64)
    return Shape(f"chain_{ecc}", ecc + 1, v[:-1], v[1:], np.zeros(lanes, np.int64),
                 [PULL if FACTOR > ecc else PUSH] * ecc + [PUSH])


def layered(ecc, width=4):
    """ecc + 1 layers of `width` vertices, full rows between neighbours, seeded with the first layer (lane i at its
    vertex i): te = E / ecc, so every level pulls up to 7 layers of rows and pushes beyond"""
    layers, V = _layers([width] * (ecc + 1))
    s, d = zip(*[full(a, b) for a, b in zip(layers[:-1], layers[1:])])
    return Shape(f"layered_{ecc}", V, _cat(s), _cat(d), layers[0], [PULL if FACTOR > ecc else PUSH] * ecc + [PUSH])


def late_pull(k):
    """two parallel chains for k - 1 levels, then 2 -> 64 full rows (level k pulls: 128 * 8 > E = 2k + 190) and 64 1:1 rows
    (level k + 1 pulls: 64 * 8 > E); the chain levels push (2 * 8 <= E).  k = 6, 7: a pull as the last level of the host's
    first chunk and as the first of its second."""
    layers, V = _layers([2] * k + [64, 64])
    s, d = [], []
    for a, b in zip(layers[:k - 1], layers[1:k]):
        s.append(a)
        d.append(b)
    x, y = full(layers[k - 1], layers[k])
    return Shape(f"late_pull_{k}", V, _cat(s + [x, layers[k]]), _cat(d + [y, layers[k + 1]]), layers[0],
                 [PUSH] * (k - 1) + [PULL, PULL, PUSH])


# ---- two-byte cells --------------------------------------------------------------------------------------------------------
def deep_all_lanes():
    """A chain of 330 vertices whose first 64 are the 64 sources (lane i at vertex i: every lane reaches every later vertex
    at a level of its own), ending in three full layers of 32.  E = 329 + 32 + 2 * 1024 = 2409: chain frontiers (at most 64
    rows of one entry, 96 at the chain's end) push; from level 267 on the frontier holds the first layer, 1024 edges, and
    levels 268 .. 332 pull -- all of them past what a one-byte cell records.  Lane i reaches the last layer at level
    332 - i >= 269."""
    c = np.arange(330, dtype=np.int64)
    (l0, l1, l2), V = _layers([32] * 3, 330)
    parts = [(c[:-1], c[1:]), full(c[-1:], l0), full(l0, l1), full(l1, l2)]
    return Shape("deep_all_lanes", V, _cat([p[0] for p in parts]), _cat([p[1] for p in parts]), c[:64],
                 [PUSH] * 267 + [PULL] * 65 + [PUSH])


def long_chain(n_vertices, lanes=4):
    """a plain chain from its head; from 9 vertices on every level pushes"""
    v = np.arange(n_vertices, dtype=np.int64)
    return Shape(f"long_chain_{n_vertices}", n_vertices, v[:-1], v[1:], np.zeros(lanes, np.int64),
                 [PUSH] * n_vertices)


# every shape the CPU test holds to its sequence and the GPU test runs; built on first use
BUILDERS = {
    "push_rows_front": lambda: push_rows("front"),
    "push_rows_corners": lambda: push_rows("corners"),
    "pull_rows_a": lambda: pull_rows("a"),
    "pull_rows_b": lambda: pull_rows("b"),
    "pull_rows_c": lambda: pull_rows("c"),
    "complete_target": complete_target,
    "transitions_push": lambda: transitions("push"),
    "transitions_pull": lambda: transitions("pull"),
    "funnel_mirrored": funnel_mirrored,
    "pull_rows_c_mirrored": pull_rows_c_mirrored,
    "late_pull_6": lambda: late_pull(6),
    "late_pull_7": lambda: late_pull(7),
    "deep_all_lanes": deep_all_lanes,
    "long_chain_254": lambda: long_chain(254),
    "long_chain_255": lambda: long_chain(255),
    "long_chain_256": lambda: long_chain(256),
}
BUILDERS.update({f"star_pull_V1_{n}": (lambda n=n: star_pull(1, n)) for n in (1, 2, 64)})
BUILDERS.update({f"star_pull_V{v}": (lambda v=v: star_pull(v)) for v in V_EDGES[1:]})
BUILDERS.update({f"star_push_V{v}": (lambda v=v: star_push(v)) for v in V_EDGES})
BUILDERS.update({f"chain_{e}": (lambda e=e: chain(e)) for e in ECCENTRICITIES})
BUILDERS.update({f"layered_{e}": (lambda e=e: layered(e)) for e in ECCENTRICITIES})

_built = {}


def shape(name):
    if name not in _built:
        _built[name] = BUILDERS[name]()
        assert _built[name].name == name, (name, _built[name].name)
    return _built[name]
