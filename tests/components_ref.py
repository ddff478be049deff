"""Weakly connected components restated in plain python / numpy (include/gg.h, gg_components): the yardstick of the device
kernels.

Two vertices are in one component iff a path of kept edge rows joins them, direction ignored; a row with an endpoint that is
no vertex does not exist.  The representative of a component is its member with the smallest dense index (position in the
vertex table) and the component's id is that vertex's id.  Table 0: one row (vertex id, component id, size) per vertex in
vertex-table order; table 1: one row (component id, size) per component, ascending by the representative's position."""
import numpy as np


def dense_edges(vid, src, dst):
    """(su, dv): dense endpoints of the kept edge rows, in row order (vid: distinct ids)"""
    vid = np.asarray(vid, np.int64)
    src, dst = np.asarray(src, np.int64).reshape(-1), np.asarray(dst, np.int64).reshape(-1)
    if vid.size == 0 or src.size == 0:
        return np.empty(0, np.int64), np.empty(0, np.int64)
    order = np.argsort(vid, kind="stable")
    ids = vid[order]

    def index(x):
        at = np.minimum(np.searchsorted(ids, x), ids.size - 1)
        return np.where(ids[at] == x, order[at], -1)

    su, dv = index(src), index(dst)
    keep = (su >= 0) & (dv >= 0)
    return su[keep], dv[keep]


def roots(V, su, dv):
    """root[v] = smallest dense index of v's component: a union-find that links the larger root under the smaller one,
    halving paths on the way"""
    parent = list(range(V))
    for a, b in zip(su.tolist(), dv.tolist()):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        while parent[b] != b:
            parent[b] = parent[parent[b]]
            b = parent[b]
        if a < b:
            parent[b] = a
        elif b < a:
            parent[a] = b
    for v in range(V):  # ascending: parent[v] < v is final already
        parent[v] = parent[parent[v]]
    return np.array(parent, np.int64).reshape(-1)


def components(vid, src, dst):
    """everything GG.components returns, but jump_launches: {"stats", "vertex", "component", "size", "components", "sizes"}"""
    vid = np.asarray(vid, np.int64).reshape(-1)
    V = int(vid.size)
    su, dv = dense_edges(vid, src, dst)
    root = roots(V, su, dv)
    count = np.bincount(root, minlength=V).astype(np.uint64) if V else np.empty(0, np.uint64)
    reps = np.nonzero(root == np.arange(V))[0]
    sizes = count[reps]
    stats = {"vertices": V, "components": int(reps.size), "largest": int(sizes.max()) if V else 0,
             "singletons": int((sizes == 1).sum()), "entries_read": int(su.size), "hooks": V - int(reps.size)}
    return {"stats": stats, "vertex": vid, "component": vid[root] if V else vid, "size": count[root] if V else count,
            "components": vid[reps], "sizes": sizes}


def brute_force_roots(V, su, dv):
    """the same labels by a breadth-first search from every vertex not yet labelled, in dense-index order"""
    adj = [[] for _ in range(V)]
    for a, b in zip(su.tolist(), dv.tolist()):
        adj[a].append(b)
        adj[b].append(a)
    root = [-1] * V
    for s in range(V):
        if root[s] >= 0:
            continue
        root[s] = s
        frontier = [s]
        while frontier:
            nxt = []
            for u in frontier:
                for w in adj[u]:
                    if root[w] < 0:
                        root[w] = s
                        nxt.append(w)
            frontier = nxt
    return np.array(root, np.int64).reshape(-1)


def min_id_partition(answer):
    """{vertex id: (smallest id of its component, size)}: what the recursive-CTE statement reports per vertex"""
    vertex, comp = answer["vertex"].tolist(), answer["component"].tolist()
    smallest = {}
    for v, c in zip(vertex, comp):
        smallest[c] = min(smallest.get(c, v), v)
    return {v: (smallest[c], int(s)) for v, c, s in zip(vertex, comp, answer["size"].tolist())}


def sql_und(person="person", key="p_personid", knows="knows", a="k_person1id", b="k_person2id") -> str:
    """the table `und`: every kept edge row in both directions (the reference refuses a UNION inside a recursive CTE's arm,
    so the statement below reads it as a table)"""
    kept = f"FROM {knows} k, {person} p1, {person} p2 WHERE p1.{key} = k.{a} AND p2.{key} = k.{b}"
    return f"CREATE TABLE und AS SELECT k.{a} AS a, k.{b} AS b {kept} UNION ALL SELECT k.{b} AS a, k.{a} AS b {kept}"


def sql_components(person="person", key="p_personid") -> str:
    """the UNION recursive CTE under an aggregate: (v, smallest id of v's component, members of v's component)"""
    return (f"WITH RECURSIVE cc(v, root) AS (SELECT {key}, {key} FROM {person} "
            f"UNION SELECT u.b, cc.root FROM cc, und u WHERE cc.v = u.a) "
            f"SELECT v, min(root), count(*) FROM cc GROUP BY v")


# ---- the shapes of tests/test_gpu_components.py: (vid, src, dst) each
def path(n, order="forward", seed=0, first_id=1000):
    """a path of n vertices, id i -> id i + 1; the vertex table in path order, reversed, or shuffled"""
    ids = np.arange(first_id, first_id + n, dtype=np.int64)
    vid = ids if order == "forward" else ids[::-1].copy() if order == "reverse" else ids[np.random.RandomState(seed).permutation(n)]
    return vid, ids[:-1].copy(), ids[1:].copy()


def star(leaves, hub_first):
    """every leaf -> the hub; the hub is the first or the last row of the vertex table"""
    hub = np.array([7], np.int64)
    ids = np.arange(100, 100 + leaves, dtype=np.int64)
    vid = np.concatenate([hub, ids]) if hub_first else np.concatenate([ids, hub])
    return vid, ids.copy(), np.full(leaves, 7, np.int64)


def pairs(n):
    """n disjoint pairs, neighbours in the vertex table: every wave holds 32 roots"""
    vid = np.arange(2 * n, dtype=np.int64) * 3 + 1
    return vid, vid[0::2].copy(), vid[1::2].copy()


def straddling(members=64 * 5 + 3, stride=3):
    """one component of `members` vertices (a shuffled path) beside singletons, interleaved in the vertex table so that every
    wave holds members and singletons"""
    rng = np.random.RandomState(5)
    V = members * stride
    vid = np.arange(V, dtype=np.int64) + 50
    chain = vid[::stride][rng.permutation(members)]
    return vid, chain[:-1].copy(), chain[1:].copy()


def late_merge(n=1 << 14):
    """two shuffled paths of n vertices each, joined by one row appended last"""
    v1, s1, d1 = path(n, "shuffle", 1, first_id=0)
    v2, s2, d2 = path(n, "shuffle", 2, first_id=10 * n)
    vid = np.concatenate([v1, v2])[np.random.RandomState(3).permutation(2 * n)]
    return vid, np.concatenate([s1, s2, v2[-1:]]), np.concatenate([d1, d2, v1[-1:]])


def ring_with_chords(V, seed=None):
    """a graph of V vertices in a few pieces: rings over slices of a shuffled vertex table plus random chords inside them,
    and the last two vertices left alone"""
    rng = np.random.RandomState(V if seed is None else seed)
    vid = (np.arange(V, dtype=np.int64) * 7 + 3)[rng.permutation(V)]
    cut = sorted({0, V // 3, V // 2, max(V - 2, 0)})
    src, dst = [], []
    for lo, hi in zip(cut[:-1], cut[1:]):
        part = vid[lo:hi][rng.permutation(hi - lo)]
        src += [part, part[rng.randint(0, part.size, part.size)]]
        dst += [np.roll(part, -1), part[rng.randint(0, part.size, part.size)]]
    return vid, np.concatenate(src), np.concatenate(dst)


def islands(V=300, seed=11):
    """about V vertices for the statements in SQL: a giant component, a few small ones, singletons, rows in one direction
    only, parallel rows, a self-loop and dangling rows; the vertex table is not in id order"""
    rng = np.random.RandomState(seed)
    vid = (np.arange(V, dtype=np.int64) * 5 - 40)[rng.permutation(V)]
    giant, rest = vid[:200], vid[200:]
    src = [giant[rng.randint(0, 200, 420)], giant[:-1]]
    dst = [giant[rng.randint(0, 200, 420)], giant[1:]]
    small = [rest[0:2], rest[2:5], rest[5:12], rest[12:40]]  # the others stay singletons
    for part in small:
        src.append(part[:-1])
        dst.append(part[1:])
    src += [rest[5:7], rest[50:51], np.array([-1000, int(rest[60]), -1001], np.int64)]
    dst += [rest[6:8], rest[50:51], np.array([int(rest[61]), -1002, -1003], np.int64)]  # parallel, a self-loop, dangling
    return vid, np.concatenate(src), np.concatenate(dst)
