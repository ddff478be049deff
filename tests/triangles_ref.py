"""Triangle rows restated in plain numpy / python (include/gg.h, gg_triangles): the yardstick of the device kernel.

A triangle row is a triple of kept edge rows e1: a->b, e2: b->c, e3: c->a — the rows of
    knows k1, knows k2, knows k3 WHERE k1.dst = k2.src AND k2.dst = k3.src AND k3.dst = k1.src
with every endpoint in the vertex table.  Closed walks, not simple cycles: parallel rows multiply, a self-loop is a row."""
import numpy as np


class TriangleGraph:
    """(vid, src, dst) with the dangling edge rows dropped; A[u, v] = number of edge rows u -> v (dense indices)."""

    def __init__(self, vid, src, dst):
        self.vid = np.asarray(vid, np.int64)
        self.V = self.vid.size
        self.index = {int(v): i for i, v in enumerate(self.vid.tolist())}
        src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
        su = np.array([self.index.get(int(s), -1) for s in src.tolist()], np.int64)
        dv = np.array([self.index.get(int(d), -1) for d in dst.tolist()], np.int64)
        keep = (su >= 0) & (dv >= 0)
        self.su, self.dv = su[keep], dv[keep]
        self.A = np.zeros((self.V, self.V), np.int64)
        np.add.at(self.A, (self.su, self.dv), 1)
        order = np.argsort(self.su, kind="stable")
        self.off = np.zeros(self.V + 1, np.int64)
        np.cumsum(np.bincount(self.su, minlength=self.V), out=self.off[1:])
        self.nbr = self.dv[order]  # out-rows with multiplicity, in edge-row order

    def trace_cube(self) -> int:
        """rows of order 0 over all sources = trace(A^3) (float64 products: exact below 2^53)"""
        a = self.A.astype(np.float64)
        return int(round(float(np.einsum("ij,ji->", a @ a, a))))

    def rows(self, order: int = 0, sources=None):
        """(dense rows [N, 3] int64 in enumeration order, wedges looked at).  sources: ids, with multiplicity, ids that
        are no vertices contribute nothing; None: every vertex.  order 1: only id(a) < id(b) < id(c), and only the
        wedges a -> b -> c that ascend are counted as looked at."""
        if sources is None:
            starts = range(self.V)
        else:
            starts = [self.index[int(s)] for s in np.asarray(sources, np.int64).tolist() if int(s) in self.index]
        out, wedges = [], 0
        vid, A = self.vid, self.A
        for a in starts:
            for b in self.nbr[self.off[a]:self.off[a + 1]].tolist():
                if order == 1 and not vid[a] < vid[b]:
                    continue
                cs = self.nbr[self.off[b]:self.off[b + 1]]
                if order == 1:
                    cs = cs[vid[cs] > vid[b]]
                wedges += cs.size
                m = A[cs, a]
                if m.any():
                    c = np.repeat(cs, m)
                    out.append(np.stack([np.full(c.size, a, np.int64), np.full(c.size, b, np.int64), c], axis=1))
        rows = np.concatenate(out, axis=0) if out else np.empty((0, 3), np.int64)
        return rows, int(wedges)

    def id_rows(self, dense_rows):
        return self.vid[dense_rows] if dense_rows.size else np.empty((0, 3), np.int64)


def sql_triangles(select: str = "count(*)", ordered: bool = False, person: str = "person", key: str = "p_personid") -> str:
    """the three-join statement over knows with every endpoint a row of `person` (bi-11.sql:22-33 when ordered)"""
    w = [f"p1.{key} = k1.k_person1id", f"p2.{key} = k2.k_person1id", f"p3.{key} = k3.k_person1id",
         "k1.k_person2id = k2.k_person1id", "k2.k_person2id = k3.k_person1id", "k3.k_person2id = k1.k_person1id"]
    if ordered:
        w += ["k1.k_person1id < k2.k_person1id", "k2.k_person1id < k3.k_person1id"]
    return (f"SELECT {select} FROM {person} p1, {person} p2, {person} p3, knows k1, knows k2, knows k3 WHERE "
            + " AND ".join(w))


SQL_ROWS = "k1.k_person1id, k2.k_person1id, k3.k_person1id"


def hard_graph(V: int = 1500, rows: int = 24_000, seed: int = 0x7A1, hub_fan: int = 600):
    """datagen.ldbc_knows plus what a triangle kernel can get wrong: parallel rows, self-loops (one on a vertex of a
    2-cycle), dangling rows, a hub wired to ~hub_fan vertices in both directions, a negative id, and a vertex table in
    an order that is not the id order."""
    from duckdb_pgq_amd import datagen

    vid, src, dst = datagen.ldbc_knows(V, rows, seed)
    rng = np.random.RandomState(seed & 0xFFFF)
    vid = vid.copy()
    old = int(vid[5])
    vid[5] = -77  # one negative id; its edge rows follow
    src, dst = np.where(src == old, -77, src), np.where(dst == old, -77, dst)
    hub = int(vid[11])
    fan = vid[rng.choice(V, hub_fan, replace=False)]
    fan = fan[fan != hub]
    extra_src = [src[:300], np.full(fan.size, hub, np.int64), fan,
                 np.array([vid[7], vid[20], vid[20], vid[21], -5, vid[3]], np.int64)]
    extra_dst = [dst[:300], fan, np.full(fan.size, hub, np.int64),
                 np.array([vid[7], vid[20], vid[21], vid[20], vid[2], -6], np.int64)]
    # (vid[7]: a self-loop; vid[20]: a self-loop on a vertex of the 2-cycle 20 <-> 21; -5, -6: dangling)
    src = np.concatenate([src] + extra_src)
    dst = np.concatenate([dst] + extra_dst)
    vid = vid[rng.permutation(V)]  # dense order != id order (ldbc_knows hands the ids out ascending)
    return vid, src, dst
