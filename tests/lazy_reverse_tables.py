"""The fully mirrored edge tables of tests/test_lazy_reverse_rows_cpu.py and tests/test_gpu_lazy_reverse_rows.py, and the
numpy model of what a derived build keeps (gg_csr_fast.hip "Derived reverse"): the forward CSR, roff == off, rrow, and
rot[v] = |A|, the number of entries of v's forward row that come from first-half rows.  The reverse rows are the
forward rows rotated by rot (gg_csr.hip: k_rotate_rows)."""
import numpy as np

from duckdb_pgq_amd import datagen
from tests.test_gpu_derived_reverse import mirrored

SHAPES = ("a_packed", "a_direct", "a_wide", "b", "star_out", "star_in", "d")
SMALL = ("a_packed", "star_small_out", "star_small_in")  # few enough 2-hop rows to hash one by one on the host


def ids(kind, V, rng):
    if kind == "packed":  # sparse ids: packed 8-byte dictionary slots
        return datagen.person_ids(V, 11)
    if kind == "direct":  # span < 2^20: direct-address array
        return (np.arange(V, dtype=np.int64) * 2 - 77)[rng.permutation(V)]
    assert kind == "wide", kind  # arbitrary 64-bit ids: 16-byte slots
    v = np.unique(rng.integers(np.iinfo(np.int64).min, np.iinfo(np.int64).max, V + V // 8, dtype=np.int64))
    return v[rng.permutation(v.size)][:V]


def _star(V, leaves, extra, inward, rng):
    """Hub -> `leaves` leaves in the first half (inward: leaves -> hub) and `extra` random rows that avoid the hub: the
    hub's forward row is all A (|B| = 0) one way and all B (|A| = 0) the other; every leaf has the opposite."""
    vid = ids("packed", V, rng)
    hub, others = vid[17], np.delete(vid, 17)
    s = np.concatenate([np.full(leaves, hub, np.int64), others[rng.integers(0, others.size, extra)]])
    d = np.concatenate([others[:leaves], others[rng.integers(0, others.size, extra)]])
    if inward:
        s[:leaves], d[:leaves] = d[:leaves].copy(), s[:leaves].copy()
    return vid, np.concatenate([s, d]), np.concatenate([d, s])


def table(name):
    """(vid, src, dst) of a fully mirrored table: row i + E/2 is row i with source and destination swapped."""
    rng = np.random.default_rng(sum(name.encode()))
    if name.startswith("a_"):  # self-loops, duplicate rows, ids that are no vertex (dropped in pairs)
        vid = ids(name[2:], 300, rng)
        return (vid,) + mirrored(vid, 4096, rng, extras=True)
    if name == "b":  # several buckets, three first-half tiles, 16-vertex groups that end before V
        vid = ids("packed", 5000, rng)
        return (vid,) + mirrored(vid, 40_000, rng)
    if name in ("star_out", "star_in"):  # a group beyond the 1 536-entry stage: the direct-store path
        return _star(2300, 2000, 200, name == "star_in", rng)
    if name in ("star_small_out", "star_small_in"):
        return _star(120, 60, 40, name == "star_small_in", rng)
    assert name == "d", name  # one bucket whose halves together exceed 16 chunks: more than one round of chunks
    vid = ids("packed", 1000, rng)
    return (vid,) + mirrored(vid, 300_000, rng)


def derived_model(vid, src, dst):
    """off, nbr, rrow, rot (int64) as a derived build leaves them, from numpy alone: the kept rows (both ids are
    vertices) sorted stably by dense source; rrow is the row-index expansion of off; rot counts the kept FIRST-half rows
    per source, which stand first in the row since forward rows are in rowid order."""
    order = np.argsort(vid, kind="stable")
    sv = vid[order]

    def dense(x):
        p = np.minimum(np.searchsorted(sv, x), sv.size - 1)
        return np.where(sv[p] == x, order[p], -1).astype(np.int64)

    u, v = dense(src), dense(dst)
    keep = (u >= 0) & (v >= 0)
    first_half = (np.arange(src.size) < src.size // 2)[keep]
    u, v = u[keep], v[keep]
    o = np.argsort(u, kind="stable")
    deg = np.bincount(u, minlength=vid.size)
    off = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    rrow = np.repeat(np.arange(vid.size, dtype=np.int64), deg)
    rot = np.bincount(u[first_half], minlength=vid.size).astype(np.int64)
    return off, v[o], rrow, rot


def rotate(off, nbr, rrow, rot):
    """k_rotate_rows, one entry position p at a time (vectorised): rnbr[p] = nbr[off[x] + (i < b ? a + i : i - b)]."""
    p = np.arange(nbr.size, dtype=np.int64)
    x = rrow
    i, a = p - off[x], rot[x]
    b = off[x + 1] - off[x] - a
    return nbr[off[x] + np.where(i < b, a + i, i - b)]
