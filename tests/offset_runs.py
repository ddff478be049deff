"""The numpy model of how k_expand_mid2 stages a tile from the reverse offsets (gg_khop.hip: k_mid_tile_rows
and mid_stage_offsets), and the khop(1, 2) figures of a range of middle vertices computed through it.  A tile is MT = 768
consecutive reverse-CSR entries [p0, p1); the model restates, step by step and with the kernels' own shapes (15 probes a
search round, XT = 256 rows a window chunk, one 64-bit word of run starts per 64 tile positions):
  1. the 16-way search for the row that holds p0 (the 64-way form of gg_internal.h: wave_find_row, which the row-index
     kernel of gg_csr.hip uses, is the same search with 64 probes a round),
  2. the walk over the window in chunks and the run table (start, out-row, out-degree, middle vertex) it compacts,
  3. the mask of run starts, and an entry's run as a population count over it.
Used by tests/test_offset_runs_cpu.py (against np.repeat and the C oracle) and by the GPU tests of the kernel."""
import numpy as np

from tests.edge_filter_ref import digest_dense_rows

MT, XT, WORDS = 768, 256, 12
M32 = 0xFFFFFFFF


def popcount64(w):
    w = np.ascontiguousarray(w, np.uint64)
    return np.unpackbits(w.view(np.uint8).reshape(w.shape + (8,)), axis=-1).sum(axis=-1).astype(np.int64)


def find_row(roff, V, p, ways=16):
    """The last x with roff[x] <= p (p < roff[V]): `ways` - 1 live probes a round over [lo, lo + n)."""
    lo, n, rounds = 0, V, 0
    lanes = np.arange(1, ways + 1, dtype=np.int64)
    while n > 1:
        step = (n + ways - 1) // ways
        live = lanes * step < n
        k = np.where(live, lo + lanes * step, 0)
        le = live & (roff[k] <= p)
        c = int(le.sum())
        assert le[:c].all()  # the offsets ascend: the lanes that say yes are a prefix
        lo += c * step
        n = min(step, n - c * step)
        rounds += 1
    return lo, rounds


def stage_tile(off, roff, V, p0, p1):
    """The run table and start mask of the tile [p0, p1), and the row of every entry of it by population count."""
    n = p1 - p0
    assert 0 < n <= MT
    x0, rounds = find_row(roff, V, p0)
    run, rst, rdout, run_x = [], [], [], []
    mask = np.zeros(WORDS, np.uint64)
    rows_last, chunks, xc = 0, 0, x0
    while True:
        x = xc + np.arange(XT, dtype=np.int64)
        inside = x < V
        xs = np.where(inside, x, 0)
        a = np.where(inside, roff[xs], 0)
        b = np.where(inside, roff[xs + 1], 0)
        is_run = (b > a) & (a < p1)
        for t in np.flatnonzero(is_run):  # compaction keeps the rows in order: so are the starts
            s, end = max(int(a[t]), p0) - p0, min(int(b[t]), p1) - p0
            dout = int(off[x[t] + 1] - off[x[t]])
            run.append(s), rst.append(int(off[x[t]])), rdout.append(dout), run_x.append(int(x[t]))
            mask[s >> 6] |= np.uint64(1) << np.uint64(s & 63)
            rows_last += (end - s) * dout
        chunks += 1
        more = bool(inside[-1]) and int(x[-1]) + 1 < V and int(b[-1]) < p1
        if not more:
            break
        xc += XT
    run.append(n)  # the end sentinel
    cnt = popcount64(mask)
    excl = np.cumsum(cnt) - cnt
    idx = np.arange(n, dtype=np.int64)
    le = (np.uint64(2) << (idx & 63).astype(np.uint64)) - np.uint64(1)  # bits 0 .. lane (2 << 63 wraps to 0: all ones)
    r = excl[idx >> 6] + popcount64(mask[idx >> 6] & le) - 1
    return {"x0": x0, "rounds": rounds, "chunks": chunks, "run": np.array(run), "rst": np.array(rst),
            "rdout": np.array(rdout), "run_x": np.array(run_x), "mask": mask, "entry_run": r,
            "entry_x": np.array(run_x, np.int64)[r], "rows_last": rows_last}


def entry_rows(off, roff, V, lo=0, hi=None):
    """The row of every reverse entry of the middle vertices [lo, hi), tile by tile through stage_tile."""
    hi = V if hi is None else hi
    fbase, M = int(roff[lo]), int(roff[hi] - roff[lo])
    tiles = [stage_tile(off, roff, V, fbase + t, fbase + min(t + MT, M)) for t in range(0, M, MT)]
    x = np.concatenate([t["entry_x"] for t in tiles]) if tiles else np.zeros(0, np.int64)
    return x, tiles


def khop12(off, nbr, roff, in_rows, V, lo=0, hi=None, block=1 << 20):
    """(rows_1, rows_2, digest_1, digest_2) of the walks u -> x -> w with x in [lo, hi), as the kernel forms them: u
    from the in-rows, x from the staged tiles, w from x's out-row.  (DESIGN.md "Row digest", vectorised.)"""
    hi = V if hi is None else hi
    x, tiles = entry_rows(off, roff, V, lo, hi)
    fbase = int(roff[lo])
    u = np.asarray(in_rows[fbase:fbase + x.size], np.int64)
    d1 = digest_dense_rows(np.stack([u, x], axis=1)) if x.size else 0
    deg = (off[x + 1] - off[x]).astype(np.int64)
    assert int(deg.sum()) == sum(t["rows_last"] for t in tiles)  # the count per run equals the count per entry
    rows2, d2 = 0, 0
    cs = np.cumsum(deg)
    i = 0
    while i < x.size:  # blocks of entries with about `block` 2-hop rows each (one entry of a hub may exceed it)
        j = max(i + 1, int(np.searchsorted(cs, (cs[i - 1] if i else 0) + block, side="right")))
        dg = deg[i:j]
        tot = int(dg.sum())
        if tot:
            e = np.repeat(np.arange(dg.size), dg)
            k = np.arange(tot) - np.repeat(np.cumsum(dg) - dg, dg)
            w = np.asarray(nbr, np.int64)[off[x[i:j]][e] + k]
            d2 = (d2 + digest_dense_rows(np.stack([u[i:j][e], x[i:j][e], w], axis=1))) & M32
            rows2 += tot
        i = j
    return x.size, rows2, d1, d2


# ---- the tables: the smallest at which each part of the indexing can go wrong ------------------------------------
EDGE_COUNTS = (1, 767, 768, 769, 2 * 768, 3 * 768 + 5)
STAR_DEGREE = 4 * 768 + 3
GAP = 2 * XT + 88  # consecutive isolated vertices: more than two window chunks


def _ids(V):
    return np.arange(V, dtype=np.int64) * 3 + 5  # ascending: the dense index of a vertex is its position


def multigraph(E, mirror):
    """E rows over few vertices: self-loops and duplicate rows are certain.  mirror: row i + E // 2 mirrors row i (an
    odd E leaves one row on its own, which keeps the build from deriving)."""
    from tests.test_gpu_derived_reverse import mirrored

    rng = np.random.default_rng(E * 2 + int(mirror))
    vid = _ids(max(3, E // 5))
    if mirror:
        return (vid,) + mirrored(vid, E, rng)
    return vid, vid[rng.integers(0, vid.size, E)], vid[rng.integers(0, vid.size, E)]


def star():
    """A mirrored star whose centre (dense index MT, behind MT leaves of one reverse entry each) has STAR_DEGREE
    entries: its row starts exactly where a tile starts, whole tiles lie inside it, and every tile behind it ends on a
    row boundary."""
    vid = _ids(STAR_DEGREE + 1)
    hub, leaves = vid[MT], np.delete(vid, MT)
    s, d = np.full(STAR_DEGREE, hub, np.int64), leaves
    return vid, np.concatenate([s, d]), np.concatenate([d, s])


def gaps(mirror=True):
    """GAP isolated vertices at the start, in the middle and at the end of the vertex range; 40 connected ones between."""
    from tests.test_gpu_derived_reverse import mirrored

    rng = np.random.default_rng(77)
    vid = _ids(3 * GAP + 80)
    live = np.concatenate([vid[GAP:GAP + 40], vid[2 * GAP + 40:2 * GAP + 80]])
    if mirror:
        return (vid,) + mirrored(live, 2000, rng)
    return vid, live[rng.integers(0, 80, 2000)], live[rng.integers(0, 80, 2000)]


def tables():
    """name -> (vid, src, dst)"""
    out = {}
    for E in EDGE_COUNTS:
        out[f"plain_{E}"] = multigraph(E, False)
        out[f"mirrored_{E}"] = multigraph(E, True)
        if E % 2:
            out[f"mirrored_{2 * E}"] = multigraph(2 * E, True)  # both halves of E rows: this one derives
    out["star"] = star()
    out["gaps_mirrored"] = gaps(True)
    out["gaps_plain"] = gaps(False)
    return out
