#!/usr/bin/env python3
"""bench_cheapest_paths.py — what the cheapest paths themselves (gg_cheapest64_paths) cost on top of the rounds that find
their costs (gg_cheapest64), over LDBC `knows` with bench_cheapest.py's weights: a fixed hash of the edge rowid into 1..100.

One 64-source batch per round, `--batches` batches of sampled sources, for two target shapes: (a) every vertex as the
target of every source (64 x V pairs), (b) `--sample` sampled vertices (64 x sample pairs).  Per shape, in alternation:
    cheapest        gg_cheapest64 to the fixpoint, the rows left on the device and dropped: the rounds alone
    paths_edges     gg_cheapest64_paths with the edge column (rounds + lengths + scans + pair table + trace)
    paths_vertices  the same without the edge column
    bfs_paths       gg_bfs64_paths on the same pairs: the yardstick for a trace step (unweighted, one byte a cell)
ms per call is a host clock around a call that ends in the library's stream synchronisation, the median over the batches
after one warm-up call each; trace_step_ms = paths_edges - cheapest is the trace's share.  Kernel times come from
gg_profile_* in a pass of their own (cpp_len, cpp_pairs, cpp_trace next to cp_pull ...).
model_bytes: entries_scanned x (4 B entry + 8 B weight + 64 B line of cost) + per step 64 B line of hops + 4 B rpos + 8 B
rowid + per row 36 B.  model_bytes_per_s is that over cpp_trace's time: a MODEL rate, not measured traffic.
`--lib` loads another build of the library: the lane-group width GG_CPP_LANES is a compile-time constant, so the 8 / 16 / 64
comparison is one run per build (`--label` names it), all in one session.  Output: one JSON line, also written to --out
(e.g. profiles/r23_cheapest_paths_sf10_l16.json).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def hashed_weights(n):
    """a fixed hash of the rowid into 1..100 (scripts/bench_cheapest.py)"""
    r = np.arange(n, dtype=np.uint64)
    return (((r * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(40)) % np.uint64(100)).astype(np.int64) + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="sf10")
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--sample", type=int, default=10_000)
    ap.add_argument("--lib", default=None, help="path of another libgg.so build")
    ap.add_argument("--label", default="", help="what this build is (e.g. GG_CPP_LANES=16)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import duckdb_pgq_amd as pkg
    from duckdb_pgq_amd import gg as ggmod

    if args.lib:
        ggmod._lib = ggmod.load_library(args.lib)
    vid, src, dst = pkg.datagen.ldbc(args.workload)
    gg = pkg.GG(0)
    gg.append_vertices(vid)
    gg.append_edges(src, dst)
    csr = gg.build_csr()
    V, E = int(csr.V), int(csr.E)
    w = gg.edge_weights(csr, hashed_weights(src.size))
    lib, i64p, u32p = gg.lib, C.POINTER(C.c_int64), C.POINTER(C.c_uint32)
    batches = [pkg.datagen.pick_sources(vid, 64, 0x5EED, batch=b) for b in range(args.batches)]
    rng = np.random.default_rng(0x9A7)
    shapes = {"every_vertex": vid, f"sample_{args.sample}": vid[rng.choice(V, min(args.sample, V), replace=False)]}

    def timed(call):
        t0 = time.perf_counter()
        st = call()
        return (time.perf_counter() - t0) * 1e3, st

    def run_cheapest(b):
        return gg.cheapest64(csr, w, b, fetch=False).stats

    def run_paths(b, lane, targets, edges):
        s, ps = ggmod._i64(b)
        st, res = ggmod.CheapestPathsStats(), C.c_void_p()
        gg._chk(lib.gg_cheapest64_paths(gg.ctx, csr.handle, w.handle, ps, s.size, lane.ctypes.data_as(u32p),
                                        targets.ctypes.data_as(i64p), targets.size, 1 if edges else 0, C.byref(st),
                                        C.byref(res)))
        lib.gg_result_destroy(res)
        return {"rounds": int(st.search.rounds), "pairs_reached": int(st.pairs_reached),
                "pairs_saturated": int(st.pairs_saturated), "rows": int(st.rows), "entries_scanned": int(st.entries_scanned)}

    def run_bfs_paths(b, lane, targets):
        s, ps = ggmod._i64(b)
        res, n = C.c_void_p(), C.c_uint64()
        gg._chk(lib.gg_bfs64_paths(gg.ctx, csr.handle, ps, s.size, -1, lane.ctypes.data_as(u32p),
                                   targets.ctypes.data_as(i64p), targets.size, 1, None, C.byref(res)))
        gg._chk(lib.gg_bfs64_paths_rows(res, C.byref(n)))
        lib.gg_result_destroy(res)
        return {"rows": int(n.value)}

    out = {"metric": "cheapest-path rows on top of the 64-source rounds (gg_cheapest64_paths), weights hash(rowid) in 1..100",
           "workload": args.workload, "V": V, "E": E, "build": args.label or "default", "batches": args.batches, "shapes": {}}
    for name, targets in shapes.items():
        lane = np.repeat(np.arange(64, dtype=np.uint32), targets.size)
        tgt = np.ascontiguousarray(np.tile(targets, 64))
        calls = {"cheapest": run_cheapest, "paths_edges": lambda b: run_paths(b, lane, tgt, True),
                 "paths_vertices": lambda b: run_paths(b, lane, tgt, False), "bfs_paths": lambda b: run_bfs_paths(b, lane, tgt)}
        for c in calls.values():
            c(batches[0])  # warm-up: pool blocks, code objects
        ms = {k: [] for k in calls}
        last = {}
        for b in batches:  # in alternation: one call of each per batch
            for k, c in calls.items():
                t, st = timed(lambda: c(b))
                ms[k].append(t)
                last[k] = st
        med = {k: statistics.median(v) for k, v in ms.items()}
        kern = {}
        for k in ("paths_edges", "bfs_paths"):  # kernel times, in passes of their own
            gg.profile_reset()
            gg.profile(True)
            for b in batches:
                calls[k](b)
            gg.profile(False)
            kern[k] = {n: {"launches": v[0], "ms_per_batch": v[1] / args.batches} for n, v in gg.profile_get().items()}
        st = last["paths_edges"]
        steps = st["rows"] - (st["pairs_reached"] - st["pairs_saturated"])
        model = st["entries_scanned"] * 76 + steps * 76 + st["rows"] * 36
        trace_ms = kern["paths_edges"].get("cpp_trace", {}).get("ms_per_batch", 0.0)
        out["shapes"][name] = {
            "pairs": int(tgt.size), "last_batch": st, "bfs_path_rows_last_batch": last["bfs_paths"]["rows"],
            "ms_per_batch_median": med, "ms_per_batch_all": ms,
            "trace_step_ms": med["paths_edges"] - med["cheapest"],
            "trace_step_vertices_only_ms": med["paths_vertices"] - med["cheapest"],
            "trace_share_of_call": (med["paths_edges"] - med["cheapest"]) / med["paths_edges"] if med["paths_edges"] else None,
            "kernels": kern, "cpp_trace_ms_per_batch": trace_ms,
            "bfs_path_trace_ms_per_batch": kern["bfs_paths"].get("path_trace", {}).get("ms_per_batch", 0.0),
            "entries_per_step": st["entries_scanned"] / steps if steps else None,
            "model_bytes_last_batch": model, "model_bytes_per_s": model / (trace_ms * 1e-3) if trace_ms > 0 else None}
        print(name, {k: "%.3f ms" % v for k, v in med.items()}, "cpp_trace %.3f ms" % trace_ms, file=sys.stderr, flush=True)
    w.close()
    csr.close()
    gg.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
