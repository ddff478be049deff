#!/usr/bin/env python3
"""bench_paths.py — what the shortest paths cost on top of the 64-source BFS that finds their lengths.

One 64-source batch over LDBC `knows` (default SF100), run to fixpoint, for two target shapes: (a) every vertex as the
target of every source (64 x V pairs), (b) `--sample` sampled vertices (64 x sample pairs).  Per shape, wall time of
    bfs        gg_bfs64, distances left on the device
    pairs      gg_bfs64_pairs (BFS + compaction of the reached rows, nothing fetched): the yardstick
    paths      gg_bfs64_paths with and without edges (BFS + lengths + scan + trace, nothing fetched)
each the median over `--batches` source batches, the path step (paths - bfs) as a multiple of the yardstick's own step
(pairs - bfs) and of the whole yardstick, rows per second of the path step, and the kernels' times from gg_profile_*.
`--lib` loads another build of the library (the lane-group width GG_PATH_LANES is a compile-time constant: the A/B is
one run per build).  Output: one JSON line, also written to --out.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="sf100")
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--sample", type=int, default=10_000)
    ap.add_argument("--max-hops", type=int, default=-1)
    ap.add_argument("--lib", default=None, help="path of another libgg.so build")
    ap.add_argument("--label", default="", help="what this build is (e.g. GG_PATH_LANES=16)")
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
    V = csr.V
    lib, i64p = gg.lib, C.POINTER(C.c_int64)
    batches = [pkg.datagen.pick_sources(vid, 64, 0x5EED, batch=b) for b in range(args.batches)]
    rng = np.random.default_rng(0x9A7)
    shapes = {"every_vertex": vid, f"sample_{args.sample}": vid[rng.choice(V, min(args.sample, V), replace=False)]}

    def timed(call):
        t0 = time.perf_counter()
        rows = call()
        return (time.perf_counter() - t0) * 1e3, rows

    def run_bfs(b):
        gg.bfs64(csr, b, args.max_hops, fetch=False)
        return 0

    def run_pairs(b):
        s, ps = ggmod._i64(b)
        res, n = C.c_void_p(), C.c_uint64()
        gg._chk(lib.gg_bfs64_pairs(gg.ctx, csr.handle, ps, s.size, args.max_hops, None, C.byref(res)))
        gg._chk(lib.gg_result_rows(res, 2, C.byref(n)))
        lib.gg_result_destroy(res)
        return int(n.value)

    def run_paths(b, lane, targets, edges):
        s, ps = ggmod._i64(b)
        res, n = C.c_void_p(), C.c_uint64()
        gg._chk(lib.gg_bfs64_paths(gg.ctx, csr.handle, ps, s.size, args.max_hops, lane.ctypes.data_as(C.POINTER(C.c_uint32)),
                                   targets.ctypes.data_as(i64p), targets.size, 1 if edges else 0, None, C.byref(res)))
        gg._chk(lib.gg_bfs64_paths_rows(res, C.byref(n)))
        lib.gg_result_destroy(res)
        return int(n.value)

    out = {"metric": "shortest-path rows on top of the 64-source BFS", "workload": args.workload, "V": V, "E": csr.E,
           "build": args.label or "default", "batches": args.batches, "max_hops": args.max_hops, "shapes": {}}
    for name, targets in shapes.items():
        lane = np.repeat(np.arange(64, dtype=np.uint32), targets.size)
        tgt = np.ascontiguousarray(np.tile(targets, 64))
        calls = {"bfs": run_bfs, "pairs": run_pairs, "paths_edges": lambda b: run_paths(b, lane, tgt, True),
                 "paths_vertices": lambda b: run_paths(b, lane, tgt, False)}
        for c in calls.values():
            c(batches[0])  # warm-up: pool blocks, reverse CSR
        ms = {k: [] for k in calls}
        rows = {}
        for b in batches:
            for k, c in calls.items():
                t, r = timed(lambda: c(b))
                ms[k].append(t)
                rows[k] = r
        med = {k: statistics.median(v) for k, v in ms.items()}
        # kernel times of the path calls from a profiled pass
        gg.profile_reset()
        gg.profile(True)
        for b in batches:
            run_paths(b, lane, tgt, True)
        gg.profile(False)
        prof = gg.profile_get()
        kern = {k: {"launches": v[0], "ms_per_batch": v[1] / args.batches} for k, v in prof.items()}
        total_kern = sum(v["ms_per_batch"] for v in kern.values())
        step = med["paths_edges"] - med["bfs"]
        yard = med["pairs"] - med["bfs"]
        out["shapes"][name] = {
            "pairs": int(tgt.size), "path_rows_last_batch": rows["paths_edges"], "reached_rows_last_batch": rows["pairs"],
            "ms_per_batch_median": med, "ms_per_batch_all": ms,
            "path_step_ms": step, "path_step_vertices_only_ms": med["paths_vertices"] - med["bfs"],
            "yardstick_pairs_ms": med["pairs"], "yardstick_step_ms": yard,
            "path_step_over_pairs_call": step / med["pairs"], "paths_call_over_pairs_call": med["paths_edges"] / med["pairs"],
            "path_rows_per_s": rows["paths_edges"] / (step * 1e-3) if step > 0 else None,
            "kernels": kern,
            "path_trace_share_of_kernel_time": kern.get("path_trace", {}).get("ms_per_batch", 0.0) / total_kern if total_kern else None,
        }
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    csr.close()
    gg.close()


if __name__ == "__main__":
    main()
