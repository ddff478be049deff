#!/usr/bin/env python3
"""bench_all_paths.py — what counting and listing ALL shortest paths costs on top of the 64-source BFS.

One 64-source batch over LDBC `knows` (default SF100), run to fixpoint, for two target shapes: (a) every vertex as the
target of every source (64 x V pairs), (b) `--sample` sampled vertices.  Per shape, wall time of calls that fetch nothing:
    bfs          gg_bfs64, distances left on the device
    count        gg_bfs64_all_paths, materialise = 0 (BFS + count passes + the pair table)
    rows_1/16/0  gg_bfs64_all_paths materialised with path_limit 1 / 16 / none — only where the call's own count says the
                 rows fit under 2^32 (the others are listed under "skipped" with their row count)
    paths        gg_bfs64_paths on the same pairs, alternated with rows_1: the yardstick of the unranking
each the median over `--batches` source batches; the kernels' times from gg_profile_*, per count pass too; the count
passes' bytes/s against the byte model of csrc/gg_all_paths.hip with the call's own sigma_entries / sigma_gathered; and
gg_khop_pair_counts' pc_pull on the same CSR and sources in the same run, the yardstick of a count pass.
Output: one JSON line, also written to --out (profiles/r19_all_paths_<workload>.json).
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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import duckdb_pgq_amd as pkg
    from duckdb_pgq_amd import gg as ggmod

    vid, src, dst = pkg.datagen.ldbc(args.workload)
    gg = pkg.GG(0)
    gg.append_vertices(vid)
    gg.append_edges(src, dst)
    csr = gg.build_csr()
    V = csr.V
    batches = [pkg.datagen.pick_sources(vid, 64, 0x5EED, batch=b) for b in range(args.batches)]
    rng = np.random.default_rng(0x9A7)
    shapes = {"every_vertex": vid, f"sample_{args.sample}": vid[rng.choice(V, min(args.sample, V), replace=False)]}

    def timed(call):
        t0 = time.perf_counter()
        r = call()
        return (time.perf_counter() - t0) * 1e3, r

    def kernels(call):
        gg.profile_reset()
        gg.profile(True)
        for b in batches:
            call(b)
        gg.profile(False)
        return {k: {"launches_per_batch": v[0] / args.batches, "ms_per_batch": v[1] / args.batches}
                for k, v in gg.profile_get().items()}

    out = {"metric": "all shortest paths and their number on top of the 64-source BFS", "workload": args.workload, "V": V,
           "E": csr.E, "batches": args.batches, "max_hops": args.max_hops, "shapes": {}}
    for name, targets in shapes.items():
        lane = np.repeat(np.arange(64, dtype=np.uint32), targets.size)
        tgt = np.ascontiguousarray(np.tile(targets, 64))

        def all_paths(b, limit, materialise):
            return gg.bfs64_all_paths(csr, b, lane, tgt, args.max_hops, limit, True, materialise, fetch=False)

        def run_paths(b):
            s, ps = ggmod._i64(b)
            res, n = C.c_void_p(), C.c_uint64()
            gg._chk(gg.lib.gg_bfs64_paths(gg.ctx, csr.handle, ps, s.size, args.max_hops,
                                          lane.ctypes.data_as(C.POINTER(C.c_uint32)), tgt.ctypes.data_as(C.POINTER(C.c_int64)),
                                          tgt.size, 1, None, C.byref(res)))
            gg._chk(gg.lib.gg_bfs64_paths_rows(res, C.byref(n)))
            gg.lib.gg_result_destroy(res)
            return int(n.value)

        calls = {"bfs": lambda b: gg.bfs64(csr, b, args.max_hops, fetch=False)[1],
                 "count": lambda b: all_paths(b, 0, False)}
        fits, skipped = {}, {}
        for limit in (1, 16, 0):  # does every batch fit under 2^32 kept paths and rows at this limit?
            worst = max((all_paths(b, limit, False) for b in batches), key=lambda st: st["rows"])
            if worst["rows"] < 1 << 32 and worst["paths_kept"] < 1 << 32:
                fits[limit] = worst
                calls[f"rows_{limit}"] = lambda b, limit=limit: all_paths(b, limit, True)
            else:
                skipped[f"rows_{limit}"] = {"paths_kept": worst["paths_kept"], "rows": worst["rows"]}
        calls["paths"] = run_paths
        for c in calls.values():
            c(batches[0])  # warm-up: pool blocks, the reverse rows by source and their positions
        ms = {k: [] for k in calls}
        last = {}
        for b in batches:
            for k, c in calls.items():  # (rows_1 and paths alternate inside this loop)
                t, r = timed(lambda: c(b))
                ms[k].append(t)
                last[k] = r
        med = {k: statistics.median(v) for k, v in ms.items()}
        kern = {k: kernels(c) for k, c in calls.items() if k != "bfs"}
        st = last["count"]
        levels = st["bfs"]["levels"]
        count_ms = kern["count"].get("ap_count", {}).get("ms_per_batch", 0.0)
        # byte model of a count pass (csrc/gg_all_paths.hip), one-byte cells: every distance row + per entry 4 B and one
        # 64-byte distance row + 512 B per gathered entry; the 512-byte stores are left out (at most one per reached pair)
        model_bytes = levels * V * 64 + st["sigma_entries"] * (4 + 64) + st["sigma_gathered"] * 512
        pc = kernels(lambda b: gg.khop_pair_counts(csr, 3, 3, b, fetch=False))
        out["shapes"][name] = {
            "pairs": int(tgt.size), "stats_last_batch": st, "ms_per_batch_median": med, "ms_per_batch_all": ms,
            "count_step_ms": med["count"] - med["bfs"], "fits": fits, "skipped": skipped,
            "rows_1_over_paths_call": med["rows_1"] / med["paths"] if "rows_1" in med else None,
            "kernels": kern, "count_passes_model_bytes": model_bytes,
            "count_passes_GBps": model_bytes / (count_ms * 1e-3) / 1e9 if count_ms else None,
            "count_pass_ms": count_ms / levels if levels else None,
            "yardstick_pc_pull": pc.get("pc_pull"), "yardstick_kernels": pc,
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
