#!/usr/bin/env python3
"""bench_cheapest.py — what the cheapest path costs from 64 sampled sources to every vertex (gg_cheapest64) cost over LDBC
`knows` with weights that are a fixed hash of the edge rowid into 1..100.

Per workload (default sf10 and sf100):
    variants   gg_cheapest64 to the fixpoint with the mask skip on (gather_mode 0) and off (1) and the long-row route at its
               default threshold and switched off (UINT32_MAX); next to them, on the same CSR and sources, gg_bfs64 (the
               unweighted search) and ONE pc_pull pass of gg_khop_pair_counts (k = 1: the same pull over counts instead of
               costs).  All of them run in alternation, `--runs` rounds after one warm-up round; ms per call is a host clock
               around a call that ends in the library's stream synchronisation, the rows left on the device and dropped.
               ms_per_round is that over the call's `rounds` (a round ends in one host synchronisation).
    kernels    of one profiled call per setting (gg_profile_*: cp_pull, cp_pull_long, cp_count, cp_write, ...), in a round
               of their own; pull_ms_per_round is (cp_pull + cp_pull_long) / rounds.
    model      bytes per call from the byte model with the call's own counters: rounds * (E * 12 + V * 16) + rows_gathered *
               (512 + 8) + cells_lowered * 20.  A lowered row is written whole (1 280 B for up to 64 cells) and a row with a
               candidate reads its 512 B of cost; the call reports cells, not rows, so those are left at their lower bound of
               20 B a cell.  model_bytes_per_s is that over the pull kernels' time: a MODEL rate, not measured traffic.
    weights    gg_edge_weights_create once (upload of 8 E bytes, the two sorts of the reverse rows on first use), timed apart.
Where the 512 V bytes of gathered state are served from (L2, Infinity Cache, HBM) is not measured.
Output: one JSON line per workload, also written to <out-prefix><workload>.json (e.g. profiles/r22_cheapest_).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NO_LONG_ROWS = 0xFFFFFFFF
SETTINGS = [("skip,long", 0, 0), ("all,long", 0, 1), ("skip,short", NO_LONG_ROWS, 0), ("all,short", NO_LONG_ROWS, 1)]


def hashed_weights(n):
    """a fixed hash of the rowid into 1..100"""
    r = np.arange(n, dtype=np.uint64)
    return (((r * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(40)) % np.uint64(100)).astype(np.int64) + 1


def timed(call):
    t0 = time.perf_counter()
    out = call()
    return out, (time.perf_counter() - t0) * 1e3


def profiled(gg, call):
    gg.profile_reset()
    gg.profile(True)
    call()
    gg.profile(False)
    return {k: {"launches": v[0], "ms": v[1]} for k, v in gg.profile_get().items()}


def cheapest_call(gg, csr, w, sources, long_row, gather_mode, max_hops=-1):
    gg.debug_cheapest(long_row, gather_mode)
    res = gg.cheapest64(csr, w, sources, max_hops)
    st = dict(res.stats, rows=res.rows())
    res.close()
    return st


def pair_pass_call(gg, csr, sources):
    res = gg.khop_pair_counts(csr, 1, 1, sources)
    st = {"pairs": res.stats["pairs"][1], "rows_gathered": res.stats["rows_gathered"]}
    res.close()
    return st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="sf10,sf100")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=22)
    ap.add_argument("--out-prefix", default=None, help="e.g. profiles/r22_cheapest_")
    args = ap.parse_args()
    import duckdb_pgq_amd as pkg

    for workload in args.workloads.split(","):
        vid, src, dst = pkg.datagen.ldbc(workload)
        gg = pkg.GG(0)
        gg.append_vertices(vid)
        gg.append_edges(src, dst)
        csr = gg.build_csr()
        V, E = int(csr.V), int(csr.E)
        weights = hashed_weights(src.size)
        w, weights_ms = timed(lambda: gg.edge_weights(csr, weights))
        w.close()
        w, weights_again_ms = timed(lambda: gg.edge_weights(csr, weights))  # (the reverse rows by source exist now)
        sources = pkg.datagen.pick_sources(vid, 64, args.seed)
        out = {"metric": "cheapest path costs from 64 sources to every vertex (gg_cheapest64), weights hash(rowid) in 1..100",
               "workload": workload, "V": V, "E": E, "runs": args.runs, "state_bytes": (3 * 512 + 256 + 24) * V,
               "gather_table_bytes": 512 * V, "gather_table_residency": "not measured",
               "edge_weights_create_ms_first": weights_ms, "edge_weights_create_ms_again": weights_again_ms, "variants": {}}
        variants = [(name, (lambda lr=lr, gm=gm: cheapest_call(gg, csr, w, sources, lr, gm))) for name, lr, gm in SETTINGS]
        variants.append(("bfs64", lambda: gg.bfs64(csr, sources, 1 << 20, fetch=False)[1]))
        variants.append(("pair_counts,1 pass", lambda: pair_pass_call(gg, csr, sources)))
        ms = {name: [] for name, _ in variants}
        last = {}
        for r in range(args.runs + 1):  # round 0 warms up every variant
            for name, call in variants:
                res, t = timed(call)
                last[name] = res
                if r:
                    ms[name].append(t)
        for name, lr, gm in SETTINGS:  # the kernel times, in a round of their own
            kernels = profiled(gg, lambda: cheapest_call(gg, csr, w, sources, lr, gm))
            st = last[name]
            pull = sum(kernels.get(x, {}).get("ms", 0.0) for x in ("cp_pull", "cp_pull_long"))
            model = st["rounds"] * (E * 12 + V * 16) + st["rows_gathered"] * 520 + st["cells_lowered"] * 20
            med = statistics.median(ms[name])
            out["variants"][name] = {
                "ms_median": med, "ms_all": ms[name], "ms_per_round": med / max(1, st["rounds"]), **st, "kernels": kernels,
                "pull_ms_per_round": pull / max(1, st["rounds"]), "model_bytes": model,
                "model_bytes_per_s": model / (pull * 1e-3) if pull > 0 else None}
        gg.debug_cheapest(0, 0)
        for name in ("bfs64", "pair_counts,1 pass"):
            out["variants"][name] = {"ms_median": statistics.median(ms[name]), "ms_all": ms[name], **last[name]}
        kernels = profiled(gg, lambda: pair_pass_call(gg, csr, sources))
        out["variants"]["pair_counts,1 pass"]["kernels"] = kernels
        print(workload, {n: "%.3f ms" % v["ms_median"] for n, v in out["variants"].items()}, file=sys.stderr, flush=True)
        w.close()
        csr.close()
        gg.close()
        line = json.dumps(out)
        print(line)
        if args.out_prefix:
            path = args.out_prefix + workload.replace(".", "_") + ".json"
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
