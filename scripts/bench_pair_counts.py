#!/usr/bin/env python3
"""bench_pair_counts.py — what count(*) per (source, end vertex) pair of the k-hop walks (gg_khop_pair_counts) costs over
LDBC `knows`, 64 sampled sources a call.

Per workload (default sf10 and sf100) and k = 2, 3:
    variants   the four settings of gg_debug_pair_counts — the mask skip on (gather_mode 0) and off (1), the long-row route
               at its default threshold and switched off (UINT32_MAX) — and the route the library offered before: the walk
               rows gg_expand_khop_result materialises from the same sources, drained over PCIe completely and grouped
               with numpy.  All of them run in alternation, `--runs` rounds after one warm-up round; ms per call is a
               host clock around a call that ends in the library's stream synchronisation (the pair rows stay on the
               device and are dropped; the walk rows are fetched, that being the point).  The walk-row route is skipped,
               and said so, where gg_khop_count says it would form more than `--max-walk-rows` rows.
    kernels    of one profiled call per setting (gg_profile_*: pc_pull, pc_pull_long, pc_count, pc_write, ...), in a
               round of their own; pull_ms_per_pass is (pc_pull + pc_pull_long) / k.
    model      bytes per call from the byte model with the call's own rows_gathered, k * (E * 12 + V * 16) +
               rows_gathered * 512; the 512 B per state row written are left out (the call does not report how many rows
               it wrote), so the model is a lower bound; model_bytes_per_s is that over the pull kernels' time.
    sql        (sf10 only unless --sql-workloads says otherwise) gg_khop_pair_counts(...) inside the compiled reference next
               to the reference's own hash-aggregate plan of the same statement
               (tests/khop_pair_counts_ref.sql_pair_counts), no planner rule on.  Skipped, and said so, where the
               reference build or the extension is not present.
Where the 512 V bytes of gathered state are served from (L2, Infinity Cache, HBM) is not measured.
Output: one JSON line per workload, also written to <out-prefix><workload>.json.
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


def pair_call(gg, csr, k, sources, long_row, gather_mode):
    gg.debug_pair_counts(long_row, gather_mode)
    res = gg.khop_pair_counts(csr, k, k, sources)
    st = res.stats
    res.close()
    return st


def walk_rows_call(gg, csr, k, sources, piece=1 << 20):
    """the earlier route: every k-hop walk row from the sources over PCIe, then the group-by on the host"""
    import ctypes as C

    table = gg.expand_khop_result(csr, k, sources)
    try:
        n = table.rows(k)
        out = np.empty((k + 1, max(n, 1)), np.int64)
        i64p = C.POINTER(C.c_int64)
        got = C.c_uint32()
        for o in range(0, n, piece):
            ptrs = (i64p * (k + 1))(*[out[c, o:].ctypes.data_as(i64p) for c in range(k + 1)])
            gg._chk(gg.lib.gg_result_fetch(table.handle, k, o, min(piece, n - o), ptrs, C.byref(got)))
    finally:
        table.close()
    pairs = np.unique(np.stack([out[0, :n], out[k, :n]], axis=1), axis=0, return_counts=True)
    return {"walk_rows": int(n), "pairs": int(pairs[1].size)}


def sql_part(workload, vid, src, dst, sources, hops_list, runs):
    from oracle import ref_duckdb as R
    from tests import khop_pair_counts_ref as P

    if not (R.available() and os.path.exists(R.EXTENSION)):
        return {"available": False, "reason": "reference build / extension not present"}
    out = {"available": True, "cases": []}
    d = R.RefDuckDB()
    try:
        d.load_table("person", {"p_personid": vid})
        d.load_table("knows", {"k_person1id": src, "k_person2id": dst})
        d.execute(f"LOAD '{R.EXTENSION}'")
        graph = "'person', 'p_personid', 'knows', 'k_person1id', 'k_person2id'"
        in_list = ", ".join(str(int(s)) for s in sources)
        for h in hops_list:
            fn = (f"SELECT count(*), sum(walks) FROM gg_khop_pair_counts({graph}, "
                  f"'SELECT p_personid FROM person WHERE p_personid IN ({in_list})', NULL, {h})")
            ref = "SELECT count(*), sum(c) FROM (" + P.sql_pair_counts(h, sources).replace("count(*)", "count(*) AS c", 1) + ") q"
            got = d.query_text(fn)  # warm-up, and the answer
            want = d.query_text(ref)
            f_ms, r_ms = [], []
            for _ in range(runs):  # in alternation
                f_ms.append(timed(lambda: d.query_text(fn))[1])
                r_ms.append(timed(lambda: d.query_text(ref))[1])
            out["cases"].append({"hops": h, "function_ms_median": statistics.median(f_ms), "function_ms_all": f_ms,
                                 "reference_plan_ms_median": statistics.median(r_ms), "reference_plan_ms_all": r_ms,
                                 "equal": got == want, "pairs_walks": list(got[0]),
                                 "reference_over_function": statistics.median(r_ms) / statistics.median(f_ms)})
            assert got == want, (got, want)
    finally:
        d.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="sf10,sf100")
    ap.add_argument("--hops", default="2,3")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=16)
    ap.add_argument("--max-walk-rows", type=int, default=100_000_000)
    ap.add_argument("--sql-workloads", default="sf10")
    ap.add_argument("--sql-hops", default="2")
    ap.add_argument("--no-sql", action="store_true")
    ap.add_argument("--out-prefix", default=None, help="e.g. profiles/r16_pair_counts_")
    args = ap.parse_args()
    import duckdb_pgq_amd as pkg

    hops = [int(x) for x in args.hops.split(",") if x]
    for workload in args.workloads.split(","):
        vid, src, dst = pkg.datagen.ldbc(workload)
        gg = pkg.GG(0)
        gg.append_vertices(vid)
        gg.append_edges(src, dst)
        csr = gg.build_csr()
        V, E = int(csr.V), int(csr.E)
        sources = pkg.datagen.pick_sources(vid, 64, args.seed)
        out = {"metric": "walks per (source, end vertex) pair, 64 sources a call (gg_khop_pair_counts)", "workload": workload,
               "V": V, "E": E, "runs": args.runs, "state_bytes": 2 * 512 * V, "gather_table_bytes": 512 * V,
               "gather_table_residency": "not measured", "cases": []}
        for k in hops:
            walk_rows = int(gg.khop_count(csr, k, k, sources)[k])
            variants = [(name, (lambda lr=lr, gm=gm: pair_call(gg, csr, k, sources, lr, gm))) for name, lr, gm in SETTINGS]
            if walk_rows <= args.max_walk_rows:
                variants.append(("walk_rows+numpy", lambda: walk_rows_call(gg, csr, k, sources)))
            ms = {name: [] for name, _ in variants}
            last = {}
            for r in range(args.runs + 1):  # round 0 warms up every variant
                for name, call in variants:
                    res, t = timed(call)
                    last[name] = res
                    if r:
                        ms[name].append(t)
            case = {"k": k, "walk_rows": walk_rows, "variants": {}}
            if walk_rows > args.max_walk_rows:
                case["walk_rows+numpy"] = f"skipped: {walk_rows} walk rows exceed --max-walk-rows"
            for name, lr, gm in SETTINGS:  # the kernel times, in a round of their own
                kernels = profiled(gg, lambda: pair_call(gg, csr, k, sources, lr, gm))
                st = last[name]
                pull = sum(kernels.get(x, {}).get("ms", 0.0) for x in ("pc_pull", "pc_pull_long"))
                model = k * (E * 12 + V * 16) + st["rows_gathered"] * 512
                case["variants"][name] = {
                    "ms_median": statistics.median(ms[name]), "ms_all": ms[name], "pairs": st["pairs"][k],
                    "walks": st["walks"][k], "entries_pulled": st["entries_pulled"], "rows_gathered": st["rows_gathered"],
                    "kernels": kernels, "pull_ms_per_pass": pull / k, "model_bytes": model,
                    "model_bytes_per_s": model / (pull * 1e-3) if pull > 0 else None}
            if "walk_rows+numpy" in ms:
                case["variants"]["walk_rows+numpy"] = {"ms_median": statistics.median(ms["walk_rows+numpy"]),
                                                       "ms_all": ms["walk_rows+numpy"], **last["walk_rows+numpy"]}
                if np.unique(sources).size == sources.size:  # distinct sources: an id pair is a (lane, vertex) pair
                    assert last["walk_rows+numpy"]["pairs"] == last["skip,long"]["pairs"][k]
            out["cases"].append(case)
            print(workload, "k", k, {n: "%.3f ms" % v["ms_median"] for n, v in case["variants"].items()}, file=sys.stderr,
                  flush=True)
        gg.debug_pair_counts(0, 0)
        csr.close()
        gg.close()
        if args.no_sql or workload not in args.sql_workloads.split(","):
            out["sql"] = {"available": False, "reason": "not asked for on this workload"}
        else:
            out["sql"] = sql_part(workload, vid, src, dst, sources, [int(x) for x in args.sql_hops.split(",") if x],
                                  max(1, args.runs // 2))
        line = json.dumps(out)
        print(line)
        if args.out_prefix:
            path = args.out_prefix + workload.replace(".", "_") + ".json"
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
