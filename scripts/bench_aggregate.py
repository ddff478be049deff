#!/usr/bin/env python3
"""bench_aggregate.py — what count(*) and sum(weight) per start or end vertex of the k-hop walks (gg_khop_aggregate) cost
over LDBC `knows`.

Per workload (default sf10 and sf100), all sources, random int64 weights:
    calls      ms per call (median over `--runs` after a warm-up; the result is left on the device and dropped, nothing is
               fetched) for k = 1, 2, 3, grouped by start and by end, with and without weights, and the kernel times of one
               profiled call (gg_profile_*: agg_pull, agg_pull_long, agg_flag, agg_write, ...).  A call of k hops runs k
               pull passes (k - 1 without weights), so the pass of level h is the difference of the agg_pull times of
               k = h and k = h - 1, reported as pass_ms.
    yardstick  gg_khop_count(3..3) from all sources runs one wc_pull over the reverse rows of the same CSR (16 lanes per
               vertex, u64 counts only): profiled in alternation with the aggregate of k = 3 grouped by end, `--runs`
               times; the ratio of one weighted pass (24-byte states) and of one counting pass (u64) to wc_pull is
               recorded.  No gate.
    long_rows  k = 3 with weights, both groupings, with the long-row route at its default threshold and switched off
               (gg_debug_aggregate_long_row(UINT32_MAX): every row goes to a 16-lane group)
    sql        gg_khop_aggregate(...) inside the compiled reference next to the reference's own hash-aggregate plan of the
               same statement (tests/khop_aggregate_ref.sql_khop_aggregate, the shape of bi-8.sql:41-53), no planner rule
               on; `--sql-hops` (default 1; 2 forms every 2-hop row on the CPU).  Skipped, and said so, where the reference
               build or the extension is not present.
Byte model of one weighted pass at level >= 2: E * (4 + 24) + V * (8 + 24) bytes; model_bytes_per_s is that over the
pass's kernel time.  Where the 24 V bytes of gathered states are served from (L2, Infinity Cache, HBM) is not measured.
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


def pull_ms(kernels):
    return sum(kernels.get(k, {}).get("ms", 0.0) for k in ("agg_pull", "agg_pull_long"))


def one_call(gg, csr, k, group_by, weights):
    agg = gg.khop_aggregate(csr, k, k, group_by, None, weights)
    st = agg.stats
    agg.close()
    return st


def measure(gg, csr, k, group_by, weights, runs):
    call = lambda: one_call(gg, csr, k, group_by, weights)  # noqa: E731
    st = call()  # warm-up: pool blocks, the reverse rows
    ms = [timed(call)[1] for _ in range(runs)]
    kernels = profiled(gg, call)
    return {"k": k, "group_by": group_by, "weights": weights is not None, "groups": st["groups"][k], "walks": st["walks"][k],
            "entries_pulled": st["entries_pulled"], "ms_median": statistics.median(ms), "ms_all": ms,
            "pull_ms": pull_ms(kernels), "kernels": kernels}


def sql_part(pkg, workload, vid, src, dst, weights, hops_list, runs):
    from oracle import ref_duckdb as R
    from tests import khop_aggregate_ref as K

    if not (R.available() and os.path.exists(R.EXTENSION)):
        return {"available": False, "reason": "reference build / extension not present"}
    out = {"available": True, "cases": []}
    d = R.RefDuckDB()
    try:
        d.load_table("person", {"p_personid": vid, "p_score": weights})
        d.load_table("knows", {"k_person1id": src, "k_person2id": dst})
        d.execute(f"LOAD '{R.EXTENSION}'")
        graph = "'person', 'p_personid', 'knows', 'k_person1id', 'k_person2id'"
        for h in hops_list:
            for group_by in K.GROUPS:
                # (count(total): the sums are formed on both sides and none is pruned)
                fn = (f"SELECT count(*), sum(walks), count(total) FROM gg_khop_aggregate({graph}, NULL, {h}, '{group_by}', "
                      f"'p_score')")
                ref = "SELECT count(*), sum(c), count(t) FROM (" + K.sql_khop_aggregate(h, group_by).replace(
                    "count(*), sum(", "count(*) AS c, sum(", 1).replace(") FROM", ") AS t FROM", 1) + ") q"
                got = d.query_text(fn)  # warm-up, and the answer
                f_ms = [timed(lambda: d.query_text(fn))[1] for _ in range(runs)]
                (want, r_ms) = timed(lambda: d.query_text(ref))
                out["cases"].append({"hops": h, "group_by": group_by, "function_ms_median": statistics.median(f_ms),
                                     "function_ms_all": f_ms, "reference_plan_ms": r_ms, "equal": got == want,
                                     "groups_walks_totals": list(got[0]),
                                     "reference_over_function": r_ms / statistics.median(f_ms)})
                assert got == want, (got, want)
    finally:
        d.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="sf10,sf100")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=14)
    ap.add_argument("--sql-hops", default="1")
    ap.add_argument("--no-sql", action="store_true")
    ap.add_argument("--out-prefix", default=None, help="e.g. profiles/r14_aggregate_")
    args = ap.parse_args()
    import duckdb_pgq_amd as pkg

    for workload in args.workloads.split(","):
        vid, src, dst = pkg.datagen.ldbc(workload)
        gg = pkg.GG(0)
        gg.append_vertices(vid)
        gg.append_edges(src, dst)
        csr = gg.build_csr()
        V, E = int(csr.V), int(csr.E)
        v2 = csr.export()[3]
        rng = np.random.RandomState(args.seed)
        w_dense = rng.randint(-(1 << 62), 1 << 62, size=V, dtype=np.int64)  # in vertex-table order
        out = {"metric": "grouped aggregates over walks (gg_khop_aggregate)", "workload": workload, "V": V, "E": E,
               "runs": args.runs, "calls": [], "byte_model_weighted_pass": E * (4 + 24) + V * (8 + 24),
               "gather_table_bytes": 24 * V, "gather_table_residency": "not measured"}
        by = {}
        for group_by in ("start", "end"):
            for weights in (w_dense, None):
                for k in (1, 2, 3):
                    e = measure(gg, csr, k, group_by, weights, args.runs)
                    prev = by.get((group_by, weights is not None, k - 1))
                    e["pass_ms"] = e["pull_ms"] - (prev["pull_ms"] if prev else 0.0)
                    if weights is not None and k >= 2 and e["pass_ms"] > 0:
                        e["model_bytes_per_s"] = out["byte_model_weighted_pass"] / (e["pass_ms"] * 1e-3)
                    by[(group_by, weights is not None, k)] = e
                    out["calls"].append(e)
                    print(workload, group_by, "weights" if weights is not None else "counts", "k", k,
                          "%.3f ms" % e["ms_median"], "pass %.3f ms" % e["pass_ms"], file=sys.stderr, flush=True)
        # the yardstick of one pass: the parent's wc_pull on the same CSR, in alternation
        yard = {"wc_pull_ms": [], "weighted_pass_ms": [], "count_pass_ms": []}
        gg.khop_count(csr, 3, 3)
        for _ in range(args.runs):
            kc = profiled(gg, lambda: gg.khop_count(csr, 3, 3))
            ka = profiled(gg, lambda: one_call(gg, csr, 3, "end", w_dense))
            kn = profiled(gg, lambda: one_call(gg, csr, 3, "end", None))
            yard["wc_pull_ms"].append(kc["wc_pull"]["ms"] / kc["wc_pull"]["launches"])
            # three weighted passes, of which two gather states; two counting passes
            yard["weighted_pass_ms"].append(pull_ms(ka) / 3)
            yard["count_pass_ms"].append(pull_ms(kn) / 2)
        m = {k: statistics.median(v) for k, v in yard.items()}
        yard.update({"weighted_pass_over_wc_pull": m["weighted_pass_ms"] / m["wc_pull_ms"],
                     "count_pass_over_wc_pull": m["count_pass_ms"] / m["wc_pull_ms"]})
        out["yardstick"] = yard
        # the long-row route on and off
        out["long_rows"] = []
        for group_by in ("start", "end"):
            for name, thr in (("default", 0), ("off", NO_LONG_ROWS)):
                gg.debug_aggregate_long_row(thr)
                e = measure(gg, csr, 3, group_by, w_dense, args.runs)
                e["long_row_route"] = name
                out["long_rows"].append(e)
        gg.debug_aggregate_long_row(0)
        csr.close()
        gg.close()
        if args.no_sql:
            out["sql"] = {"available": False, "reason": "--no-sql"}
        else:
            order = np.argsort(vid, kind="stable")  # the weight of vertex id x is w_dense[dense index of x]
            at = np.argsort(v2, kind="stable")
            w_table = np.empty(V, np.int64)
            w_table[order] = w_dense[at]
            out["sql"] = sql_part(pkg, workload, vid, src, dst, w_table, [int(x) for x in args.sql_hops.split(",") if x],
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
