#!/usr/bin/env python3
"""bench_components.py — what labelling the weakly connected components (gg_components) costs over LDBC `knows` and over
the synthetic reply forest of scripts/bench_closure.py.

Per workload (default sf10, sf100 and forest):
    variants   gg_components with both values of gg_debug_components' init_mode (when profiles/r17_components_*.json were
               taken, 0 started a vertex under its first smaller out-neighbour and 1 as its own root; the former lost and
               was removed, so the two are one start now), the same call on a second context created with
               GG_CC_SIZE_FOLD=0 (sizes added per lane, never per wave), and gg_reach_closure from one seed of the largest
               component — the nearest earlier way to get one component.  All of them run in alternation, `--runs` rounds
               after one warm-up round; ms per call is a host clock around a call that ends in the library's stream
               synchronisation; the rows stay on the device and are dropped.
    kernels    of one profiled call per gg_components variant (gg_profile_*: cc_init, cc_hook, cc_jump, cc_size, cc_flag,
               cc_rows, cc_reps and the scan), in a round of their own, with the call's jump_launches.
    model      8 E + 12 V * jump_launches + 28 V bytes per call; model_bytes_per_s is that over the summed kernel time.
    sql        (--sql) gg_components(...) inside the compiled reference next to the reference's own UNION recursive CTE
               under an aggregate (tests/components_ref.sql_components), no planner rule on, on datagen.ldbc_knows graphs
               of growing size: the ladder stops before the size at which the statement, quadratic in the giant component,
               is predicted to need more than a minute.  Skipped, and said so, where the reference build or the extension is
               not present.
Whether `parent` (4 V bytes) stays resident in L2 is not measured.
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

CC_KERNELS = ("cc_init", "cc_hook", "cc_jump", "cc_size", "cc_flag", "cc_rows", "cc_reps")


def timed(call):
    t0 = time.perf_counter()
    out = call()
    return out, (time.perf_counter() - t0) * 1e3


def profiled(gg, call):
    gg.profile_reset()
    gg.profile(True)
    out = call()
    gg.profile(False)
    return out, {k: {"launches": v[0], "ms": v[1]} for k, v in gg.profile_get().items()}


def cc_call(gg, csr, init_mode, fetch):
    gg.debug_components(init_mode, 0)
    if not fetch:
        return gg.components(csr, fetch=False)["stats"]
    import ctypes as C

    from duckdb_pgq_amd.gg import CcStats

    st, res = CcStats(), C.c_void_p()  # the rows are made and stay on the device
    gg._chk(gg.lib.gg_components(gg.ctx, csr.handle, C.byref(st), C.byref(res)))
    gg.lib.gg_result_destroy(res)
    return {name: int(getattr(st, name)) for name, _ in CcStats._fields_}


def reach_call(gg, csr, seed):
    res = gg.reach_closure(csr, np.array([seed], np.int64), np.zeros(1, np.uint32))
    rows = res.rows()
    res.close()
    return {"levels": len(rows), "rows": int(sum(rows))}


def load(workload, posts):
    import duckdb_pgq_amd as pkg

    if workload != "forest":
        return pkg.datagen.ldbc(workload)
    from bench_closure import reply_forest

    src, dst, _, n = reply_forest(posts, 100_000, 64, 1000, 7)
    return np.arange(n, dtype=np.int64) * 16 + 1_000_000_007, src, dst


def build(gg, vid, src, dst):
    gg.set_edge_rowid(False)  # the labels need none
    gg.append_vertices(vid)
    gg.append_edges(src, dst)
    return gg.build_csr()


def sql_part(runs, budget_s):
    import duckdb_pgq_amd as pkg
    from oracle import ref_duckdb as R
    from tests import components_ref as K

    if not (R.available() and os.path.exists(R.EXTENSION)):
        return {"available": False, "reason": "reference build / extension not present"}
    out = {"available": True, "budget_s": budget_s, "cases": []}
    graph = "'person', 'p_personid', 'knows', 'k_person1id', 'k_person2id'"
    fn = f"SELECT count(*), sum(size), max(size) FROM gg_components({graph})"
    ref = "SELECT count(*), sum(c), max(c) FROM (" + K.sql_components().replace("count(*)", "count(*) AS c", 1) + ") q"
    V = 500
    while True:
        vid, s, d_ = pkg.datagen.ldbc_knows(V, 8 * V, 17)
        src, dst = np.concatenate([s, d_]), np.concatenate([d_, s])
        d = R.RefDuckDB()
        try:
            d.load_table("person", {"p_personid": vid})
            d.load_table("knows", {"k_person1id": src, "k_person2id": dst})
            d.execute(K.sql_und())
            d.execute(f"LOAD '{R.EXTENSION}'")
            got, want = d.query_text(fn), d.query_text(ref)  # warm-up, and the answers
            f_ms, r_ms = [], []
            for _ in range(runs):  # in alternation
                f_ms.append(timed(lambda: d.query_text(fn))[1])
                r_ms.append(timed(lambda: d.query_text(ref))[1])
        finally:
            d.close()
        case = {"V": V, "edge_rows": int(src.size), "function_ms_median": statistics.median(f_ms), "function_ms_all": f_ms,
                "reference_plan_ms_median": statistics.median(r_ms), "reference_plan_ms_all": r_ms, "equal": got == want,
                "rows_sum_max": list(got[0]), "reference_over_function": statistics.median(r_ms) / statistics.median(f_ms)}
        out["cases"].append(case)
        print("sql V", V, "function %.1f ms, reference %.1f ms" % (case["function_ms_median"], case["reference_plan_ms_median"]),
              file=sys.stderr, flush=True)
        assert got == want, (got, want)
        if case["reference_plan_ms_median"] * 4 > budget_s * 1e3:  # quadratic: twice the vertices, four times the time
            out["largest_within_budget"] = V
            out["next_size_predicted_ms"] = case["reference_plan_ms_median"] * 4
            break
        V *= 2
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="sf10,sf100,forest")
    ap.add_argument("--forest-posts", type=int, default=400_000)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--sql", action="store_true", help="add the SQL ladder to the first workload's output")
    ap.add_argument("--sql-budget-s", type=float, default=60.0)
    ap.add_argument("--out-prefix", default=None, help="e.g. profiles/r17_components_")
    args = ap.parse_args()
    import duckdb_pgq_amd as pkg

    for n_w, workload in enumerate(args.workloads.split(",")):
        vid, src, dst = load(workload, args.forest_posts)
        gg = pkg.GG(0)
        csr = build(gg, vid, src, dst)
        os.environ["GG_CC_SIZE_FOLD"] = "0"  # read when a context is created
        gg_lane = pkg.GG(0)
        del os.environ["GG_CC_SIZE_FOLD"]
        csr_lane = build(gg_lane, vid, src, dst)
        V, E = int(csr.V), int(csr.E)
        first = gg.components(csr)
        seed = int(first["components"][int(np.argmax(first["sizes"]))])  # a member of the largest component
        out = {"metric": "weakly connected components (gg_components)", "workload": workload, "V": V, "E": E,
               "runs": args.runs, "stats": first["stats"], "parent_bytes": 4 * V, "parent_l2_residency": "unmeasured",
               "variants": {}}
        variants = [("init0", lambda: cc_call(gg, csr, 0, True)), ("init1", lambda: cc_call(gg, csr, 1, True)),
                    ("init0,stats_only", lambda: cc_call(gg, csr, 0, False)),
                    ("init0,size_per_lane", lambda: cc_call(gg_lane, csr_lane, 0, True)),
                    ("reach_closure_one_seed", lambda: reach_call(gg, csr, seed))]
        ms = {name: [] for name, _ in variants}
        last = {}
        for r in range(args.runs + 1):  # round 0 warms up every variant
            for name, call in variants:
                last[name], t = timed(call)
                if r:
                    ms[name].append(t)
        for name, call in variants:
            v = {"ms_median": statistics.median(ms[name]), "ms_all": ms[name], "result": last[name]}
            if name != "reach_closure_one_seed":
                ctx = gg_lane if "per_lane" in name else gg
                st, kernels = profiled(ctx, call)  # the kernel times, in a round of their own
                kernel_ms = sum(k["ms"] for k in kernels.values())
                model = 8 * E + 12 * V * st["jump_launches"] + 28 * V
                v.update({"kernels": kernels, "jump_launches": st["jump_launches"], "kernel_ms": kernel_ms,
                          "phases_ms": {"hook": sum(kernels.get(x, {}).get("ms", 0.0) for x in ("cc_init", "cc_hook")),
                                        "jump": kernels.get("cc_jump", {}).get("ms", 0.0),
                                        "size": kernels.get("cc_size", {}).get("ms", 0.0),
                                        "emit": sum(k["ms"] for n, k in kernels.items()
                                                    if n not in ("cc_init", "cc_hook", "cc_jump", "cc_size"))},
                          "model_bytes": model, "model_bytes_per_s": model / (kernel_ms * 1e-3) if kernel_ms > 0 else None})
            out["variants"][name] = v
        print(workload, {n: "%.3f ms" % v["ms_median"] for n, v in out["variants"].items()}, file=sys.stderr, flush=True)
        gg.debug_components(0, 0)
        for c, g in ((csr, gg), (csr_lane, gg_lane)):
            c.close()
            g.close()
        if args.sql and n_w == 0:
            out["sql"] = sql_part(max(1, args.runs // 2), args.sql_budget_s)
        line = json.dumps(out)
        print(line)
        if args.out_prefix:
            path = args.out_prefix + workload.replace(".", "_") + ".json"
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
