#!/usr/bin/env python3
"""bench_triangles.py — what counting and listing triangle rows (gg_triangles) costs over LDBC `knows`.

Per workload (default sf10 and sf100) and per `order` (0: every closed 3-edge walk, 1: id(a) < id(b) < id(c)):
    count      gg_triangles, count + digest only
    rows       gg_triangles materialising (a, b, c) in HBM, nothing fetched — skipped where the rows would not fit the
               2^32-row limit or `--max-rows`
    edges      gg_triangles_edges: the rows with the rowids (e1, e2, e3) of their edge rows, same CSR, nothing fetched;
               timed ALTERNATING with the ids-only materialisation (one call of each per round), so that both medians
               come from the same run, with the k_tri_write_edges kernel time
each the median wall time over `--runs` calls after a warm-up, with wedges/s, rows/s and the kernels' times from
gg_profile_*.  The first gg_triangles_edges call on a CSR also sorts the forward positions by destination
(csr->rpos_by_src): that one-time cost is reported per workload as `rpos_by_src_build`, apart from the steady state.  Two yardsticks that do not depend on the code under test are recorded next to them:
    khop3      gg_expand_khop(3..3, count) on the same CSR: it expands the same wedges and then all their leaves, where
               the triangle count does one search per wedge
    reference  the compiled reference's own plan of the three-join statement under count(*) (no planner rule), on the
               largest of `--ref-workloads` that finishes within `--ref-limit` seconds (needs oracle/_ref)
Output: one JSON line per workload, also written to <out-prefix><workload>.json.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(call, runs):
    call()  # warm-up: pool blocks, the reverse rows sorted by source
    ms = []
    for _ in range(runs):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), ms


def alternated_ms(call_a, call_b, runs):
    """medians of two calls timed in turns (a, b, a, b, ...) after a warm-up of each: drift hits both alike"""
    call_a()
    call_b()
    a, b = [], []
    for _ in range(runs):
        for call, ms in ((call_a, a), (call_b, b)):
            t0 = time.perf_counter()
            call()
            ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(a), a, statistics.median(b), b


def profiled(gg, call):
    gg.profile_reset()
    gg.profile(True)
    call()
    gg.profile(False)
    return {k: {"launches": v[0], "ms": v[1]} for k, v in gg.profile_get().items()}


def reference_yardstick(pkg, workloads, limit_s):
    from oracle import ref_duckdb as R
    from tests import triangles_ref as T

    if not R.available():
        return {"available": False}
    out = {"available": True, "statement": T.sql_triangles("count(*)", True), "runs": []}
    for w in workloads:
        vid, src, dst = pkg.datagen.ldbc(w)
        d = R.RefDuckDB()
        try:
            d.load_ldbc(vid, src, dst)
            entry = {"workload": w}
            for ordered in (False, True):
                t0 = time.perf_counter()
                n = int(d.execute(T.sql_triangles("count(*)", ordered))[0, 0])
                entry["order%d" % int(ordered)] = {"rows": n, "seconds": time.perf_counter() - t0}
        finally:
            d.close()
        out["runs"].append(entry)
        if max(entry["order0"]["seconds"], entry["order1"]["seconds"]) > limit_s:
            break  # this size is past the limit: the one before it is the yardstick
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="sf10,sf100")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--max-rows", type=int, default=1 << 30, help="materialise only results of at most this many rows")
    ap.add_argument("--ref-workloads", default="sf0.1,sf1,sf10")
    ap.add_argument("--ref-limit", type=float, default=60.0)
    ap.add_argument("--no-khop3", action="store_true")
    ap.add_argument("--out-prefix", default=None, help="e.g. profiles/r11_triangles_")
    args = ap.parse_args()
    import duckdb_pgq_amd as pkg

    ref = reference_yardstick(pkg, [w for w in args.ref_workloads.split(",") if w], args.ref_limit)
    for workload in args.workloads.split(","):
        vid, src, dst = pkg.datagen.ldbc(workload)
        gg = pkg.GG(0)
        gg.append_vertices(vid)
        gg.append_edges(src, dst)
        csr = gg.build_csr()
        out = {"metric": "triangle rows (closed 3-edge walks)", "workload": workload, "V": csr.V, "E": csr.E,
               "runs": args.runs, "orders": {}, "reference_three_join_count": ref}
        def edges_call(order):
            _, res = gg.triangles_edges(csr, ordered=bool(order))
            res.close()

        # the one-time cost of csr->rpos_by_src: the first edges call against the ones after it (the ordered form, the
        # cheaper of the two; rnbr_by_src is there already, so the difference is the position sort alone)
        gg.triangles(csr, ordered=True)
        t0 = time.perf_counter()
        first_kernels = profiled(gg, lambda: edges_call(1))
        first_ms = (time.perf_counter() - t0) * 1e3
        steady, steady_all = median_ms(lambda: edges_call(1), args.runs)
        out["rpos_by_src_build"] = {"bytes": 4 * csr.E, "first_call_ms_profiled": first_ms, "steady_call_ms_median": steady,
                                    "steady_call_ms_all": steady_all, "difference_ms": first_ms - steady,
                                    "kernels_first_call": first_kernels}
        for order in (0, 1):
            st = gg.triangles(csr, ordered=bool(order))
            med, ms = median_ms(lambda: gg.triangles(csr, ordered=bool(order)), args.runs)
            gg.profile_reset()
            gg.profile(True)
            gg.triangles(csr, ordered=bool(order))
            gg.profile(False)
            entry = {"stats": st, "count_ms_median": med, "count_ms_all": ms,
                     "wedges_per_s": st["wedges"] / (med * 1e-3), "rows_per_s": st["rows"] / (med * 1e-3),
                     "kernels_count": {k: {"launches": v[0], "ms": v[1]} for k, v in gg.profile_get().items()}}
            if st["rows"] <= min(args.max_rows, (1 << 32) - 1):
                def rows_call():
                    _, res = gg.triangles(csr, ordered=bool(order), materialise=True)
                    res.close()
                rmed, rms = median_ms(rows_call, args.runs)
                gg.profile_reset()
                gg.profile(True)
                rows_call()
                gg.profile(False)
                entry.update({"rows_ms_median": rmed, "rows_ms_all": rms, "materialised_rows_per_s": st["rows"] / (rmed * 1e-3),
                              "kernels_rows": {k: {"launches": v[0], "ms": v[1]} for k, v in gg.profile_get().items()}})
                emed, ems, imed, ims = alternated_ms(lambda: edges_call(order), rows_call, args.runs)
                kernels = profiled(gg, lambda: edges_call(order))
                entry.update({"edges_ms_median": emed, "edges_ms_all": ems, "ids_only_ms_median_same_run": imed,
                              "ids_only_ms_all_same_run": ims, "edges_over_ids_only": emed / imed,
                              "edge_rows_per_s": st["rows"] / (emed * 1e-3),
                              "k_tri_write_edges_ms": kernels.get("k_tri_write_edges", {}).get("ms"),
                              "kernels_edges": kernels})
            else:
                entry["rows_ms_median"] = None  # too many rows to materialise in one call
            out["orders"]["order%d" % order] = entry
        if not args.no_khop3:
            k3 = gg.expand_khop(csr, 3, 3)
            kmed, kms = median_ms(lambda: gg.expand_khop(csr, 3, 3), max(1, args.runs // 2))
            out["yardstick_khop3_count"] = {"rows": k3["rows"][3], "traversed_edges": k3["traversed_edges"],
                                           "ms_median": kmed, "ms_all": kms,
                                           "triangle_count_order0_over_khop3": out["orders"]["order0"]["count_ms_median"] / kmed}
        line = json.dumps(out)
        print(line)
        if args.out_prefix:
            path = args.out_prefix + workload.replace(".", "_") + ".json"
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(line + "\n")
        csr.close()
        gg.close()


if __name__ == "__main__":
    main()
