#!/usr/bin/env python3
"""bench_aggregate_top.py — what the best n groups of a walk aggregate cost when they are ordered on the device
(gg_khop_aggregate_top) and when every group is drained and ordered on the host, over LDBC `knows`.

Per workload (default sf10 and sf100): k = 2, grouped by start, random int64 weights, ORDER BY total DESC, id, and
n in {100, 1024, 65536, all}:
    device     ms per call of gg_khop_aggregate_top + the fetch of its n rows (median over `--runs` after a warm-up), the
               kernel times of one profiled call by profile name (top_hist, top_pick, top_compact, top_count, top_place,
               top_sort_lds, top_chunk, radix_*, top_gather, ...) and the call's stats
    yardstick  what the library offered before for the same answer: fetch every group into gg_host_alloc memory
               (gg_khop_aggregate_fetch, four columns), numpy.lexsort on (hi, lo, id), slice n.  Both sides are timed in
               alternation in the same process, on the same resident aggregate; the rows are compared once.
    sql        gg_khop_aggregate_top(...) inside the compiled reference next to the reference's own ORDER BY ... LIMIT n
               above its hash-aggregate plan (tests/khop_aggregate_top_ref.sql_khop_aggregate_top), `--sql-hops` (default
               1; 2 forms every 2-hop row on the CPU), n = 100.  Skipped, and said so, where the reference build or the
               extension is not present.
No gate: the ratio yardstick / device is recorded per n.
Output: one JSON line per workload, also written to <out-prefix><workload>.json.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(call):
    t0 = time.perf_counter()
    out = call()
    return out, (time.perf_counter() - t0) * 1e3


def fetch_into(gg, agg, h, bufs):
    """every row of level h into the four page-locked arrays"""
    n = agg.rows(h)
    i64p, u64p = C.POINTER(C.c_int64), C.POINTER(C.c_uint64)
    got, o = C.c_uint32(), 0
    while o < n:
        gg._chk(gg.lib.gg_khop_aggregate_fetch(agg.handle, h, o, min(n - o, 1 << 20), bufs[0][o:].ctypes.data_as(i64p),
                                               C.cast(bufs[1][o:].ctypes.data, u64p), C.cast(bufs[2][o:].ctypes.data, u64p),
                                               bufs[3][o:].ctypes.data_as(i64p), C.byref(got)))
        o += got.value
    return n


def device_top(gg, agg, h, n, bufs):
    top = gg.khop_aggregate_top(agg, h, "total", True, n)
    try:
        rows = fetch_into(gg, top, h, bufs)
        return rows, top.stats
    finally:
        top.close()


def host_top(gg, agg, h, n, bufs):
    rows = fetch_into(gg, agg, h, bufs)
    ids, lo, hi = bufs[0][:rows], bufs[2][:rows].view(np.uint64), bufs[3][:rows]
    order = np.lexsort((ids, ~lo, ~hi))[:n]  # descending 128-bit total (hi signed, lo unsigned), then ascending id
    return order


def sql_part(workload, vid, src, dst, weights, hops_list, runs):
    from oracle import ref_duckdb as R
    from tests import khop_aggregate_top_ref as KT

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
            fn = (f"SELECT vertex, walks, total FROM gg_khop_aggregate_top({graph}, NULL, {h}, 'start', 'p_score', 'total', "
                  "true, NULL, 100) ORDER BY rank")
            ref = KT.sql_khop_aggregate_top(h, "start", 100)
            got = d.query_text(fn)  # warm-up, and the answer
            f_ms = [timed(lambda: d.query_text(fn))[1] for _ in range(runs)]
            (want, r_ms) = timed(lambda: d.query_text(ref))
            out["cases"].append({"hops": h, "n": 100, "function_ms_median": statistics.median(f_ms), "function_ms_all": f_ms,
                                 "reference_plan_ms": r_ms, "equal": got == want,
                                 "reference_over_function": r_ms / statistics.median(f_ms)})
            assert got == want
    finally:
        d.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="sf10,sf100")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--seed", type=int, default=15)
    ap.add_argument("--hops", type=int, default=2)
    ap.add_argument("--sql-hops", default="1")
    ap.add_argument("--no-sql", action="store_true")
    ap.add_argument("--out-prefix", default=None, help="e.g. profiles/r15_aggregate_top_")
    args = ap.parse_args()
    import duckdb_pgq_amd as pkg

    for workload in args.workloads.split(","):
        vid, src, dst = pkg.datagen.ldbc(workload)
        gg = pkg.GG(0)
        gg.append_vertices(vid)
        gg.append_edges(src, dst)
        csr = gg.build_csr()
        V, E, h = int(csr.V), int(csr.E), args.hops
        v2 = csr.export()[3]
        w_dense = np.random.RandomState(args.seed).randint(-(1 << 62), 1 << 62, size=V, dtype=np.int64)
        agg = gg.khop_aggregate(csr, h, h, "start", None, w_dense)
        groups = agg.rows(h)
        bufs = [gg.host_buffer(max(groups, 1)) for _ in range(4)]
        out = {"metric": "top n groups of a walk aggregate (gg_khop_aggregate_top)", "workload": workload, "V": V, "E": E,
               "hops": h, "groups": groups, "runs": args.runs, "drained_bytes_yardstick": 32 * groups, "cases": []}
        for n in (100, 1024, 65536, groups):
            n = min(n, groups)
            rows, st = device_top(gg, agg, h, n, bufs)  # warm-up: pool blocks
            dev_ids = bufs[0][:rows].copy()
            order = host_top(gg, agg, h, n, bufs)
            equal = bool(np.array_equal(bufs[0][order], dev_ids))
            d_ms, y_ms = [], []
            for _ in range(args.runs):  # in alternation
                d_ms.append(timed(lambda: device_top(gg, agg, h, n, bufs))[1])
                y_ms.append(timed(lambda: host_top(gg, agg, h, n, bufs))[1])
            step_ms = [timed(lambda: gg.khop_aggregate_top(agg, h, "total", True, n).close())[1] for _ in range(args.runs)]
            gg.profile_reset()
            gg.profile(True)
            gg.khop_aggregate_top(agg, h, "total", True, n).close()
            gg.profile(False)
            kernels = {k: {"launches": v[0], "ms": v[1]} for k, v in gg.profile_get().items()}
            e = {"n": n, "stats": st, "equal": equal, "top_step_ms_median": statistics.median(step_ms),
                 "device_ms_median": statistics.median(d_ms), "device_ms_all": d_ms,
                 "yardstick_ms_median": statistics.median(y_ms), "yardstick_ms_all": y_ms,
                 "yardstick_over_device": statistics.median(y_ms) / statistics.median(d_ms),
                 "kernel_ms_total": sum(v["ms"] for v in kernels.values()), "kernels": kernels}
            out["cases"].append(e)
            print(workload, "n", n, "top step %.3f ms" % e["top_step_ms_median"], "device %.3f ms" % e["device_ms_median"],
                  "yardstick %.3f ms" % e["yardstick_ms_median"], "equal", equal, file=sys.stderr, flush=True)
            assert equal
        agg.close()
        csr.close()
        gg.close()
        if args.no_sql:
            out["sql"] = {"available": False, "reason": "--no-sql"}
        else:
            order = np.argsort(vid, kind="stable")  # the weight of vertex id x is w_dense[dense index of x]
            at = np.argsort(v2, kind="stable")
            w_table = np.empty(V, np.int64)
            w_table[order] = w_dense[at]
            out["sql"] = sql_part(workload, vid, src, dst, w_table, [int(x) for x in args.sql_hops.split(",") if x],
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
