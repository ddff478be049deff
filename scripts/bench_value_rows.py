#!/usr/bin/env python3
"""bench_value_rows.py — what a value predicate and a top n over a walk table cost on the device (gg_result_filter_value,
gg_result_top_rows) over LDBC `knows`.

Per workload (default sf10) bench_extend.py's Zipf-skewed creator -> message table is staged beside `knows`; every message
gets a date (a seeded int64 in [0, 2^20), so dates tie).  With `--sources` (default 64 and 4096) seeded sample sources and
hops 1 and 2, the walks are extended from their last column over the message table, and on the extended rows
    filter   date in a range of about 1 %, 50 % and 100 % of the rows, materialised (with the extension's rowid column)
    top      n = 20, 1024 and 65536 by date descending, with and without the message id as tie column
are timed: the median wall time over `--runs` calls after a warm-up, the result left on the device, the kernels' times
from gg_profile_*, and bytes per second against the byte model of csrc/gg_value.hip:
    probe    per row 8 B cell + 16 B dictionary slot + 8 B value + 1/8 B mask (+ 8 B value scratch for the top)
    write    per row 1/8 B mask; per kept row 16 B (read + written) per column
    top      per digit pass before the compaction 1/8 B mask + 8 B per key word read (the value; + the tie cell below it;
             the row number is free); per survivor 16 B per column gathered
Next to each, in the same alternation, today's only other route: every row drained over PCIe in 1 Mi-row pieces and numpy on
the host — a boolean mask over the looked-up dates, or numpy.lexsort of the candidates.
Output: one JSON line per workload, also written to <out-prefix><workload>.json.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_extend import message_table, profiled, timed  # noqa: E402

PIECE = 1 << 20
DATES = 1 << 20


def drain(res, hops):
    """every id column of a table to the host in pieces, as a plan without the device operators drains them"""
    n = res.rows(hops)
    out = np.empty((hops + 1, max(n, 1)), np.int64)
    i64p = C.POINTER(C.c_int64)
    for o in range(0, n, PIECE):
        ptrs = (i64p * (hops + 1))(*[out[c, o:].ctypes.data_as(i64p) for c in range(hops + 1)])
        got = C.c_uint32()
        res.gg._chk(res.gg.lib.gg_result_fetch(res.handle, hops, o, min(PIECE, n - o), ptrs, C.byref(got)))
    return out[:, :n]


def host_dates(cols, col, sorted_ids, dates_sorted):
    return dates_sorted[np.searchsorted(sorted_ids, cols[col])]


def median_of(runs, device, host):
    device(), host and host()  # warm-up: pool blocks, the id table
    d_ms, h_ms, st = [], [], None
    for _ in range(runs):
        st, t = timed(device)
        d_ms.append(t)
        if host:
            _, t = timed(host)
            h_ms.append(t)
    return st, d_ms, h_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="sf10")
    ap.add_argument("--sources", default="64,4096")
    ap.add_argument("--per-person", type=int, default=30)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=13)
    ap.add_argument("--max-rows", type=int, default=400_000_000, help="extended tables of more rows are skipped")
    ap.add_argument("--max-host-rows", type=int, default=50_000_000, help="the host yardstick is skipped above")
    ap.add_argument("--out-prefix", default=None, help="e.g. profiles/r21_value_rows_")
    args = ap.parse_args()
    import duckdb_pgq_amd as pkg

    for workload in args.workloads.split(","):
        vid, src, dst = pkg.datagen.ldbc(workload)
        es, ed, er, counts = message_table(vid, args.per_person, args.seed)
        gg = pkg.GG(0)
        gg.append_vertices(vid)
        gg.append_edges(es, ed, er)
        gg.vertices_from_edges(keep_staged=True)
        ext_csr = gg.build_csr()
        ext_ids = ext_csr.export()[3]
        gg.staging_clear()
        gg.append_vertices(vid)
        gg.append_edges(src, dst)
        walk_csr = gg.build_csr()
        dates = np.random.RandomState(args.seed + 3).randint(0, DATES, ext_ids.size).astype(np.int64)
        order = np.argsort(ext_ids)
        sorted_ids, dates_sorted = ext_ids[order], dates[order]
        out = {"metric": "walk rows filtered by a value range and cut to the top n on the device", "workload": workload,
               "V": walk_csr.V, "E": walk_csr.E, "message_rows": int(es.size), "message_vertices": ext_csr.V,
               "runs": args.runs, "cases": {}}
        for n_src in [int(x) for x in args.sources.split(",") if x]:
            sources = pkg.datagen.pick_sources(vid, n_src, args.seed)
            for hops in (1, 2):
                tag = "%dhop_%d" % (hops, n_src)
                walks = gg.expand_khop_result(walk_csr, hops, sources)
                try:
                    counted = gg.extend_edge(walks, hops, ext_csr, hops, materialise=False)
                    if counted["rows_out"] > args.max_rows:
                        out["cases"][tag] = {"skipped": "%d rows" % counted["rows_out"]}
                        continue
                    _, ext = gg.extend_edge(walks, hops, ext_csr, hops, edges=True)
                finally:
                    walks.close()
                h, ncols = hops + 1, 2 * (hops + 1) + 1
                rows = counted["rows_out"]
                host = rows <= args.max_host_rows
                case = {"rows": rows, "filter": {}, "top": {}}
                try:
                    for name, hi in (("1pct", DATES // 100), ("50pct", DATES // 2), ("100pct", DATES)):
                        def device():
                            st, res = gg.filter_value(ext, h, h, ext_csr, dates, None, 0, hi - 1)
                            res.close()
                            return st

                        def on_host():
                            cols = drain(ext, h)
                            x = host_dates(cols, h, sorted_ids, dates_sorted)
                            return cols[:, (x >= 0) & (x < hi)].shape[1]

                        print("case filter", tag, name, file=sys.stderr, flush=True)
                        st, d_ms, h_ms = median_of(args.runs, device, on_host if host else None)
                        kernels = profiled(gg, device)
                        k_ms = sum(v["ms"] for k, v in kernels.items() if k.startswith("k_value"))
                        model = (8 + 16 + 8 + 0.125) * rows + 0.125 * rows + 16.0 * ncols * st["rows_out"]
                        med = statistics.median(d_ms)
                        case["filter"][name] = {
                            "stats": st, "ms_median": med, "ms_all": d_ms, "kernels": kernels, "k_value_ms": k_ms,
                            "model_bytes": model, "model_bytes_per_s_of_the_call": model / (med * 1e-3),
                            "model_bytes_per_s_of_the_kernels": model / (k_ms * 1e-3) if k_ms else None,
                            "host_drain_and_numpy_mask_ms_median": statistics.median(h_ms) if h_ms else None, "host_ms_all": h_ms}
                    for n in (20, 1024, 65536):
                        for tie in (None, h):
                            def device():
                                st, res = gg.top_rows(ext, h, h, ext_csr, dates, n, descending=True, tie_col=tie)
                                res.close()
                                return st

                            def on_host():
                                cols = drain(ext, h)
                                x = host_dates(cols, h, sorted_ids, dates_sorted)
                                keys = (np.arange(x.size), cols[tie], -x) if tie is not None else (np.arange(x.size), -x)
                                return cols[:, np.lexsort(keys)[:n]].shape[1]

                            name = "n%d_%s" % (n, "tie" if tie is not None else "no_tie")
                            print("case top", tag, name, file=sys.stderr, flush=True)
                            st, d_ms, h_ms = median_of(args.runs, device, on_host if host else None)
                            kernels = profiled(gg, device)
                            k_ms = sum(v["ms"] for k, v in kernels.items() if k.startswith(("k_value", "top_")))
                            med = statistics.median(d_ms)
                            probe = (8 + 16 + 8 + 0.125 + 8) * rows
                            case["top"][name] = {
                                "stats": st, "ms_median": med, "ms_all": d_ms, "kernels": kernels, "kernels_ms": k_ms,
                                "probe_model_bytes": probe, "rows_per_s_of_the_call": rows / (med * 1e-3),
                                "host_drain_and_numpy_lexsort_ms_median": statistics.median(h_ms) if h_ms else None,
                                "host_ms_all": h_ms}
                finally:
                    ext.close()
                out["cases"][tag] = case
        line = json.dumps(out)
        print(line)
        if args.out_prefix:
            path = args.out_prefix + workload.replace(".", "_") + ".json"
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(line + "\n")
        for c in (walk_csr, ext_csr):
            c.close()
        gg.close()


if __name__ == "__main__":
    main()
