#!/usr/bin/env python3
"""bench_distinct.py — what SELECT DISTINCT over chosen columns of a walk table costs on the device (gg_result_distinct)
over LDBC `knows`.

Per workload (default sf10) bench_extend.py's Zipf-skewed creator -> message table is staged beside `knows`.  With
`--sources` (default 64 and 4096) seeded sample sources, the 2-hop walk table is deduplicated over [2], [0, 2] and all
columns, and the table extended from its last column over the message table over [3], [0, 3] and [0] (the sources
themselves: long runs of equal adjacent rows, the case the combining is for).  Per case and setting —
the default, the adjacent-lane combining off, twice and half the default slot count (gg_debug_distinct) — it records the
median wall time over `--runs` materialising calls after a warm-up (the result left on the device), every repeat, the
kernels' times per pass from gg_profile_* in a run of its own, rows_in / rows_out / probe_steps, and the bytes of the byte
model of csrc/gg_distinct.hip over the kernels' time:
    insert   per row 8 c B of cells + 4 B of slot number written; per probed slot 4 B of slot word + 8 c B of the
             occupant's cells
    flag     per row 4 B slot number + 4 B slot word + 1/8 B mask
    write    per row 1/8 B mask; per kept row 16 c B (read + written)
    table    4 B per slot set to 0xFF
That figure is a model, not traffic: a slot word and a gathered cell each cost a 32 B sector at the least.
Yardsticks, in the same alternation: every row drained over PCIe in 1 Mi-row pieces and numpy.unique(axis=0) on the host
(tables of at most --max-host-rows rows; repeated --runs times up to 5 M rows, once above) and, for [0, 2] with at most 64
sources, gg_khop_pair_counts' rows with walks != 0 — the same set from an independent kernel; the two sets must be equal.
Output: one JSON line per workload, also written to <out-prefix><workload>.json.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_extend import message_table, profiled, timed  # noqa: E402
from bench_value_rows import drain  # noqa: E402

PASSES = ("k_distinct_insert", "k_distinct_flag", "k_value_groups", "k_value_write")


def commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        return None  # (a copy of the tree without its history)


def model_bytes(st, c):
    rows, out, steps = st["rows_in"], st["rows_out"], st["probe_steps"]
    return {"insert": (8.0 * c + 4) * rows + (4 + 8.0 * c) * steps, "flag": 8.125 * rows,
            "write": 0.125 * rows + 16.0 * c * out, "table": 4.0 * st["slots"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="sf10")
    ap.add_argument("--sources", default="64,4096")
    ap.add_argument("--per-person", type=int, default=30)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=13)
    ap.add_argument("--max-rows", type=int, default=400_000_000, help="tables of more rows are skipped")
    ap.add_argument("--max-host-rows", type=int, default=30_000_000, help="the host yardstick is skipped above")
    ap.add_argument("--out-prefix", default=None, help="e.g. profiles/r24_distinct_")
    ap.add_argument("--commit", default=None, help="the commit measured, where the tree has no history to ask")
    args = ap.parse_args()
    import duckdb_pgq_amd as pkg

    for workload in args.workloads.split(","):
        vid, src, dst = pkg.datagen.ldbc(workload)
        es, ed, er, _ = message_table(vid, args.per_person, args.seed)
        gg = pkg.GG(0)
        gg.append_vertices(vid)
        gg.append_edges(es, ed, er)
        gg.vertices_from_edges(keep_staged=True)
        ext_csr = gg.build_csr()
        gg.staging_clear()
        gg.append_vertices(vid)
        gg.append_edges(src, dst)
        walk_csr = gg.build_csr()
        out = {"metric": "distinct tuples over chosen columns of a walk table on the device (gg_result_distinct)",
               "workload": workload, "commit": args.commit or commit(), "V": walk_csr.V, "E": walk_csr.E,
               "message_rows": int(es.size), "runs": args.runs, "cases": {}}
        for n_src in [int(x) for x in args.sources.split(",") if x]:
            sources = pkg.datagen.pick_sources(vid, n_src, args.seed)
            walks = gg.expand_khop_result(walk_csr, 2, sources)
            tables = [("walks", walks, 2, ([2], [0, 2], [0, 1, 2]))]
            counted = gg.extend_edge(walks, 2, ext_csr, 2, materialise=False)
            if counted["rows_out"] > args.max_rows:
                out["cases"]["extended_%d" % n_src] = {"skipped": "%d rows" % counted["rows_out"]}
            else:
                tables.append(("extended", gg.extend_edge(walks, 2, ext_csr, 2)[1], 3, ([3], [0, 3], [0])))
            for name, table, hops, column_sets in tables:
                rows = table.rows(hops)
                if rows > args.max_rows:
                    out["cases"]["%s_%d" % (name, n_src)] = {"skipped": "%d rows" % rows}
                    continue
                for cols in column_sets:
                    tag = "%s_%d_cols_%s" % (name, n_src, "_".join(map(str, cols)))
                    print("case", tag, rows, "rows", file=sys.stderr, flush=True)
                    c = len(cols)

                    def device():
                        st, res = gg.distinct(table, hops, cols)
                        res.close()
                        return st

                    def on_host():
                        got = drain(table, hops)
                        return np.unique(got[cols].T, axis=0).shape[0]

                    base = gg.distinct(table, hops, cols, materialise=False)
                    host = rows <= args.max_host_rows
                    host_runs = args.runs if rows <= 5_000_000 else 1
                    case = {"rows_in": rows, "rows_out": base["rows_out"], "settings": {}}
                    settings = [("default", 0, 0), ("no_combine", 0, 1), ("slots_x2", 2 * base["slots"], 0),
                                ("slots_half", base["slots"] // 2, 0)]
                    device()  # warm-up: pool blocks
                    h_ms = []
                    for r in range(args.runs):  # the settings and the host yardstick alternate inside every repeat
                        for sname, slots, combine in settings:
                            gg.debug_distinct(slots, combine)
                            st, t = timed(device)
                            s = case["settings"].setdefault(sname, {"ms_all": [], "probe_steps_all": []})
                            s["stats"] = st
                            s["ms_all"].append(t)
                            s["probe_steps_all"].append(st["probe_steps"])
                            assert st["rows_out"] == base["rows_out"], (tag, sname, st, base)
                        gg.debug_distinct(0, 0)
                        if host and r < host_runs:
                            n, t = timed(on_host)
                            assert n == base["rows_out"], (tag, n, base)
                            h_ms.append(t)
                    for sname, slots, combine in settings:  # the kernels' times: a run of its own per setting
                        gg.debug_distinct(slots, combine)
                        kernels = profiled(gg, device)
                        s = case["settings"][sname]
                        s["ms_median"] = statistics.median(s["ms_all"])
                        s["kernels"] = {k: v for k, v in kernels.items() if k in PASSES}
                        k_ms = sum(v["ms"] for v in s["kernels"].values())
                        model = model_bytes(s["stats"], c)
                        s["kernels_ms"] = k_ms
                        s["model_bytes"] = model
                        s["model_bytes_per_s_of_the_kernels"] = sum(model[p] for p in ("insert", "flag", "write")) / (k_ms * 1e-3) if k_ms else None
                    gg.debug_distinct(0, 0)
                    case["host_drain_and_numpy_unique_ms_median"] = statistics.median(h_ms) if h_ms else None
                    case["host_ms_all"] = h_ms
                    if name == "walks" and cols == [0, 2] and n_src <= 64:
                        def pairs():
                            pc = gg.khop_pair_counts(walk_csr, 2, 2, sources)
                            n = pc.rows(2)
                            pc.close()
                            return n

                        pairs()
                        p_ms = [timed(pairs)[1] for _ in range(args.runs)]
                        pc = gg.khop_pair_counts(walk_csr, 2, 2, sources)
                        idx, ids, w = pc.fetch(2)
                        pc.close()
                        assert (w != 0).all()
                        want = np.unique(np.stack([sources[idx], ids], axis=1), axis=0)
                        _, res = gg.distinct(table, hops, cols)
                        got = np.unique(drain(res, 1).T, axis=0)
                        res.close()
                        assert np.array_equal(got, want), "gg_result_distinct and gg_khop_pair_counts disagree"
                        case["pair_counts_ms_all"] = p_ms
                        case["pair_counts_ms_median"] = statistics.median(p_ms)
                        case["pair_counts_pairs"] = int(want.shape[0])
                    out["cases"][tag] = case
            for _, table, _, _ in tables:
                table.close()
        line = json.dumps(out)
        print(line)
        if args.out_prefix:
            path = args.out_prefix + workload.replace(".", "_") + ".json"
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(line + "\n")
        for csr in (walk_csr, ext_csr):
            csr.close()
        gg.close()


if __name__ == "__main__":
    main()
