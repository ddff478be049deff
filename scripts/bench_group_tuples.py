#!/usr/bin/env python3
"""bench_group_tuples.py — what GROUP BY several columns of a walk table costs on the device (gg_result_group_tuples) over
LDBC `knows`.

Per workload (default sf10) bench_extend.py's Zipf-skewed creator -> message table and bench_group_by.py's message -> tag
table are staged beside `knows`.  With `--sources` (default 64 and 4096) seeded sample sources it groups the 2-hop walk table
over [2], [0, 2] and all columns, the table extended from its last column over the message table over [3] and [0, 3], and
that table extended once more over the tag table over [0, tag] (and [tag] alone, for the yardstick below) — each in the count
form and in the valued form (a date per message; the tag column's value is the tag's own number).  Per case and setting —
the LDS route forced where the groups fit, the global route forced, each with the adjacent-lane combining on and off
(gg_debug_group_tuples, gg_debug_distinct) — it records every repeat of `--runs` calls after a warm-up (the result left on
the device), the kernels' times per pass from gg_profile_* in a run of its own, the stats, and the bytes of the byte model
of csrc/gg_group_tuples.hip over the kernels' time:
    insert, flag   as scripts/bench_distinct.py
    accumulate     per row 8 c B of cells, valued form + 8 B cell + 16 B dictionary slot + 8 B value + 1/8 B valid (the run
                   heads' slot, prefix and mask words and the atomics are not in the model: their number is not reported)
    groups         per group 8 / 48 B initialised + read once + 8 c + 8 / 48 B written
That figure is a model, not traffic.
Yardsticks, in the same alternation: gg_result_distinct on the same columns (the insert pass alone); for [3] and [tag]
gg_result_group_by on the same table (count form: no weights; valued form: the same values as weights); and every row drained
over PCIe in 1 Mi-row pieces, numpy.unique(axis=0, return_inverse=True) and np.add.at / np.minimum.at / np.maximum.at on the
host (tables of at most --max-host-rows rows; once above 5 M rows).  Cases that are skipped say so.
Output: one JSON line per workload, also written to <out-prefix><workload>.json.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_distinct import commit  # noqa: E402
from bench_extend import message_table, profiled, timed  # noqa: E402
from bench_group_by import tag_table  # noqa: E402
from bench_value_rows import drain  # noqa: E402

PASSES = ("k_distinct_insert", "k_distinct_flag", "k_value_groups", "k_tuple_init", "k_tuple_accum", "k_tuple_accum_lds",
          "k_tuple_accum_valued", "k_tuple_accum_lds_valued", "k_value_write", "k_tuple_write")


def model_bytes(st, c, valued):
    rows, groups, steps = st["rows_in"], st["groups"], st["probe_steps"]
    cell = 48 if valued else 8
    return {"insert": (8.0 * c + 4) * rows + (4 + 8.0 * c) * steps, "flag": 8.125 * rows,
            "accumulate": (8.0 * c + (32.125 if valued else 0)) * rows, "groups": (2 * cell + 8.0 * c + cell) * groups,
            "table": 4.0 * st["slots"]}


def host_groups(cols_of_table, cols, value_cells, sorted_ids, values_sorted):
    keys = np.stack([cols_of_table[c] for c in cols], axis=1)
    uniq, inverse = np.unique(keys, axis=0, return_inverse=True)
    inverse = np.asarray(inverse).reshape(-1)
    rows = np.bincount(inverse, minlength=uniq.shape[0])
    if value_cells is None:
        return uniq.shape[0], int(rows.sum())
    x = values_sorted[np.searchsorted(sorted_ids, value_cells)]
    total = np.zeros(uniq.shape[0], np.float64)  # (a yardstick: the host's sum is not 128-bit)
    mn = np.full(uniq.shape[0], np.iinfo(np.int64).max, np.int64)
    mx = np.full(uniq.shape[0], np.iinfo(np.int64).min, np.int64)
    np.add.at(total, inverse, x)
    np.minimum.at(mn, inverse, x)
    np.maximum.at(mx, inverse, x)
    return uniq.shape[0], int(rows.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="sf10")
    ap.add_argument("--sources", default="64,4096")
    ap.add_argument("--per-person", type=int, default=30)
    ap.add_argument("--tags", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=13)
    ap.add_argument("--max-rows", type=int, default=400_000_000, help="tables of more rows are skipped")
    ap.add_argument("--max-host-rows", type=int, default=30_000_000, help="the host yardstick is skipped above")
    ap.add_argument("--out-prefix", default=None, help="e.g. profiles/r25_group_tuples_")
    ap.add_argument("--commit", default=None, help="the commit measured, where the tree has no history to ask")
    args = ap.parse_args()
    import duckdb_pgq_amd as pkg

    for workload in args.workloads.split(","):
        vid, src, dst = pkg.datagen.ldbc(workload)
        es, ed, er, _ = message_table(vid, args.per_person, args.seed)
        ts, td = tag_table(ed, args.tags, args.seed + 1)
        gg = pkg.GG(0)
        gg.append_vertices(vid)
        gg.append_edges(es, ed, er)
        gg.vertices_from_edges(keep_staged=True)
        ext_csr = gg.build_csr()
        ext_ids = ext_csr.export()[3]
        gg.staging_clear()
        gg.append_edges(ts, td)
        gg.vertices_from_edges()
        tag_csr = gg.build_csr()
        tag_ids = tag_csr.export()[3]
        gg.staging_clear()
        gg.append_vertices(vid)
        gg.append_edges(src, dst)
        walk_csr = gg.build_csr()
        walk_ids = walk_csr.export()[3]
        # a value per vertex of each CSR: a date per message (and per person), the tag's own number per tag
        rng = np.random.RandomState(args.seed + 2)
        values = {id(ext_csr): rng.randint(0, 1 << 40, ext_ids.size).astype(np.int64),
                  id(tag_csr): tag_ids.copy(), id(walk_csr): rng.randint(0, 1 << 40, walk_ids.size).astype(np.int64)}
        ids_of = {id(ext_csr): ext_ids, id(tag_csr): tag_ids, id(walk_csr): walk_ids}
        out = {"metric": "aggregates per key tuple over chosen columns of a walk table on the device (gg_result_group_tuples)",
               "workload": workload, "commit": args.commit or commit(), "V": walk_csr.V, "E": walk_csr.E,
               "message_rows": int(es.size), "tag_rows": int(ts.size), "runs": args.runs, "cases": {}, "not_run": []}
        for n_src in [int(x) for x in args.sources.split(",") if x]:
            sources = pkg.datagen.pick_sources(vid, n_src, args.seed)
            walks = gg.expand_khop_result(walk_csr, 2, sources)
            # (name, table, hops, column sets, the value column and its CSR, the one-column sets gg_result_group_by answers)
            tables = [("walks", walks, 2, ([2], [0, 2], [0, 1, 2]), (2, walk_csr), ())]
            counted = gg.extend_edge(walks, 2, ext_csr, 2, materialise=False)
            if counted["rows_out"] > args.max_rows:
                out["not_run"].append("extended_%d and tagged_%d: %d rows" % (n_src, n_src, counted["rows_out"]))
            else:
                ext = gg.extend_edge(walks, 2, ext_csr, 2)[1]
                tables.append(("extended", ext, 3, ([3], [0, 3]), (3, ext_csr), ([3],)))
                counted = gg.extend_edge(ext, 3, tag_csr, 3, materialise=False)
                if counted["rows_out"] > args.max_rows:
                    out["not_run"].append("tagged_%d: %d rows" % (n_src, counted["rows_out"]))
                else:
                    tables.append(("tagged", gg.extend_edge(ext, 3, tag_csr, 3)[1], 4, ([4], [0, 4]), (4, tag_csr), ([4],)))
            for name, table, hops, column_sets, (vc, vcsr), by_one in tables:
                rows = table.rows(hops)
                if rows > args.max_rows:
                    out["not_run"].append("%s_%d: %d rows" % (name, n_src, rows))
                    continue
                vals, vids = values[id(vcsr)], ids_of[id(vcsr)]
                order = np.argsort(vids, kind="stable")
                for cols in column_sets:
                    for valued in (False, True):
                        tag = "%s_%d_cols_%s_%s" % (name, n_src, "_".join(map(str, cols)), "valued" if valued else "count")
                        print("case", tag, rows, "rows", file=sys.stderr, flush=True)
                        c = len(cols)
                        vargs = (vc, vcsr, vals) if valued else ()

                        def device():
                            tg = gg.group_tuples(table, hops, cols, *vargs)
                            tg.close()
                            return tg.stats

                        def distinct():
                            st, res = gg.distinct(table, hops, cols)
                            res.close()
                            return st

                        def group_by():
                            agg = gg.group_by(table, hops, cols[0], vcsr, *((vc, vcsr, vals) if valued else ()))
                            agg.close()
                            return agg.stats

                        def on_host():
                            got = drain(table, hops)
                            return host_groups(got, cols, got[vc] if valued else None, vids[order], vals[order])

                        base = gg.group_tuples(table, hops, cols, *vargs, fetch=False).stats
                        host = rows <= args.max_host_rows
                        host_runs = args.runs if rows <= 5_000_000 else 1
                        case = {"rows_in": rows, "groups": base["groups"], "rows_valued": base["rows_valued"], "settings": {}}
                        settings = [("lds", 1, 0), ("lds_no_combine", 1, 1), ("global", 2, 0), ("global_no_combine", 2, 1)]
                        device()  # warm-up: pool blocks, the id table
                        d_ms, g_ms, h_ms = [], [], []
                        for r in range(args.runs):  # the settings and the yardsticks alternate inside every repeat
                            for sname, route, combine in settings:
                                gg.debug_group_tuples(route)
                                gg.debug_distinct(0, combine)
                                st, t = timed(device)
                                s = case["settings"].setdefault(sname, {"ms_all": []})
                                s["stats"] = st
                                s["ms_all"].append(t)
                                assert st["groups"] == base["groups"] and st["rows_valued"] == base["rows_valued"], (tag, st)
                            gg.debug_group_tuples(0)
                            gg.debug_distinct(0, 0)
                            st, t = timed(distinct)
                            assert st["rows_out"] == base["groups"], (tag, st, base)
                            d_ms.append(t)
                            if cols in by_one:
                                st, t = timed(group_by)
                                assert st["groups"] == base["groups"], (tag, st, base)
                                g_ms.append(t)
                            if host and r < host_runs:
                                (n, total), t = timed(on_host)
                                assert n == base["groups"] and total == rows, (tag, n, total, base)
                                h_ms.append(t)
                        for sname, route, combine in settings:  # the kernels' times: a run of its own per setting
                            gg.debug_group_tuples(route)
                            gg.debug_distinct(0, combine)
                            kernels = profiled(gg, device)
                            s = case["settings"][sname]
                            s["ms_median"] = statistics.median(s["ms_all"])
                            s["kernels"] = {k: v for k, v in kernels.items() if k in PASSES}
                            k_ms = sum(v["ms"] for v in s["kernels"].values())
                            model = model_bytes(s["stats"], c, valued)
                            s["kernels_ms"] = k_ms
                            s["model_bytes"] = model
                            s["model_bytes_per_s_of_the_kernels"] = (sum(v for k, v in model.items() if k != "table") / (k_ms * 1e-3)
                                                                     if k_ms else None)
                        gg.debug_group_tuples(0)
                        gg.debug_distinct(0, 0)
                        case["gg_result_distinct_ms_all"] = d_ms
                        case["gg_result_group_by_ms_all"] = g_ms if cols in by_one else "not run: more than one column"
                        case["host_drain_unique_and_at_ms_all"] = h_ms if host else "not run: %d rows" % rows
                        out["cases"][tag] = case
            for _, table, _, _, _, _ in tables:
                table.close()
        line = json.dumps(out)
        print(line)
        if args.out_prefix:
            path = args.out_prefix + workload.replace(".", "_") + ".json"
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(line + "\n")
        for csr in (walk_csr, tag_csr, ext_csr):
            csr.close()
        gg.close()


if __name__ == "__main__":
    main()
