#!/usr/bin/env python3
"""bench_group_by.py — what GROUP BY one column of a walk table on the device (gg_result_group_by) costs over LDBC `knows`.

Per workload (default sf10) bench_extend.py's Zipf-skewed creator -> message table is staged beside `knows`, and a message
-> tag table over `--tags` (default 2000) Zipf-skewed tags beside that.  With `--sources` (default 64 and 4096) seeded
sample sources and hops 1 and 2, the walks are extended from their last column over the message table, and the extended
rows grouped
    by v0           long runs: the copies of a parent are consecutive and so are the walks of a source
    by v_hops       the extended-from column: one run per parent
    by w            the message: scattered keys (each message occurs once per walk that ends in its creator)
    by tag          the rows extended once more over message -> tag and grouped by the tag: few keys, skewed — the only key
                    table of the four that fits the workgroup-private LDS table (6144 keys for counts, 2048 with weights)
each with and without weights (a seeded int64 per person, read through column 0), with routes 1 (LDS where the table fits)
and 2 (global cells) forced in alternation inside one loop (stats["route"] says which ran), the median wall time over
`--runs` calls after a warm-up with the groups left on the device, the kernels' times from gg_profile_*, and bytes per
second against the byte model of csrc/gg_group.hip:
    per input row  8 B of key cell + one 16-byte dictionary slot; with weights 8 B + 16 B + 8 B more
    per key        8 B (24 B with weights) zeroed and read twice, 4 B of flag written, scanned (read + written) and read
    per group      32 B written
Next to that, in the same alternation:
    host      the key column of the extended rows drained over PCIe in 1 MiB-row pieces and numpy.unique(return_counts) of it
    aggregate for the plain walks grouped by v0: gg_khop_aggregate(group_by start) on the same CSR and sources
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_extend import message_table, profiled, timed  # noqa: E402

LDS_KEYS = {False: 6144, True: 2048}
PIECE = 1 << 20


def tag_table(messages, n_tags, seed):
    """(message, tag): 0..3 tags per message, the tag of a row Zipf-skewed"""
    rng = np.random.RandomState(seed)
    n = rng.randint(0, 4, messages.size)
    src = np.repeat(messages, n)
    share = np.arange(1, n_tags + 1, dtype=np.float64) ** -0.8
    dst = 5_000_000_000_000 + rng.choice(n_tags, src.size, p=share / share.sum()).astype(np.int64)
    return src, dst


def byte_model(rows_in, V, groups, weighted):
    per_row = 8 + 16 + (8 + 16 + 8 if weighted else 0)
    per_key = 3 * (24 if weighted else 8) + 4 * 4
    return {"per_input_row_bytes": per_row, "per_key_bytes": per_key, "per_group_bytes": 32,
            "bytes": float(per_row) * rows_in + float(per_key) * V + 32.0 * groups}


def drain_column(res, hops, col):
    """every row of a table to the host in pieces, as a plan without the device operator drains them; column `col` is kept
    whole, the other columns land in one piece-sized buffer each"""
    n = res.rows(hops)
    out = np.empty(max(n, 1), np.int64)
    rest = [np.empty(PIECE, np.int64) for _ in range(hops + 1)]
    i64p = C.POINTER(C.c_int64)
    for o in range(0, n, PIECE):
        ptrs = (i64p * (hops + 1))(*[(out[o:] if c == col else rest[c]).ctypes.data_as(i64p) for c in range(hops + 1)])
        got = C.c_uint32()
        res.gg._chk(res.gg.lib.gg_result_fetch(res.handle, hops, o, min(PIECE, n - o), ptrs, C.byref(got)))
    return out[:n]


def group_case(gg, table, hops, key_col, key_csr, walk_csr, weights, runs, host):
    """routes 1 and 2 (and the host yardstick) in alternation over one table"""
    wargs = (None, None, None) if weights is None else (0, walk_csr, weights)
    weighted = weights is not None

    def one(route):
        gg.debug_group(route)
        agg, ms = timed(lambda: gg.group_by(table, hops, key_col, key_csr, *wargs))
        st = agg.stats
        agg.close()
        return st, ms

    def on_host():
        keys = drain_column(table, hops, key_col)
        return np.unique(keys, return_counts=True)[0].size

    for route in (1, 2):
        one(route)  # warm-up: pool blocks, the id table
    ms = {1: [], 2: []}
    h_ms, h_groups = [], None
    stats = {}
    for _ in range(runs):
        for route in (1, 2):
            stats[route], t = one(route)
            ms[route].append(t)
        if host:
            h_groups, t = timed(on_host)
            h_ms.append(t)
    entry = {"key_col": key_col, "weighted": weighted, "keys": key_csr.V,
             "fits_lds": key_csr.V <= LDS_KEYS[weighted], "routes": {}}
    for route in (1, 2):
        gg.debug_group(route)
        kernels = profiled(gg, lambda: gg.group_by(table, hops, key_col, key_csr, *wargs).close())
        st = stats[route]
        model = byte_model(st["rows_in"], key_csr.V, st["groups"], weighted)
        med = statistics.median(ms[route])
        k_ms = sum(v["ms"] for k, v in kernels.items() if k.startswith("k_group"))
        accum = sum(v["ms"] for k, v in kernels.items() if k.startswith("k_group_accum"))
        entry["routes"]["forced_%d" % route] = {
            "stats": st, "ms_median": med, "ms_all": ms[route], "kernels": kernels, "k_group_ms": k_ms,
            "k_group_accum_ms": accum, "byte_model": model, "model_bytes_per_s_of_the_call": model["bytes"] / (med * 1e-3),
            "model_bytes_per_s_of_the_kernels": model["bytes"] / (k_ms * 1e-3) if k_ms else None,
            "input_rows_per_s": st["rows_in"] / (med * 1e-3)}
    gg.debug_group(0)
    if host:
        assert h_groups >= stats[2]["groups"]  # (the host counts the keys that are no vertex too)
        entry["host_drain_and_numpy_unique"] = {"ms_median": statistics.median(h_ms), "ms_all": h_ms, "groups": h_groups}
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="sf10")
    ap.add_argument("--sources", default="64,4096")
    ap.add_argument("--per-person", type=int, default=30)
    ap.add_argument("--tags", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=13)
    ap.add_argument("--max-rows", type=int, default=400_000_000, help="extended tables of more rows are skipped")
    ap.add_argument("--max-host-rows", type=int, default=50_000_000, help="the host yardstick is skipped above")
    ap.add_argument("--out-prefix", default=None, help="e.g. profiles/r20_group_by_")
    args = ap.parse_args()
    import duckdb_pgq_amd as pkg

    for workload in args.workloads.split(","):
        vid, src, dst = pkg.datagen.ldbc(workload)
        es, ed, er, counts = message_table(vid, args.per_person, args.seed)
        ts, td = tag_table(ed, args.tags, args.seed + 1)
        gg = pkg.GG(0)
        gg.append_vertices(vid)
        gg.append_edges(es, ed, er)
        gg.vertices_from_edges(keep_staged=True)
        ext_csr = gg.build_csr()
        gg.staging_clear()
        gg.append_edges(ts, td)
        gg.vertices_from_edges()
        tag_csr = gg.build_csr()  # messages and tags: the join
        gg.staging_clear()
        gg.append_vertices(np.unique(td))
        tags_only = gg.build_csr()  # the tags alone: the key's table
        gg.staging_clear()
        gg.append_vertices(vid)
        gg.append_edges(src, dst)
        walk_csr = gg.build_csr()
        weights = np.random.RandomState(args.seed + 2).randint(-(1 << 62), 1 << 62, vid.size).astype(np.int64)
        out = {"metric": "walk rows grouped by one column on the device (gg_result_group_by)", "workload": workload,
               "V": walk_csr.V, "E": walk_csr.E, "message_rows": int(es.size), "message_vertices": ext_csr.V,
               "tag_rows": int(ts.size), "tags": tags_only.V, "runs": args.runs, "cases": {}}
        for n in [int(x) for x in args.sources.split(",") if x]:
            sources = pkg.datagen.pick_sources(vid, n, args.seed)
            for hops in (1, 2):
                tag = "%dhop_%d" % (hops, n)
                walks = gg.expand_khop_result(walk_csr, hops, sources)
                try:
                    # the plain walks by v0, next to gg_khop_aggregate
                    plain = group_case(gg, walks, hops, 0, walk_csr, walk_csr, None, args.runs, False)
                    a_ms = []
                    for _ in range(args.runs + 1):
                        agg, t = timed(lambda: gg.khop_aggregate(walk_csr, hops, hops, "start", sources=sources))
                        agg.close()
                        a_ms.append(t)
                    plain["gg_khop_aggregate_ms_median"] = statistics.median(a_ms[1:])
                    out["cases"]["walks_by_v0_" + tag] = plain
                    counted = gg.extend_edge(walks, hops, ext_csr, hops, materialise=False)
                    if counted["rows_out"] > args.max_rows:
                        out["cases"]["extended_" + tag] = {"skipped": "%d rows" % counted["rows_out"]}
                        continue
                    _, ext = gg.extend_edge(walks, hops, ext_csr, hops)
                finally:
                    walks.close()
                try:
                    host = counted["rows_out"] <= args.max_host_rows
                    for name, kc, key_csr in (("by_v0_", 0, walk_csr), ("by_from_col_", hops, walk_csr),
                                              ("by_w_", hops + 1, ext_csr)):
                        for w in (None, weights):
                            print("case", name + tag, "weighted" if w is not None else "count", file=sys.stderr, flush=True)
                            out["cases"][name + tag + ("_sum" if w is not None else "")] = group_case(
                                gg, ext, hops + 1, kc, key_csr, walk_csr, w, args.runs, host and w is None)
                    tagged_rows = gg.extend_edge(ext, hops + 1, tag_csr, hops + 1, materialise=False)["rows_out"]
                    if tagged_rows <= args.max_rows:
                        _, tagged = gg.extend_edge(ext, hops + 1, tag_csr, hops + 1)
                        try:
                            for w in (None, weights):
                                out["cases"]["by_tag_" + tag + ("_sum" if w is not None else "")] = group_case(
                                    gg, tagged, hops + 2, hops + 2, tags_only, walk_csr, w, args.runs,
                                    tagged_rows <= args.max_host_rows and w is None)
                        finally:
                            tagged.close()
                finally:
                    ext.close()
        line = json.dumps(out)
        print(line)
        if args.out_prefix:
            path = args.out_prefix + workload.replace(".", "_") + ".json"
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(line + "\n")
        for c in (walk_csr, tags_only, tag_csr, ext_csr):
            c.close()
        gg.close()


if __name__ == "__main__":
    main()
