#!/usr/bin/env python3
"""bench_edge_filter.py — what an edge condition over materialised walk rows (gg_result_filter_edge) costs over LDBC `knows`.

Per workload (default sf10), with `--sources` (default 64 and 4096) seeded sample sources:
    (a) closed4    the 3-hop walks of the sources closed to v0: hops 3, 3 -> 0, inner
    (b) anti2      the 2-hop walks of the sources, 0 -> 2, anti — the NOT EXISTS of interactive-complex-10
    (c) all2       the 2-hop table of ALL sources closed 2 -> 0, inner, next to gg_triangles(order 0, materialise) on the same
                   CSR, the two timed in alternation; their row counts must be equal.  Skipped, and said so, where the table
                   does not fit `--max-table-gb` (SF100: 12.8 G rows x 24 B does not fit in HBM)
each the median wall time over `--runs` calls after a warm-up, nothing fetched, split into expansion (gg_expand_khop_result,
waited for) and filter (gg_result_filter_edge, materialising), with input rows/s, output rows/s, the two kernels' times from
gg_profile_* and the filter's bytes per second against its own byte model (csrc/gg_filter.hip), per input row:
    16 B of condition cells + two 16-byte dictionary slots + 2 * ceil(log2 |in(v_to)|) * 4 B of probes + 4 B of m written and
    4 B read + 8 (hops + 1) B read, and 8 (hops + 1) B written per output row
(the probe term is the mean over the input rows, computed on the host from the CSR and the walk counts).
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


def walk_weights(off, nbr, V, sources_dense, hops, to_col):
    """weight of every vertex as v_to over the `hops`-hop walks of the sources (None: every vertex): how many walks have
    it in column to_col (float64: a model, not a count)"""
    row = np.repeat(np.arange(V), np.diff(off))
    w = np.ones(V) if sources_dense is None else np.bincount(sources_dense, minlength=V).astype(np.float64)
    for _ in range(to_col):  # walks of to_col edges from the sources ending at v
        w = np.bincount(nbr, weights=w[row], minlength=V)
    c = np.ones(V)
    for _ in range(hops - to_col):  # walks of the remaining edges starting at v
        c = np.bincount(row, weights=c[nbr], minlength=V)
    return w * c


def byte_model(off, nbr, V, sources_dense, hops, to_col, rows_in, rows_out):
    indeg = np.bincount(nbr, minlength=V)
    weight = walk_weights(off, nbr, V, sources_dense, hops, to_col)
    probes = 2.0 * np.ceil(np.log2(np.maximum(indeg, 1)))
    mean_probe_bytes = float((probes * weight).sum() / max(weight.sum(), 1.0)) * 4.0
    per_row = 16 + 32 + mean_probe_bytes + 8 + 8 * (hops + 1)
    return {"per_input_row_bytes": per_row, "mean_probe_bytes": mean_probe_bytes, "per_output_row_bytes": 8 * (hops + 1),
            "bytes": per_row * rows_in + 8.0 * (hops + 1) * rows_out}


def case(gg, csr, arrays, sources, hops, from_col, to_col, mode, runs, max_rows):
    off, nbr, V, lookup = arrays
    n_walks = gg.khop_count(csr, hops, hops, sources)[hops]
    print("case", hops, from_col, to_col, mode, "sources", None if sources is None else len(sources), "walks", n_walks,
          file=sys.stderr, flush=True)
    entry = {"hops": hops, "from_col": from_col, "to_col": to_col, "mode": mode,
             "sources": None if sources is None else int(len(sources)), "walks": int(n_walks)}
    if n_walks > max_rows:
        entry["skipped"] = "the walk table of %d rows is above --max-rows / --max-table-gb" % n_walks
        return entry, None

    def one():
        def expand():  # (the expansion may return with its last kernels queued: wait for them, or the filter is charged)
            walks = gg.expand_khop_result(csr, hops, sources)
            gg.staging_sync()
            return walks

        walks, e_ms = timed(expand)
        try:
            (st, res), f_ms = timed(lambda: gg.filter_edge(walks, hops, csr, from_col, to_col, mode))
            res.close()
        finally:
            walks.close()
        return st, e_ms, f_ms

    st, _, _ = one()  # warm-up: pool blocks, the reverse rows sorted by source, the id table
    e_all, f_all = [], []
    for _ in range(runs):
        _, e_ms, f_ms = one()
        e_all.append(e_ms)
        f_all.append(f_ms)
    kernels = profiled(gg, one)
    e_med, f_med = statistics.median(e_all), statistics.median(f_all)
    dense = None if sources is None else lookup(sources)
    model = byte_model(off, nbr, V, dense, hops, to_col, st["rows_in"], st["rows_out"])
    k_count = kernels.get("k_edge_filter_count", {}).get("ms")
    k_write = kernels.get("k_edge_filter_write", {}).get("ms")
    k_other = sum(v["ms"] for k, v in kernels.items() if not k.startswith("k_edge_filter_"))
    entry.update({"stats": st, "expand_ms_median": e_med, "expand_ms_all": e_all, "filter_ms_median": f_med,
                  "filter_ms_all": f_all, "call_ms_median": e_med + f_med,
                  "input_rows_per_s": st["rows_in"] / (f_med * 1e-3), "output_rows_per_s": st["rows_out"] / (f_med * 1e-3),
                  "k_edge_filter_count_ms": k_count, "k_edge_filter_write_ms": k_write, "other_kernels_ms": k_other, "byte_model": model,
                  "model_bytes_per_s_of_the_call": model["bytes"] / (f_med * 1e-3),
                  "model_bytes_per_s_of_the_kernels": (model["bytes"] / ((k_count + k_write) * 1e-3)
                                                       if k_count and k_write else None),
                  "kernels": kernels})
    return entry, one


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="sf10")
    ap.add_argument("--sources", default="64,4096")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=13)
    ap.add_argument("--max-rows", type=int, default=(1 << 32) - 1, help="walk tables of more rows are skipped")
    ap.add_argument("--max-table-gb", type=float, default=120.0, help="walk tables of more bytes are skipped")
    ap.add_argument("--out-prefix", default=None, help="e.g. profiles/r13_edge_filter_")
    args = ap.parse_args()
    import duckdb_pgq_amd as pkg

    for workload in args.workloads.split(","):
        vid, src, dst = pkg.datagen.ldbc(workload)
        gg = pkg.GG(0)
        gg.append_vertices(vid)
        gg.append_edges(src, dst)
        csr = gg.build_csr()
        off, nbr, _, v2 = csr.export()
        order = np.argsort(v2, kind="stable")

        def lookup(ids, v2=v2, order=order):
            ids = np.asarray(ids, np.int64)
            at = np.clip(np.searchsorted(v2[order], ids), 0, v2.size - 1)
            hit = v2[order][at] == ids
            return order[at][hit]

        arrays = (np.asarray(off, np.int64), np.asarray(nbr, np.int64), int(csr.V), lookup)
        out = {"metric": "edge condition over walk rows (gg_result_filter_edge)", "workload": workload, "V": csr.V,
               "E": csr.E, "runs": args.runs, "cases": {}}

        def limit(hops):
            return min(args.max_rows, int(args.max_table_gb * 1e9 / (8 * (hops + 1))))

        for n in [int(x) for x in args.sources.split(",") if x]:
            sources = pkg.datagen.pick_sources(vid, n, args.seed)
            out["cases"]["a_closed4_%d" % n], _ = case(gg, csr, arrays, sources, 3, 3, 0, "inner", args.runs, limit(3))
            out["cases"]["b_anti2_%d" % n], _ = case(gg, csr, arrays, sources, 2, 0, 2, "anti", args.runs, limit(2))
        entry, one = case(gg, csr, arrays, None, 2, 2, 0, "inner", args.runs, limit(2))
        if one is not None:  # (c) against gg_triangles on the same CSR, in alternation
            def tri_call():
                st, res = gg.triangles(csr, materialise=True)
                res.close()
                return st

            tst = tri_call()
            t_all, c_all = [], []
            for _ in range(args.runs):
                _, t_ms = timed(tri_call)
                (_, e_ms, f_ms), _ = timed(one)
                t_all.append(t_ms)
                c_all.append((e_ms, f_ms))
            entry["gg_triangles_materialise"] = {"stats": tst, "ms_median": statistics.median(t_all), "ms_all": t_all,
                                                 "kernels": profiled(gg, tri_call)}
            entry["alternated_expand_filter_ms"] = c_all
            entry["rows_equal_gg_triangles"] = entry["stats"]["rows_out"] == tst["rows"]
            entry["filter_over_gg_triangles"] = statistics.median([f for _, f in c_all]) / statistics.median(t_all)
            entry["call_over_gg_triangles"] = statistics.median([e + f for e, f in c_all]) / statistics.median(t_all)
            assert entry["rows_equal_gg_triangles"], (entry["stats"], tst)
        out["cases"]["c_all2"] = entry
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
