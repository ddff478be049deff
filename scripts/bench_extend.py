#!/usr/bin/env python3
"""bench_extend.py — what one more hop over a second edge table (gg_result_extend_edge) costs over LDBC `knows`.

Per workload (default sf10) a synthetic creator -> message table is staged beside `knows`: about `--per-person` (30) rows
per person, Zipf-skewed (person of rank r gets a share ~ r^-0.8, ranks in a seeded random order), message ids of their own
range, rowids that are not the append positions.  With `--sources` (default 64 and 4096) seeded sample sources and hops 1
and 2, with and without edge columns:
    (a) message   the `hops`-hop walks of the sources extended from their last column over the message table
    (b) knows     the same walks extended from their last column over the walk graph itself — as a multiset the
                  (hops + 1)-hop walk table — next to the yardstick: gg_expand_khop_result / gg_expand_khop_edges at
                  hops + 1 minus the expansion at hops, the three timed in alternation in the same run, and the yardstick
                  call's last-level kernel (mat_last, above 2^20 rows its product form mat_front / mat_rows_edges) next to
                  k_extend_write[_edges]
each the median wall time over `--runs` calls after a warm-up, nothing fetched, split into expansion (waited for) and
extend (materialising), with input rows/s, output rows/s, the kernels' times from gg_profile_* and bytes per second against
the byte model of csrc/gg_extend.hip:
    per input row   8 B of condition cell + one 16-byte dictionary slot + 8 B of offsets + 8 B of u and prefix written + 8 B
                    of them read
    per output row  8 (hops + 1) B of parent cells + 4 B of nbr + 8 B of vid read, 8 (hops + 2) B written; with edge columns
                    8 B of rowid (4 B where the rowid is the append position) + 8 hops B of parent edge cells read (0 B if
                    the input has none) and 8 (hops + 1) B written
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


def message_table(vid, per_person, seed):
    """(creator, message id, rowid): Zipf-skewed rows per person, in a seeded random append order"""
    rng = np.random.RandomState(seed)
    V = vid.size
    share = np.arange(1, V + 1, dtype=np.float64) ** -0.8
    counts = rng.multinomial(per_person * V, share / share.sum())[rng.permutation(V)]
    src = np.repeat(vid, counts)
    src = src[rng.permutation(src.size)]
    dst = 1_000_000_000_000 + rng.permutation(src.size).astype(np.int64)
    rowid = 3 * np.arange(src.size, dtype=np.int64)[::-1] + 7
    return src, dst, rowid, counts


def byte_model(hops, edges, in_edges, explicit_rowid, rows_in, rows_out):
    per_in = 8 + 16 + 8 + 8 + 8
    read = 8 * (hops + 1) + 4 + 8
    write = 8 * (hops + 2)
    if edges:
        read += (8 if explicit_rowid else 4) + (8 * hops if in_edges else 0)
        write += 8 * (hops + 1)
    return {"per_input_row_bytes": per_in, "per_output_row_read_bytes": read, "per_output_row_written_bytes": write,
            "bytes": float(per_in) * rows_in + float(read + write) * rows_out, "written_bytes": float(write) * rows_out}


def expand(gg, csr, hops, sources, edges):
    """the walk table, waited for (the expansion may return with its last kernels queued)"""
    walks = gg.expand_khop_edges(csr, hops, sources) if edges else gg.expand_khop_result(csr, hops, sources)
    gg.staging_sync()
    return walks


def case(gg, walk_csr, ext_csr, sources, hops, edges, explicit_rowid, runs, max_rows, yardstick):
    walks = expand(gg, walk_csr, hops, sources, False)
    try:
        counted = gg.extend_edge(walks, hops, ext_csr, hops, materialise=False)
    finally:
        walks.close()
    entry = {"hops": hops, "from_col": hops, "edges": edges, "sources": int(len(sources)), "counted": counted}
    print("case", entry, file=sys.stderr, flush=True)
    if counted["rows_out"] > max_rows:
        entry["skipped"] = "%d output rows are above --max-rows / --max-out-gb" % counted["rows_out"]
        return entry
    in_edges = edges and yardstick  # (the yardstick's input carries edge columns, as gg_expand_khop_edges' own prefix does)

    def one():
        walks, e_ms = timed(lambda: expand(gg, walk_csr, hops, sources, in_edges))
        try:
            (st, res), x_ms = timed(lambda: gg.extend_edge(walks, hops, ext_csr, hops, edges=edges))
            res.close()
        finally:
            walks.close()
        return st, e_ms, x_ms

    def longer():
        expand(gg, walk_csr, hops + 1, sources, edges).close()

    st, _, _ = one()  # warm-up: pool blocks, the id table
    e_all, x_all, l_all = [], [], []
    if yardstick:
        longer()
    for _ in range(runs):
        _, e_ms, x_ms = one()
        e_all.append(e_ms)
        x_all.append(x_ms)
        if yardstick:
            l_all.append(timed(longer)[1])
    kernels = profiled(gg, one)
    e_med, x_med = statistics.median(e_all), statistics.median(x_all)
    model = byte_model(hops, edges, in_edges, explicit_rowid, st["rows_in"], st["rows_out"])
    k_count = kernels.get("k_extend_count", {}).get("ms")
    k_tiles = kernels.get("k_extend_tiles", {}).get("ms")
    k_write = kernels.get("k_extend_write_edges" if edges else "k_extend_write", {}).get("ms")
    entry.update({"stats": st, "expand_ms_median": e_med, "expand_ms_all": e_all, "extend_ms_median": x_med,
                  "extend_ms_all": x_all, "call_ms_median": e_med + x_med,
                  "input_rows_per_s": st["rows_in"] / (x_med * 1e-3), "output_rows_per_s": st["rows_out"] / (x_med * 1e-3),
                  "k_extend_count_ms": k_count, "k_extend_tiles_ms": k_tiles, "k_extend_write_ms": k_write,
                  "byte_model": model, "model_bytes_per_s_of_the_call": model["bytes"] / (x_med * 1e-3),
                  "model_bytes_per_s_of_the_kernels": (model["bytes"] / ((k_count + k_tiles + k_write) * 1e-3)
                                                       if k_count and k_tiles and k_write else None),
                  "write_kernel_output_bytes_per_s": model["written_bytes"] / (k_write * 1e-3) if k_write else None,
                  "kernels": kernels})
    if yardstick:
        y_kernels = profiled(gg, longer)
        # the kernel that writes the yardstick's last level: mat_rows_edges with edges; mat_last, or above 2^20 rows the
        # product form mat_front, without
        ran = [k for k in ("mat_rows_edges", "mat_last", "mat_front", "mat_mid2") if k in y_kernels]
        name = max(ran, key=lambda k: y_kernels[k]["ms"]) if ran else None
        l_med = statistics.median(l_all)
        y_ms = y_kernels.get(name, {}).get("ms")
        entry["yardstick"] = {
            "call": "gg_expand_khop_edges" if edges else "gg_expand_khop_result", "hops": hops + 1,
            "ms_median": l_med, "ms_all": l_all, "minus_the_expansion_at_hops_ms": l_med - e_med,
            "last_level_kernel": name, "last_level_kernel_ms": y_ms,
            "last_level_kernel_output_bytes_per_s": model["written_bytes"] / (y_ms * 1e-3) if y_ms else None,
            "kernels": y_kernels}
        entry["extend_over_yardstick_call"] = x_med / max(l_med - e_med, 1e-6)
        entry["write_kernel_over_yardstick_kernel"] = k_write / y_ms if k_write and y_ms else None
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="sf10")
    ap.add_argument("--sources", default="64,4096")
    ap.add_argument("--per-person", type=int, default=30)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=13)
    ap.add_argument("--max-rows", type=int, default=(1 << 32) - 1, help="outputs of more rows are skipped")
    ap.add_argument("--max-out-gb", type=float, default=120.0, help="outputs of more bytes are skipped")
    ap.add_argument("--out-prefix", default=None, help="e.g. profiles/r18_extend_")
    args = ap.parse_args()
    import duckdb_pgq_amd as pkg

    for workload in args.workloads.split(","):
        vid, src, dst = pkg.datagen.ldbc(workload)
        es, ed, er, counts = message_table(vid, args.per_person, args.seed)
        gg = pkg.GG(0)
        gg.append_vertices(vid)
        gg.append_edges(es, ed, er)
        gg.vertices_from_edges(keep_staged=True)  # persons and messages: no row of the message table is dropped
        ext_csr = gg.build_csr()
        gg.staging_clear()
        gg.append_vertices(vid)
        gg.append_edges(src, dst)
        walk_csr = gg.build_csr()
        out = {"metric": "walk rows extended by one hop over a second edge table (gg_result_extend_edge)",
               "workload": workload, "V": walk_csr.V, "E": walk_csr.E,
               "message_table": {"rows": int(es.size), "vertices": ext_csr.V, "per_person_mean": float(counts.mean()),
                                 "per_person_max": int(counts.max()), "persons_without": int((counts == 0).sum())},
               "runs": args.runs, "cases": {}}
        for n in [int(x) for x in args.sources.split(",") if x]:
            sources = pkg.datagen.pick_sources(vid, n, args.seed)
            for hops in (1, 2):
                for edges in (False, True):
                    width = 8 * ((hops + 2) + (hops + 1 if edges else 0))
                    limit = min(args.max_rows, int(args.max_out_gb * 1e9 / width))
                    tag = "%dhop_%d%s" % (hops, n, "_edges" if edges else "")
                    for name, csr2, explicit, yardstick in (("a_message_", ext_csr, True, False),
                                                            ("b_knows_", walk_csr, False, True)):
                        try:
                            entry = case(gg, walk_csr, csr2, sources, hops, edges, explicit, args.runs, limit, yardstick)
                        except pkg.GGError as e:  # (an output the device cannot hold: said, and the other cases still run)
                            entry = {"hops": hops, "edges": edges, "sources": n, "failed": str(e)}
                        out["cases"][name + tag] = entry
        line = json.dumps(out)
        print(line)
        if args.out_prefix:
            path = args.out_prefix + workload.replace(".", "_") + ".json"
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(line + "\n")
        walk_csr.close()
        ext_csr.close()
        gg.close()


if __name__ == "__main__":
    main()
