"""Reachability closure (gg_reach_closure) and UNION recursive CTEs with the planner rules off and on.

(a) forest: scripts/bench_closure.py's synthetic reply forest (about 10^8 messages, 10 M posts), every post a seed in a
    class of its own — the hash-set visited form.  On a forest the rows are the walk closure's (seed, end vertex) pairs:
    both closures run, their row sets are compared, and ms per closure is reported next to the walk closure's.
(b) knows: reachability from one person over the SF100 knows CSR (one class: the bitmap form).
(c) sql: the same statement over SF10 inside the compiled reference (oracle/_ref), rules off, then rules on with
    PRAGMA enable_gpu_recursive_union; both results must be equal.
(d) ic12: interactive-complex-12.sql as shipped, both ways, over the populated test database with a tag-class hierarchy.
Each part writes profiles/r07_reach_<part>.json (--out-dir).  Kernel tables come from a run under
rocprofv3 --kernel-trace --stats with --only forest,knows.

    python scripts/bench_reach.py [--only forest,knows,sql,ic12] [--out-dir profiles]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

KERNELS = ("reach_deg", "scan_chained", "tile_partition", "reach_expand", "reach_insert", "reach_emit", "radix_hist",
           "radix_scatter")


def _timed(fn, warmup, runs):
    times = []
    for r in range(warmup + runs):
        t = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t
        if r >= warmup:
            times.append(dt)
        if r < warmup + runs - 1:
            out.close()
    return out, times


def _kernels(gg, fn):
    gg.profile_reset()
    gg.profile_select(None)
    gg.profile(True)
    fn().close()
    gg.profile(False)
    return {name: {"launches": int(n), "ms": round(ms, 3)} for name, (n, ms) in gg.profile_get().items()}


def bench_forest(a):
    import duckdb_pgq_amd as pkg
    from bench_closure import reply_forest

    src, dst, posts, n_messages = reply_forest(a.posts, 100_000, 8, 40, 7)
    gg = pkg.GG(0)
    gg.append_edges(src, dst)
    gg.vertices_from_edges()
    csr = gg.build_csr()
    classes = np.arange(posts.size, dtype=np.uint32)
    run = lambda: gg.reach_closure(csr, posts, classes, None, posts.size)  # noqa: E731
    res, times = _timed(run, a.warmup, a.runs)
    per_level = res.rows()
    cls, vid, _ = res.fetch()
    res.close()
    walk = lambda: gg.walk_closure(csr, posts)  # noqa: E731
    wres, wtimes = _timed(walk, a.warmup, a.runs)
    w_levels = wres.rows()
    w_seed, w_rowid, _ = wres.fetch()
    wres.close()
    kernels = _kernels(gg, run)
    csr.close()
    gg.close()
    # the walk's end vertex is the destination of its last edge (rowid = append position)
    keys = np.sort((cls << 32) | vid)
    w_keys = np.sort((w_seed << 32) | dst[w_rowid])
    equal = bool(keys.size == w_keys.size and np.array_equal(keys, w_keys) and per_level == w_levels)
    best, wbest = min(times), min(wtimes)
    return {"what": "gg_reach_closure over scripts/bench_closure.py's reply forest, every post a seed in a class of its "
                    "own (hash-set visited form), against gg_walk_closure on the same CSR (1 MI355X)",
            "messages": int(n_messages), "edges": int(src.size), "seeds": int(posts.size), "classes": int(posts.size),
            "levels": len(per_level), "rows_per_level": per_level, "rows": int(sum(per_level)),
            "ms_per_closure_best": round(best * 1e3, 3), "ms_per_closure_all": [round(t * 1e3, 3) for t in times],
            "walk_closure_ms_best": round(wbest * 1e3, 3), "walk_closure_ms_all": [round(t * 1e3, 3) for t in wtimes],
            "ratio_to_walk_closure": round(best / wbest, 3),
            "rows_compared": int(keys.size), "row_sets_equal": equal, "kernels_one_closure": kernels}


def bench_knows(a):
    import duckdb_pgq_amd as pkg

    vid, src, dst = pkg.datagen.ldbc("sf100")
    gg = pkg.GG(0)
    gg.append_vertices(vid)
    gg.append_edges(src, dst)
    csr = gg.build_csr()
    seed = pkg.datagen.pick_sources(vid, 1, 3)
    one = np.zeros(1, np.uint32)
    run = lambda: gg.reach_closure(csr, seed, one, [1], 1)  # noqa: E731
    res, times = _timed(run, a.warmup, a.runs)
    per_level = res.rows()
    res.close()
    kernels = _kernels(gg, run)
    out = {"what": "gg_reach_closure from one person over the SF100 knows CSR (bitmap visited form, 1 MI355X)",
           "vertices": int(csr.V), "edges": int(csr.E), "seed": int(seed[0]), "levels": len(per_level),
           "rows_per_level": per_level, "rows": int(sum(per_level)),
           "ms_per_closure_best": round(min(times) * 1e3, 3), "ms_per_closure_all": [round(t * 1e3, 3) for t in times],
           "kernels_one_closure": kernels}
    csr.close()
    gg.close()
    return out


def _both_ways(d, sql, runs):
    out, results = {}, {}
    for mode in ("disable", "enable"):
        d.execute(f"PRAGMA {mode}_gpu_graph")
        d.execute(f"PRAGMA {mode}_gpu_recursive_union")
        plan = d.explain(sql)
        times = []
        for _ in range(runs):
            t = time.perf_counter()
            results[mode] = d.query_text(sql)
            times.append(time.perf_counter() - t)
        out[mode + "d"] = {"GG_RECURSIVE_REACH_in_plan": "GG_RECURSIVE_REACH" in plan, "s_best": round(min(times), 4),
                           "s_all": [round(t, 4) for t in times]}
    d.execute("PRAGMA disable_gpu_recursive_union")
    d.execute("PRAGMA disable_gpu_graph")
    key = lambda r: tuple("" if v is None else v for v in r)  # noqa: E731
    out["equal_results"] = sorted(results["disable"], key=key) == sorted(results["enable"], key=key)
    out["result_rows"] = len(results["enable"])
    return out


def bench_sql(a):
    import duckdb_pgq_amd as pkg
    from oracle import ref_duckdb as R

    vid, src, dst = pkg.datagen.ldbc("sf10")
    seed = int(pkg.datagen.pick_sources(vid, 1, 3)[0])
    d = R.RefDuckDB()
    d.load_ldbc(vid, src, dst)
    d.execute(f"LOAD '{R.EXTENSION}'")
    sql = (f"WITH RECURSIVE reach(p) AS (SELECT {seed}::BIGINT UNION SELECT k.k_person2id FROM reach r, knows k "
           "WHERE r.p = k.k_person1id) SELECT count(*), sum(p) FROM reach")
    out = {"what": "reachability from one person as a UNION recursive CTE over SF10 knows inside the compiled reference, "
                   "rules off vs rules + PRAGMA enable_gpu_recursive_union (1 MI355X)", "sql": sql,
           "persons": int(vid.size), "knows_rows": int(src.size)}
    out.update(_both_ways(d, sql, a.sql_runs))
    d.close()
    return out


def bench_ic12(a):
    from tests.test_gpu_recursive_union_sql import db as fixture, _ic12

    d = next(fixture.__wrapped__())  # the GPU test's populated database with its tag-class hierarchy
    out = {"what": "interactive-complex-12.sql as shipped over the populated test database (tests/"
                   "test_gpu_recursive_union_sql.py), rules off vs on (1 MI355X)"}
    out.update(_both_ways(d, _ic12(), a.sql_runs))
    d.close()
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--posts", type=int, default=10_000_000)
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--sql-runs", type=int, default=2)
    p.add_argument("--only", default="forest,knows,sql,ic12")
    p.add_argument("--out-dir", default=None)
    a = p.parse_args()
    parts = {"forest": bench_forest, "knows": bench_knows, "sql": bench_sql, "ic12": bench_ic12}
    for name in a.only.split(","):
        got = parts[name](a)
        print(json.dumps({k: v for k, v in got.items() if k != "kernels_one_closure"}), flush=True)
        if a.out_dir:
            with open(os.path.join(a.out_dir, f"r07_reach_{name}.json"), "w") as f:
                json.dump(got, f, indent=1)


if __name__ == "__main__":
    main()
