"""Level sets (gg_level_sets) and UNION recursive CTEs with a depth counter, with the planner rules off and on.

(a) knows: one person, then 64 persons as 64 classes, over the SF100 knows CSR, max_levels 5 — every forced
    (set, order) combination and auto; 4096 persons as 4096 classes for one level (a large map under a sparse level:
    the other side of the order routes' crossover); for one person gg_reach_closure on the same CSR beside it.
(b) forest: scripts/bench_closure.py's synthetic reply forest (about 10^8 messages, 10 M posts), every post a seed in a
    class of its own — 10^15 bits are over the bitmap's budget, so this is the hash set's case.
(c) sql: the friends CTE of bi-10-shortestpath.sql without its min consumer over SF10 inside the compiled reference
    (oracle/_ref), rules off, then rules on with PRAGMA enable_gpu_recursive_levels; both results must be equal.
Per combination: ms per call as best of --runs with min and max, rows per level, the library's per-kernel event times of
one call, and ms per call at max_levels 1..5 (a level's time is the difference of two).  "auto_within_spread" says
whether auto's best exceeds the best forced combination's best by no more than that combination's own max - min.
Each part writes profiles/r08_levels_<part>.json (--out-dir).  --kernel-stats DIR turns the *kernel_stats.csv of a run
under rocprofv3 --kernel-trace --stats --output-format csv into profiles/r08_levels_kernel_stats.json.

    python scripts/bench_levels.py [--only knows,forest,sql] [--out-dir profiles]
"""
import argparse
import csv
import glob
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

COMBINATIONS = {"bitmap+sort": (1, 1), "bitmap+compact": (1, 2), "hash+sort": (2, 1), "auto": (0, 0)}


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


def _ms(times):
    return {"ms_best": round(min(times) * 1e3, 3), "ms_min": round(min(times) * 1e3, 3),
            "ms_max": round(max(times) * 1e3, 3), "ms_all": [round(t * 1e3, 3) for t in times]}


def _combinations(gg, csr, seeds, classes, n_classes, max_levels, names, a, by_level=True):
    out, rows = {}, None
    for name in names:
        gg.debug_level_sets(*COMBINATIONS[name])
        run = lambda m=max_levels: gg.level_sets(csr, seeds, classes, n_classes, m)  # noqa: E731
        res, times = _timed(run, a.warmup, a.runs)
        got = (res.rows(), res.fetch())
        res.close()
        if rows is None:
            rows = got
        same = got[0] == rows[0] and all(np.array_equal(x, y) for x, y in zip(got[1], rows[1]))
        entry = dict(_ms(times), rows_per_level=got[0], rows_equal_first_combination=bool(same),
                     kernels_one_call=_kernels(gg, run))
        if by_level and max_levels > 1:
            entry["ms_best_by_max_levels"] = {}
            for m in range(1, max_levels + 1):
                r, t = _timed(lambda: run(m), 1, a.runs)
                r.close()
                entry["ms_best_by_max_levels"][str(m)] = round(min(t) * 1e3, 3)
        out[name] = entry
    gg.debug_level_sets(0, 0)
    forced = {n: e for n, e in out.items() if n != "auto"}
    if forced and "auto" in out:
        best = min(forced, key=lambda n: forced[n]["ms_best"])
        spread = forced[best]["ms_max"] - forced[best]["ms_min"]
        out["best_forced"] = best
        out["auto_minus_best_forced_ms"] = round(out["auto"]["ms_best"] - forced[best]["ms_best"], 3)
        out["best_forced_spread_ms"] = round(spread, 3)
        out["auto_within_spread"] = bool(out["auto"]["ms_best"] - forced[best]["ms_best"] <= spread)
    return out


def bench_knows(a):
    import duckdb_pgq_amd as pkg

    vid, src, dst = pkg.datagen.ldbc("sf100")
    gg = pkg.GG(0)
    gg.append_vertices(vid)
    gg.append_edges(src, dst)
    csr = gg.build_csr()
    out = {"what": "gg_level_sets over the SF100 knows CSR, max_levels 5, every forced (set, order) combination and auto "
                   "(1 MI355X)", "vertices": int(csr.V), "edges": int(csr.E)}
    for n in (1, 64):
        seeds = pkg.datagen.pick_sources(vid, n, 3)
        classes = np.arange(n, dtype=np.uint32)
        out[f"{n}_person" + ("s" if n > 1 else "")] = dict(
            seeds=[int(s) for s in seeds[:4]], classes=n,
            **_combinations(gg, csr, seeds, classes, n, 5, list(COMBINATIONS), a))
    # the other side of the order routes' crossover: a large map (4096 classes: 1.8 G bits) under a sparse level
    seeds = pkg.datagen.pick_sources(vid, 4096, 3)
    out["4096_persons_1_level"] = dict(classes=4096, **_combinations(
        gg, csr, seeds, np.arange(4096, dtype=np.uint32), 4096, 1, ["bitmap+sort", "bitmap+compact", "auto"], a))
    seed = pkg.datagen.pick_sources(vid, 1, 3)
    run = lambda: gg.reach_closure(csr, seed, np.zeros(1, np.uint32), [1], 1)  # noqa: E731
    res, times = _timed(run, a.warmup, a.runs)
    out["reach_closure_1_person"] = dict(_ms(times), rows_per_level=res.rows(), kernels_one_call=_kernels(gg, run))
    res.close()
    csr.close()
    gg.close()
    return out


def bench_forest(a):
    import duckdb_pgq_amd as pkg
    from bench_closure import reply_forest

    src, dst, posts, n_messages = reply_forest(a.posts, 100_000, 8, 40, 7)
    gg = pkg.GG(0)
    gg.append_edges(src, dst)
    gg.vertices_from_edges()
    csr = gg.build_csr()
    classes = np.arange(posts.size, dtype=np.uint32)
    out = {"what": "gg_level_sets over scripts/bench_closure.py's reply forest, every post a seed in a class of its own, "
                   "unbounded: the hash set (the bitmap is over its budget), forced and as auto chooses it (1 MI355X)",
           "messages": int(n_messages), "edges": int(src.size), "seeds": int(posts.size), "classes": int(posts.size)}
    out.update(_combinations(gg, csr, posts, classes, posts.size, -1, ["hash+sort", "auto"], a, by_level=False))
    walk, wtimes = _timed(lambda: gg.walk_closure(csr, posts), a.warmup, a.runs)
    out["walk_closure"] = dict(_ms(wtimes), rows_per_level=walk.rows())
    walk.close()
    csr.close()
    gg.close()
    return out


FRIENDS = ("WITH RECURSIVE friends(startPerson, hopCount, friend) AS (SELECT p_personid, 0, p_personid FROM person "
           "WHERE 1=1 AND p_personid = {} UNION SELECT f.startPerson, f.hopCount+1, CASE WHEN f.friend = k.k_person1id "
           "then k.k_person2id ELSE k.k_person1id END FROM friends f, knows k WHERE 1=1 AND f.friend = k.k_person1id "
           "AND f.hopCount < 5) SELECT hopCount, count(*), sum(friend) FROM friends GROUP BY hopCount ORDER BY hopCount")


def bench_sql(a):
    import duckdb_pgq_amd as pkg
    from oracle import ref_duckdb as R

    vid, src, dst = pkg.datagen.ldbc("sf10")
    seed = int(pkg.datagen.pick_sources(vid, 1, 3)[0])
    d = R.RefDuckDB()
    d.load_ldbc(vid, src, dst)
    d.execute(f"LOAD '{R.EXTENSION}'")
    sql = FRIENDS.format(seed)
    out = {"what": "the friends CTE of bi-10-shortestpath.sql under count(*), sum(friend) GROUP BY hopCount over SF10 inside "
                   "the compiled reference, rules off vs rules + PRAGMA enable_gpu_recursive_levels (1 MI355X)",
           "sql": sql, "persons": int(vid.size), "knows_rows": int(src.size)}
    results = {}
    for mode in ("disable", "enable"):
        d.execute(f"PRAGMA {mode}_gpu_graph")
        d.execute(f"PRAGMA {mode}_gpu_recursive_levels")
        plan = d.explain(sql)
        times = []
        for _ in range(a.sql_runs):
            t = time.perf_counter()
            results[mode] = d.query_text(sql)
            times.append(time.perf_counter() - t)
        out[mode + "d"] = {"GG_RECURSIVE_LEVELS_in_plan": "GG_RECURSIVE_LEVELS" in plan, "s_best": round(min(times), 4),
                           "s_all": [round(t, 4) for t in times]}
    d.execute("PRAGMA disable_gpu_recursive_levels")
    d.execute("PRAGMA disable_gpu_graph")
    d.close()
    out["equal_results"] = results["disable"] == results["enable"]
    out["result"] = results["enable"]
    out["rules_on_faster"] = out["enabled"]["s_best"] < out["disabled"]["s_best"]
    return out


def kernel_stats(directory, out_dir, what):
    stats = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                name = re.search(r"k_\w+|[\w:]+(?=\(|$)", row["Name"].replace("(anonymous namespace)::", ""))
                stats.append({"kernel": name.group(0) if name else row["Name"], "calls": int(row["Calls"]),
                              "total_us": round(float(row["TotalDurationNs"]) / 1e3, 1),
                              "avg_us": round(float(row["AverageNs"]) / 1e3, 2), "percent": float(row["Percentage"])})
    with open(os.path.join(out_dir, "r08_levels_kernel_stats.json"), "w") as f:
        json.dump({"what": what, "stats": stats}, f, indent=1)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--posts", type=int, default=10_000_000)
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--sql-runs", type=int, default=2)
    p.add_argument("--only", default="knows,forest,sql")
    p.add_argument("--out-dir", default=None)
    p.add_argument("--kernel-stats", default=None)
    p.add_argument("--kernel-stats-what", default="rocprofv3 --kernel-trace --stats of scripts/bench_levels.py --only knows")
    a = p.parse_args()
    if a.kernel_stats:
        kernel_stats(a.kernel_stats, a.out_dir or os.path.join(ROOT, "profiles"), a.kernel_stats_what)
        return
    parts = {"knows": bench_knows, "forest": bench_forest, "sql": bench_sql}
    for name in a.only.split(","):
        got = parts[name](a)
        print(json.dumps(got)[:4000], flush=True)
        if a.out_dir:
            with open(os.path.join(a.out_dir, f"r08_levels_{name}.json"), "w") as f:
                json.dump(got, f, indent=1)


if __name__ == "__main__":
    main()
