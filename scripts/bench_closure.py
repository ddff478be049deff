"""Walk closure (gg_walk_closure) on a synthetic reply forest, and bi-9.sql's statement with the planner rules off and on.

Forest: --posts roots, each level a fraction of the one above it (replies to random messages of the level above: the
shape of LDBC's reply trees — most replies within a few levels of their post), one hub post with --hub direct replies,
and --chains reply chains --chain-depth deep; about 10^8 messages at the defaults.  Every post is a seed, so one
closure returns every comment once per post above it (one row per walk).  Reports ms per closure (best of --runs,
fetch excluded), rows/s, rows per level, the kernel totals of one closure and the kernel time of every level
(library events of closures bounded at L and L - 1 levels, differenced).

SQL: bi-9.sql as shipped over a `message` table (the schema's view is a UNION ALL, which the reference refuses inside a
recursive arm) of --sql-messages rows and its persons, timed inside the compiled reference (oracle/_ref) with
PRAGMA disable_gpu_graph and enable_gpu_graph; both results must be equal.

    python scripts/bench_closure.py [--posts N] [--out profiles/r06_closure_forest.json] [--sql-out ...]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FANOUT = (1.6, 1.3, 1.0, 0.8, 0.6, 0.45, 0.3, 0.2, 0.12, 0.07, 0.04, 0.02, 0.01)  # level L+1 / level L


def reply_forest(posts, hub, chains, chain_depth, seed):
    """(parent id, child id) edges and the post ids; message ids are 0..n-1 shuffled into sparse ids"""
    rng = np.random.default_rng(seed)
    levels = [np.arange(posts, dtype=np.int64)]
    parents, children = [], []
    nxt = posts
    for f in FANOUT:
        m = int(levels[-1].size * f)
        if m == 0:
            break
        kids = np.arange(nxt, nxt + m, dtype=np.int64)
        parents.append(levels[-1][rng.integers(0, levels[-1].size, m)])
        children.append(kids)
        levels.append(kids)
        nxt += m
    parents.append(np.zeros(hub, np.int64))  # post 0 is the hub
    children.append(np.arange(nxt, nxt + hub, dtype=np.int64))
    nxt += hub
    for c in range(chains):
        ids = np.arange(nxt, nxt + chain_depth, dtype=np.int64)
        parents.append(np.concatenate([[1 + c], ids[:-1]]))
        children.append(ids)
        nxt += chain_depth
    src, dst = np.concatenate(parents), np.concatenate(children)
    perm = rng.permutation(src.size)
    sparse = np.arange(nxt, dtype=np.int64) * 16 + 1_000_000_007  # LDBC-like sparse message ids
    return sparse[src[perm]], sparse[dst[perm]], sparse[:posts], nxt


def bench_forest(a):
    import duckdb_pgq_amd as pkg

    src, dst, posts, n_messages = reply_forest(a.posts, a.hub, a.chains, a.chain_depth, 7)
    gg = pkg.GG(0)
    gg.append_edges(src, dst)
    gg.vertices_from_edges()
    csr = gg.build_csr()
    times, per_level = [], None
    for r in range(a.warmup + a.runs):
        gg.staging_sync()
        t = time.perf_counter()
        res = gg.walk_closure(csr, posts)
        dt = time.perf_counter() - t
        per_level = res.rows()
        res.close()
        if r >= a.warmup:
            times.append(dt)
    gg.profile_reset()
    gg.profile_select(None)
    gg.profile(True)
    res = gg.walk_closure(csr, posts)
    gg.profile(False)
    kernels = {name: {"launches": int(n), "ms": round(ms, 3)} for name, (n, ms) in gg.profile_get().items()}
    seed, rowid, level = res.fetch(0, 1 << 20)  # a slice, to show the fetch works at this size
    res.close()
    # per-level kernel times: closures bounded at 1, 2, ... levels, library events; level L's kernels (its degree
    # gather over level L-1, scan, tiles, expansion and its emit) = the bounded run at L minus the one at L-1
    closure_kernels = ("closure_deg", "scan_chained", "tile_partition", "closure_expand", "closure_emit")
    cumulative = [0.0]
    for bound in range(1, len(per_level) + 1):
        gg.profile_reset()
        gg.profile(True)
        gg.walk_closure(csr, posts, bound).close()
        gg.profile(False)
        got = gg.profile_get()
        cumulative.append(sum(got[k][1] for k in closure_kernels if k in got))
    level_ms = [round(cumulative[i] - cumulative[i - 1], 4) for i in range(1, len(cumulative))]
    csr.close()
    gg.close()
    rows = sum(per_level)
    best = min(times)
    return {"what": "gg_walk_closure over a synthetic reply forest, every post a seed (1 MI355X)",
            "messages": int(n_messages), "edges": int(src.size), "posts": int(a.posts), "hub_replies": a.hub,
            "chains": a.chains, "chain_depth": a.chain_depth, "levels": len(per_level), "rows_per_level": per_level,
            "rows": rows, "ms_per_closure_best": round(best * 1e3, 3),
            "ms_per_closure_all": [round(t * 1e3, 3) for t in times], "rows_per_s": round(rows / best),
            "kernels_one_closure": kernels, "kernel_ms_per_level": level_ms,
            "kernel_ms_per_level_note": "library events of closures bounded at L and L - 1 levels, differenced: the "
                                        "kernels that make level L (degree gather over level L - 1, scan, tile "
                                        "partition, expansion, emit)",
            "fetched_rows_checked": int(seed.size)}


def bench_sql(a):
    from oracle import ref_duckdb as R
    from tests.test_plan_rule import _ldbc_texts

    sql = _ldbc_texts()["queries"]["bi-9.sql"].strip().rstrip(";")
    n = a.sql_messages
    src, dst, posts, n_messages = reply_forest(n // 4, 0, 4, 30, 11)
    rng = np.random.default_rng(5)
    persons = np.arange(1, a.sql_persons + 1, dtype=np.int64) * 1000
    mid = np.concatenate([posts, dst])
    reply = np.concatenate([np.full(posts.size, -1, np.int64), src])
    d = R.RefDuckDB()
    d.load_table("raw", {"m_messageid": mid, "m_c_replyof": reply, "m_creatorid": persons[rng.integers(0, persons.size, mid.size)],
                         "day": rng.integers(0, 60, mid.size)})
    d.execute("CREATE TABLE message AS SELECT m_messageid, CASE WHEN m_c_replyof < 0 THEN NULL ELSE m_c_replyof END "
              "AS m_c_replyof, m_creatorid, TIMESTAMP '2012-05-15 00:00:00' + INTERVAL (day) DAY AS m_creationdate FROM raw")
    d.execute("DROP TABLE raw")
    d.load_table("pid", {"p_personid": persons})
    d.execute("CREATE TABLE person AS SELECT p_personid, 'first' AS p_firstname, 'last' AS p_lastname FROM pid")
    d.execute(f"LOAD '{R.EXTENSION}'")
    out = {"what": "bi-9.sql as shipped inside the compiled reference, rules off vs on (1 MI355X)",
           "messages": int(mid.size), "persons": int(persons.size)}
    results = {}
    for mode in ("disable", "enable"):
        d.execute(f"PRAGMA {mode}_gpu_graph")
        plan = d.explain(sql)
        runs = []
        for _ in range(a.sql_runs):
            t = time.perf_counter()
            results[mode] = d.execute_text(sql)
            runs.append(time.perf_counter() - t)
        out[mode + "d"] = {"GG_RECURSIVE_WALKS_in_plan": "GG_RECURSIVE_WALKS" in plan,
                           "s_best": round(min(runs), 4), "s_all": [round(t, 4) for t in runs]}
    d.execute("PRAGMA disable_gpu_graph")
    out["equal_results"] = results["disable"] == results["enable"]
    out["result_rows"] = len(results["enable"])
    d.close()
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--posts", type=int, default=10_000_000)
    p.add_argument("--hub", type=int, default=100_000)
    p.add_argument("--chains", type=int, default=8)
    p.add_argument("--chain-depth", type=int, default=40)
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--sql-messages", type=int, default=2_000_000)
    p.add_argument("--sql-persons", type=int, default=20_000)
    p.add_argument("--sql-runs", type=int, default=2)
    p.add_argument("--out", default=None)
    p.add_argument("--sql-out", default=None)
    p.add_argument("--skip-sql", action="store_true")
    a = p.parse_args()
    forest = bench_forest(a)
    print(json.dumps({k: v for k, v in forest.items() if k != "kernels_one_closure"}))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(forest, f, indent=1)
    if not a.skip_sql:
        sql = bench_sql(a)
        print(json.dumps(sql))
        if a.sql_out:
            with open(a.sql_out, "w") as f:
                json.dump(sql, f, indent=1)


if __name__ == "__main__":
    main()
