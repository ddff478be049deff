"""gg_khop_aggregate_top restated in plain python integers (include/gg.h): the yardstick of the device selection and sort.

The input is one level of tests/khop_aggregate_ref.aggregate(): (ids, walks, totals).  Row a comes before row b iff key(a)
is better than key(b) — greater when descending, else smaller — or the keys are equal and a's id is the smaller one, in
both directions: ORDER BY key [DESC], id LIMIT n.  key is walks (an unsigned 64-bit value) or wrap128(total + bias of the
row's vertex); the rows keep their unbiased totals."""
import numpy as np

from tests import khop_aggregate_ref as K

ORDERS = ("total", "walks")


def top(level, n: int, order_by: str = "total", descending: bool = True, bias_of=None) -> tuple:
    """the first n rows of `level` = (ids, walks, totals) in rank order, as the same kind of triple.  bias_of: {vertex id:
    bias} (None: no bias; only with "total")"""
    assert order_by in ORDERS and (bias_of is None or order_by == "total")
    ids = [int(x) for x in np.asarray(level[0], np.int64).tolist()]
    walks, totals = [int(x) for x in level[1]], [int(x) for x in level[2]]
    assert len(set(ids)) == len(ids)
    if order_by == "walks":
        keys = [w % K.M64 for w in walks]
    else:
        keys = [K.wrap128(t + (bias_of[i] if bias_of is not None else 0)) for i, t in zip(ids, totals)]
    order = sorted(range(len(ids)), key=lambda r: (-keys[r] if descending else keys[r], ids[r]))[:max(int(n), 0)]
    return (np.array([ids[r] for r in order], np.int64), [walks[r] for r in order], [totals[r] for r in order])


def bias_by_id(g, bias) -> dict:
    """{vertex id: bias} from V integers in vertex-table order"""
    return {int(v): int(b) for v, b in zip(g.vid.tolist(), np.asarray(bias).tolist())}


def sql_khop_aggregate_top(h: int, group_by: str, n: int, order_by: str = "total", descending: bool = True,
                           sources=None, weighted: bool = True, biased: bool = False) -> str:
    """tests/khop_aggregate_ref.sql_khop_aggregate's chain ending like benchmark/ldbc/queries/bi-8.sql:41-53:
    ORDER BY [p_key.p_bias +] sum(...) | count(*) [DESC], p_key.p_personid LIMIT n, over person(p_personid, p_score,
    p_bias) and knows.  The bias joins the GROUP BY as bi-8's p.score does."""
    assert order_by in ORDERS and not (biased and order_by == "walks")
    sql = K.sql_khop_aggregate(h, group_by, sources, weighted)
    key = "p0" if group_by == "start" else f"p{h}"
    val = f"p{h}" if group_by == "start" else "p0"
    agg = "count(*)" if order_by == "walks" else (f"sum({val}.p_score)" if weighted else "sum(1)")
    if biased:
        sql += f", {key}.p_bias"
        agg = f"{key}.p_bias + {agg}"
    return sql + f" ORDER BY {agg}{' DESC' if descending else ''}, {key}.p_personid LIMIT {int(n)}"
