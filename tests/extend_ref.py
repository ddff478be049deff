"""gg_result_extend_edge restated in plain numpy (include/gg.h): the yardstick of the device kernel.

Walk rows v0..vh are joined with the rows (key, next, rowid) of a second edge table on v_from_col = key: one output row
(v0..vh, next) per such edge row.  Input rows keep their order; the copies of one input row are consecutive and stand in
the append order of the edge rows (CSR order).  The rowid of an edge row is the one given, or its append position."""
import numpy as np

from tests import edge_filter_ref as F


def extend_rows(table, ext_src, ext_dst, ext_rowid, from_col: int, vertices=None):
    """(rows [M, h + 2], rowids [M], stats as gg_extend_stats reports them).  table: id rows [N, h + 1]; ext_rowid None:
    the append positions; vertices (ids) not None: an edge row with an endpoint outside them is dropped, as a CSR build
    drops it — its append position is still counted."""
    table = np.asarray(table, np.int64)
    es, ed = np.asarray(ext_src, np.int64), np.asarray(ext_dst, np.int64)
    pos = np.arange(es.size, dtype=np.int64)
    rid = pos if ext_rowid is None else np.asarray(ext_rowid, np.int64)
    if vertices is not None:
        keep = np.isin(es, vertices) & np.isin(ed, vertices)
        es, ed, rid = es[keep], ed[keep], rid[keep]
    order = np.argsort(es, kind="stable")  # the rows of a key in append order
    keys = es[order]
    cells = table[:, from_col] if table.shape[0] else np.empty(0, np.int64)
    lo, hi = np.searchsorted(keys, cells, "left"), np.searchsorted(keys, cells, "right")
    deg = (hi - lo).astype(np.int64)
    parent = np.repeat(np.arange(table.shape[0]), deg)
    within = np.arange(int(deg.sum())) - np.repeat(np.cumsum(deg) - deg, deg)
    pick = order[lo[parent] + within]
    rows = np.concatenate([table[parent], ed[pick].reshape(-1, 1)], axis=1)
    stats = {"rows_in": int(table.shape[0]), "rows_out": int(rows.shape[0]), "rows_matched": int((deg > 0).sum())}
    return rows, rid[pick], stats


def extend_rows_brute(table, ext_src, ext_dst, ext_rowid, from_col: int):
    """the same by two python loops (small inputs)"""
    rows, rids, matched = [], [], 0
    es, ed = np.asarray(ext_src, np.int64).tolist(), np.asarray(ext_dst, np.int64).tolist()
    rid = list(range(len(es))) if ext_rowid is None else np.asarray(ext_rowid, np.int64).tolist()
    for r in np.asarray(table, np.int64).tolist():
        hit = False
        for i, s in enumerate(es):
            if s == r[from_col]:
                rows.append(r + [ed[i]])
                rids.append(rid[i])
                hit = True
        matched += hit
    width = np.asarray(table).shape[1] + 1
    out = np.array(rows, np.int64).reshape(-1, width)
    return out, np.array(rids, np.int64), {"rows_in": len(table), "rows_out": len(rows), "rows_matched": matched}


HUB_ROWS = 3000
NOT_A_PERSON = 987_654_321_012
MESSAGE_BASE = 1_000_000_000


def two_hop_counts(g) -> np.ndarray:
    """2-hop walks per start vertex (dense)"""
    deg = np.diff(g.off)
    return np.bincount(g.su, weights=deg[g.dv].astype(np.float64), minlength=g.V).astype(np.int64)


def ext_table(g, seed: int = 0xE17):
    """A creator -> message table over the persons of g (a TriangleGraph of triangles_ref.hard_graph()): (src, dst, rowid,
    info).  info: hub (the key of HUB_ROWS rows, a person of few 2-hop walks), z (a person without rows and with more
    2-hop walks than the write pass stages input rows, 1024), stranger (a key that is no person)."""
    rng = np.random.RandomState(seed)
    two = two_hop_counts(g)
    one = np.diff(g.off)
    # the hub: a person of 8..30 two-hop walks, so its walk tables times HUB_ROWS stay small
    cand = np.nonzero((two >= 8) & (two <= 30) & (one >= 2))[0]
    hub_d = int(cand[0])
    # z: the person of the fewest 2-hop walks above 1100
    big = np.nonzero((two >= 1100) & (np.arange(g.V) != hub_d))[0]
    z_d = int(big[np.argmin(two[big])])
    hub, z = int(g.vid[hub_d]), int(g.vid[z_d])
    others = np.setdiff1d(np.arange(g.V), [hub_d, z_d])
    light = rng.choice(others, g.V // 10, replace=False)
    n_light = rng.randint(1, 9, light.size)
    src = np.concatenate([np.repeat(g.vid[light], n_light), np.full(HUB_ROWS, hub, np.int64)])
    src = src[rng.permutation(src.size)]  # the rows of a key are not adjacent in append order
    dst = MESSAGE_BASE + rng.permutation(src.size).astype(np.int64)
    dst[::7] = g.vid[rng.randint(0, g.V, dst[::7].size)]  # next ids that are person ids
    dst[3] = -4242  # a negative next id
    # parallel rows (same key, same next), and a key that is no person
    twice = np.nonzero(src == hub)[0][:5]
    src = np.concatenate([src, src[twice], np.full(3, NOT_A_PERSON, np.int64)])
    dst = np.concatenate([dst, dst[twice], MESSAGE_BASE + np.array([1, 2, 2], np.int64)])
    rowid = (src.size - np.arange(src.size, dtype=np.int64)) * 3 + 5
    info = {"hub": hub, "z": z, "stranger": NOT_A_PERSON}
    # what the tests rely on
    per_key = dict(zip(*np.unique(src, return_counts=True)))
    assert per_key[hub] >= HUB_ROWS
    persons = set(g.vid.tolist())
    with_rows = [k for k in per_key if k in persons and k != hub]
    assert abs(len(with_rows) - g.V // 10) <= 1 and all(1 <= per_key[k] <= 8 for k in with_rows)
    assert z not in per_key and two[z_d] >= 256 and two[z_d] > 1024
    assert NOT_A_PERSON not in persons and per_key[NOT_A_PERSON] == 3
    pairs = np.stack([src, dst], axis=1)
    assert np.unique(pairs, axis=0).shape[0] < pairs.shape[0]
    assert np.isin(dst, g.vid).any() and (dst < 0).sum() >= 1
    assert not np.array_equal(rowid, np.arange(src.size))
    return src, dst, rowid, info


def tag_table(ext_dst, seed: int = 0x7A6):
    """message -> tag rows over the next ids of an ext_table: 0..3 tags per distinct message, (src, dst, rowid)"""
    rng = np.random.RandomState(seed)
    msgs = np.unique(np.asarray(ext_dst, np.int64))
    n = rng.randint(0, 4, msgs.size)
    src = np.repeat(msgs, n)
    src = src[rng.permutation(src.size)]
    dst = 5_000_000 + rng.randint(0, 50, src.size).astype(np.int64)
    return src, dst, 11 + 2 * np.arange(src.size, dtype=np.int64)


def dense_rows(index: dict, id_rows: np.ndarray) -> np.ndarray:
    """id rows -> dense rows of the graph whose id dictionary is index (every id must be known)"""
    d = F.dense_of(index, np.asarray(id_rows, np.int64).reshape(-1)).reshape(np.asarray(id_rows).shape)
    assert (d >= 0).all()
    return d


# ---- the yardstick statements over person / knows / message(m_creatorid, m_messageid)
def sql_extend(hops: int, from_col: int, sources, select: str | None = None) -> str:
    """the `hops`-hop walks from a list of distinct persons joined with message on v_from_col = m_creatorid, every walk
    endpoint a row of person: hops 1, from 1 is the join of benchmark/ldbc/queries/interactive-complex-2.sql:2-7, hops 2,
    from 2 the friends-of-friends arm of interactive-complex-9.sql:13-15.  Rows (v0..vh, m_messageid, m.rowid)."""
    frm, cond = F._chain(hops)
    cols = select or (F.select_list(hops) + ", m.m_messageid, m.rowid")
    return (f"SELECT {cols} FROM {', '.join(frm)}, message m WHERE "
            + " AND ".join(cond + F._sources(sources) + [f"m.m_creatorid = p{from_col}.p_personid"]))
