"""tests/edge_ids.py by itself (no GPU): every placement has the ids it is named for, and every reference answer that
tests/test_gpu_edge_ids.py compares the device with is non-empty and holds an edge id — so no GPU test there can pass on an
empty answer.  Only the suite's existing restatements are used."""
from math import comb

import numpy as np
import pytest

from tests import edge_ids as EI
from tests import shortest_path_ref as SP
from tests import all_shortest_paths_ref as AP


def _has_edge_id(eg, ids) -> bool:
    return bool(np.isin(np.asarray(ids, np.int64).reshape(-1), eg.named).any())


def test_the_24_edge_ids():
    ids = EI.EDGE_IDS
    assert ids.dtype == np.int64 and ids.size == 24 == np.unique(ids).size
    low, high = ids.astype(np.uint64) & np.uint64(0xFFFFFFFF), ids.astype(np.uint64) >> np.uint64(32)
    flipped = high ^ np.uint64(0x80000000)
    marker = np.uint64(0xFFFFFFFF)
    assert (low == marker).sum() >= 6 and (flipped == marker).sum() >= 4          # either half is the sort's marker
    assert ((low == marker) & (flipped == marker)).sum() == 1 and ids[-1] == EI.I64_MAX  # both at once
    assert -1 in ids and np.iinfo(np.int64).min in ids                              # both plain halves; HT_EMPTY
    assert (low == 0).sum() >= 4                                                    # a group that shares a low half
    assert max(np.unique(high, return_counts=True)[1]) >= 4                         # and one that shares a high half


def test_relabel_keeps_strangers_strangers():
    vid = np.array([5, 9, 7], np.int64)
    src, dst = np.array([5, 100, 9, -3]), np.array([9, 7, 200, 100])
    v, s, d = EI.relabel(vid, src, dst, np.array([-1, EI.I64_MAX, EI.I64_MIN], np.int64))
    assert v.tolist() == [-1, EI.I64_MAX, EI.I64_MIN]
    assert s[0] == -1 and d[0] == EI.I64_MAX and s[2] == EI.I64_MAX and d[1] == EI.I64_MIN
    strangers = [int(s[1]), int(d[2]), int(s[3]), int(d[3])]
    assert not set(strangers) & set(v.tolist()) and strangers[0] == strangers[3] and len(set(strangers)) == 3


@pytest.mark.parametrize("kind", EI.PLACEMENTS)
def test_placement(kind):
    eg = EI.edge_graph(kind)
    vid = eg.vid
    assert vid.dtype == np.int64 and vid.size == 224 == np.unique(vid).size
    assert 2400 < eg.src.size == eg.dst.size < 4000
    assert np.isin(eg.named, vid).all() and np.isin(eg.wired, vid).all() and np.isin(eg.named, eg.wired).all()
    assert eg.wired.size == 24 == np.unique(eg.wired).size
    assert not np.array_equal(vid, np.sort(vid))  # the vertex-table order is not the id order
    span = int(vid.max()) - int(vid.min())
    if kind.startswith("dense"):
        assert span < 1 << 20
        # the dangling rows' ids are no vertices and lie inside the window
        strangers = np.setdiff1d(np.concatenate([eg.src, eg.dst]), vid)
        assert strangers.size >= 2 and (strangers > vid.min()).all() and (strangers < vid.max()).all()
    elif kind == "sparse":
        assert (1 << 20) <= span < 1 << 57 and vid.min() < 0 < vid.max()
    else:
        assert span == (1 << 64) - 1 and np.isin(EI.EDGE_IDS, vid).all()
    assert {"dense_zero": -1, "dense_u32": (1 << 32) - 1, "dense_max": EI.I64_MAX, "dense_min": EI.I64_MIN,
            "sparse": -1, "wide": -1}[kind] in vid
    if kind == "dense_max":
        assert vid.max() == EI.I64_MAX
    if kind == "dense_min":
        assert vid.min() == EI.I64_MIN
    # what hard_graph is for survives the relabelling
    g = eg.tri
    assert (g.A.diagonal() > 0).sum() == 2 and g.A.max() >= 2 and g.su.size < eg.src.size
    assert np.bincount(g.dv, minlength=g.V).max() > 80 and int(g.vid[np.bincount(g.dv, minlength=g.V).argmax()]) == eg.hub


@pytest.mark.parametrize("kind", EI.PLACEMENTS)
def test_triangle_rows_hold_the_edge_ids(kind):
    eg = EI.edge_graph(kind)
    ref = EI.references(eg)["triangles"]
    for order in (0, 1):
        rows, wedges = ref[(order, "all")]
        ids = eg.tri.id_rows(rows)
        assert np.isin(eg.wired, ids).all()  # each of the 24 occurs in a row of this order
        if kind == "wide":
            assert np.isin(EI.EDGE_IDS, ids).all()
        listed, _ = ref[(order, "list")]
        assert listed.shape[0] > 0 and _has_edge_id(eg, eg.tri.id_rows(listed))
    assert ref[(1, "all")][0].shape[0] >= comb(24, 3) == 2024
    assert ref[(0, "all")][0].shape[0] > ref[(1, "all")][0].shape[0]


@pytest.mark.parametrize("kind", EI.PLACEMENTS)
def test_every_other_reference_answer_is_non_empty_and_holds_an_edge_id(kind):
    eg = EI.edge_graph(kind)
    ref = EI.references(eg)
    for key, levels in ref["aggregate"].items():
        for h in (1, 2):
            ids, walks, totals = levels[h]
            assert len(walks) > 24 and _has_edge_id(eg, ids), (key, h)
            assert (set(totals) == {0}) == key[1]  # the zero weights make every group tie
    for name in ("pair_counts", "pair_counts_all"):
        for h in (1, 2):
            idx, ids, walks = ref[name]["rows"][h]
            assert len(walks) > 0 and _has_edge_id(eg, ids), (name, h)
    assert len(ref["pair_counts"]["rows"][2][2]) < len(ref["pair_counts_all"]["rows"][2][2])
    assert ref["components"]["stats"]["components"] == 1 and ref["components"]["sizes"].tolist() == [224]
    cc = ref["components_few_rows"]
    assert 10 < cc["stats"]["components"] < 224 and cc["stats"]["largest"] >= 24 and cc["stats"]["singletons"] > 0
    assert _has_edge_id(eg, cc["vertex"]) and np.isin(cc["components"], eg.wired).sum() == 1
    table = ref["table"]
    assert table.shape[0] > 100 and table.shape[1] == 3 and all(_has_edge_id(eg, table[:, c]) for c in range(3))
    if kind == "wide":  # the probed cells are edge ids, one of them INT64_MIN (HT_EMPTY)
        assert all(EI.I64_MIN in table[:, c] for c in range(3))
    for key, (rows, st) in ref["filter"].items():
        assert rows.shape[0] > 0 and _has_edge_id(eg, rows), key
    for fc, (rows, rid, st) in ref["extend"].items():
        assert 0 < st["rows_matched"] <= st["rows_in"] and rows.shape[0] > 0 and _has_edge_id(eg, rows[:, -1]), fc
    for key, ((ids, walks, totals), st) in ref["group_by"].items():
        assert st["groups"] > 0 and st["rows_grouped"] == st["rows_in"] and _has_edge_id(eg, ids), key


@pytest.mark.parametrize("kind", EI.PLACEMENTS)
def test_shortest_path_references_between_edge_ids(kind):
    eg = EI.edge_graph(kind)
    off, nbr, eid, vid = AP.csr_of(eg.vid, eg.src, eg.dst)
    assert np.array_equal(vid, eg.vid)
    s, t = EI.path_pairs(eg)
    pair, step, vertex, edge = SP.shortest_paths(off, nbr, eid, vid, s, t)
    assert pair.size > 0 and _has_edge_id(eg, vertex) and int(step.max()) >= 2
    rows = AP.all_shortest_paths(off, nbr, eid, vid, s, t)
    assert rows[0].size > pair.size and int(rows[1].max()) >= 1  # some pair has more than one shortest path


def test_tiny_graphs():
    t = EI.tiny_graphs()
    assert t["one_vertex"][0].tolist() == [-1] and t["one_vertex"][1].size == 0
    vid, src, dst = t["two_vertices"]
    assert vid.tolist() == [-1, EI.I64_MAX] and src.tolist() == dst[::-1].tolist() == [-1, EI.I64_MAX]
