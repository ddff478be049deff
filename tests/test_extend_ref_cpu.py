"""The extension restatement (tests/extend_ref.py) pinned against a brute-force loop, against the walk restatement when the
joined table is the walk graph itself and, where the compiled reference is present, against the reference's own hash-join
plan of `walk JOIN ext ON v = key`.  One test needs the built library but no GPU: the C-ABI exports the entry points."""
import ctypes as C

import numpy as np
import pytest

from oracle import ref_duckdb as R
from tests import edge_filter_ref as F
from tests import extend_ref as X
from tests import triangles_ref as T
from tests.oracle_lib import sort_rows


@pytest.fixture(scope="module")
def hard():
    vid, src, dst = T.hard_graph()
    g = T.TriangleGraph(vid, src, dst)
    return vid, src, dst, g, X.ext_table(g)


def test_the_fixture_has_the_shapes_the_device_tests_need(hard):
    vid, src, dst, g, (es, ed, er, info) = hard
    assert int((es == info["hub"]).sum()) >= 3000 and not (es == info["z"]).any()
    assert X.two_hop_counts(g)[g.index[info["z"]]] >= 256
    assert info["stranger"] not in g.index and (es == info["stranger"]).any()
    assert (ed < 0).any() and np.isin(ed, g.vid).any() and not np.array_equal(er, np.arange(er.size))


@pytest.mark.parametrize("hops", [1, 2])
def test_equals_the_brute_force_loop_for_every_column(hard, hops):
    vid, src, dst, g, (es, ed, er, info) = hard
    light = es[es != info["hub"]][:2]
    table = g.vid[F.walks(g, [info["hub"], int(light[0]), info["hub"], int(light[1])], hops)][:40]
    keep = np.concatenate([np.nonzero(es == info["hub"])[0][:7], np.nonzero(es != info["hub"])[0]])
    keep.sort()
    for fc in range(hops + 1):
        for rid in (er[keep], None):
            got = X.extend_rows(table, es[keep], ed[keep], rid, fc)
            want = X.extend_rows_brute(table, es[keep], ed[keep], rid, fc)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    assert X.extend_rows(table, es[keep], ed[keep], None, 0)[2]["rows_out"] > 0


@pytest.mark.parametrize("hops", [1, 2])
def test_over_the_walk_graph_from_the_last_column_it_is_the_next_hop(hard, hops):
    vid, src, dst, g, _ = hard
    S = g.vid[[3, 11, 3]]
    table = g.vid[F.walks(g, S, hops)]
    kept = np.isin(src, g.vid) & np.isin(dst, g.vid)  # the dangling rows of hard_graph never become CSR entries
    rows, rid, st = X.extend_rows(table, src, dst, None, hops, vertices=g.vid)
    want = g.vid[F.walks(g, S, hops + 1)]
    assert np.array_equal(rows, want) and st["rows_out"] == want.shape[0] > 0  # the same rows in the same order
    assert np.isin(rid, np.nonzero(kept)[0]).all()
    assert np.array_equal(src[rid], rows[:, hops]) and np.array_equal(dst[rid], rows[:, hops + 1])


def test_unknown_ids_empty_tables_and_order(hard):
    vid, src, dst, g, (es, ed, er, info) = hard
    table = np.array([[1, info["stranger"]], [2, -999], [3, info["hub"]]], np.int64)
    rows, rid, st = X.extend_rows(table, es, ed, er, 1)
    assert st == {"rows_in": 3, "rows_out": 3 + int((es == info["hub"]).sum()), "rows_matched": 2}
    assert rows[:3, 0].tolist() == [1, 1, 1] and (rows[3:, 0] == 3).all()  # input order; -999 matches nothing
    at = np.nonzero(es == info["hub"])[0]
    assert np.array_equal(rid[3:], er[at]) and np.array_equal(rows[3:, 2], ed[at])  # append order inside a parent
    none = X.extend_rows(np.empty((0, 2), np.int64), es, ed, er, 0)
    assert none[0].shape == (0, 3) and none[2] == {"rows_in": 0, "rows_out": 0, "rows_matched": 0}
    bare = X.extend_rows(table, np.empty(0, np.int64), np.empty(0, np.int64), None, 1)
    assert bare[0].shape == (0, 3) and bare[2]["rows_matched"] == 0


def test_the_library_exports_the_entry_points_and_the_binding_has_the_methods():
    import duckdb_pgq_amd as pkg
    from duckdb_pgq_amd import gg as binding

    lib = C.CDLL(binding.LIB_PATH)
    for name in ("gg_result_extend_edge", "gg_debug_extend"):
        assert hasattr(lib, name) and name in binding.SYMBOLS
    assert callable(getattr(pkg.GG, "extend_edge", None)) and callable(getattr(pkg.GG, "debug_extend", None))
    assert [f[0] for f in binding.ExtendStats._fields_] == ["rows_in", "rows_out", "rows_matched"]


needs_reference = pytest.mark.skipif(not R.available(), reason="reference build not present")


@pytest.fixture(scope="module")
def ref(hard):
    vid, src, dst, g, (es, ed, er, info) = hard
    d = R.RefDuckDB(threads=4)
    d.load_ldbc(vid, src, dst)
    d.load_table("message", {"m_creatorid": es, "m_messageid": ed, "m_rid": er})
    yield d
    d.close()


@needs_reference
@pytest.mark.parametrize("case", [(1, 1), (2, 2), (2, 1), (2, 0)])
def test_against_the_reference_hash_join_plan(hard, ref, case):
    vid, src, dst, g, (es, ed, er, info) = hard
    hops, fc = case
    light = np.unique(es[(es != info["hub"]) & np.isin(es, g.vid)])[:2]
    S = np.unique(np.concatenate([[info["hub"], info["z"]], light]))  # an IN list does not multiply
    got = ref.execute(X.sql_extend(hops, fc, S, F.select_list(hops) + ", m.m_messageid, m.m_rid"))  # (the rowids given)
    rows, rid, st = X.extend_rows(g.vid[F.walks(g, S, hops)], es, ed, er, fc)
    want = np.concatenate([rows, rid.reshape(-1, 1)], axis=1)
    assert want.shape[0] > 0 and np.array_equal(sort_rows(got), sort_rows(want))
