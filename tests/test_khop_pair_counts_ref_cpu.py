"""The pair-count restatement (tests/khop_pair_counts_ref.py) pinned against a brute-force group-by over the walk rows of
tests/edge_filter_ref.walks, against rows of the adjacency matrix's powers and, where the compiled reference is present,
against the reference's own hash-aggregate plan on two keys.  One test needs the built library but no GPU: the C-ABI exports
the four entry points."""
import ctypes as C

import numpy as np
import pytest

from oracle import ref_duckdb as R
from tests import edge_filter_ref as F
from tests import khop_pair_counts_ref as P
from tests import triangles_ref as T


@pytest.fixture(scope="module")
def hard():
    vid, src, dst = T.hard_graph(V=300, rows=3000, seed=0x51, hub_fan=120)
    g = T.TriangleGraph(vid, src, dst)
    return vid, src, dst, g


def listed(g):
    """6 sources with a duplicate and an id that is no vertex"""
    hub = int(np.bincount(g.dv, minlength=g.V).argmax())
    return np.concatenate([g.vid[[hub, 3, hub, 17, 250]], [-123456789]])


def test_restatement_equals_the_group_by_over_the_walk_rows_and_the_matrix_powers(hard):
    vid, src, dst, g = hard
    S = listed(g)
    got = P.pair_counts(g, 3, S)
    E = int(g.su.size)
    assert got["entries_pulled"] == 3 * E and 0 < got["rows_gathered"] < 3 * E
    for h in (1, 2, 3):
        rows = got["rows"][h]
        assert len(rows[2]) > 0
        assert P.same(rows, P.group_walk_rows(g, S, h, F.walks))
        assert sum(rows[2]) == F.walks(g, S, h).shape[0]
        # the duplicate's two lanes hold equal rows, the non-vertex none
        lane0, lane2 = rows[0] == 0, rows[0] == 2
        assert np.array_equal(rows[1][lane0], rows[1][lane2]) and not (rows[0] == 5).any()
        # rows of A^h (float64 bound first: the int64 power is exact where it stays below 2^62)
        assert np.linalg.matrix_power(g.A.astype(np.float64), h).max() < 2.0 ** 62
        Ah = np.linalg.matrix_power(g.A, h)
        for lane, s in enumerate(S.tolist()):
            mine = rows[0] == lane
            if s not in g.index:
                assert not mine.any()
                continue
            row = Ah[g.index[s]]
            nz = np.nonzero(row)[0]
            assert np.array_equal(rows[1][mine], g.vid[nz])
            assert [int(x) for x in row[nz]] == [w for w, m in zip(rows[2], mine.tolist()) if m]


def test_targets_filter_the_rows_and_never_the_recurrence(hard):
    vid, src, dst, g = hard
    S = listed(g)
    targets = np.concatenate([g.vid[[3, 40, 40, 7]], [S[0]], [-999]])
    full = P.pair_counts(g, 3, S)
    cut = P.pair_counts(g, 3, S, targets)
    for h in (1, 2, 3):
        assert P.same(cut["rows"][h], P.filtered(full["rows"][h], g, targets))
    assert len(cut["rows"][3][2]) > 0
    assert cut["rows_gathered"] == full["rows_gathered"] and cut["entries_pulled"] == full["entries_pulled"]
    none = P.pair_counts(g, 2, S, np.empty(0, np.int64))
    assert all(len(none["rows"][h][2]) == 0 for h in (1, 2))


def test_counts_wrap_mod_2_64_and_a_wrapped_zero_is_no_pair():
    a, b = 5, 9
    vid = np.array([a, b], np.int64)
    src = np.concatenate([np.full(256, a), np.full(256, b)]).astype(np.int64)
    dst = np.concatenate([np.full(256, b), np.full(256, a)]).astype(np.int64)
    got = P.pair_counts(T.TriangleGraph(vid, src, dst), 8, [a])["rows"]
    assert got[7][2] == [256 ** 7] and got[7][1].tolist() == [b]
    assert len(got[8][2]) == 0  # 256^8 = 2^64 = 0
    src2, dst2 = src[:-1], dst[:-1]  # 255 rows b -> a
    got = P.pair_counts(T.TriangleGraph(vid, src2, dst2), 8, [a])["rows"]
    assert got[8][1].tolist() == [a] and got[8][2] == [(256 * 255) ** 4] and got[8][2][0] > 1 << 63


def test_the_library_exports_the_entry_points_and_the_binding_has_the_methods():
    import duckdb_pgq_amd as pkg
    from duckdb_pgq_amd import gg as binding

    lib = C.CDLL(binding.LIB_PATH)
    for name in ("gg_khop_pair_counts", "gg_khop_pair_counts_rows", "gg_khop_pair_counts_fetch", "gg_debug_pair_counts"):
        assert hasattr(lib, name) and name in binding.SYMBOLS
    assert callable(getattr(pkg.GG, "khop_pair_counts", None)) and callable(getattr(pkg.GG, "debug_pair_counts", None))
    assert C.sizeof(binding.PairStats) == 8 * (2 * (binding.GG_MAX_HOPS + 1) + 2)


needs_reference = pytest.mark.skipif(not R.available(), reason="reference build not present")


@pytest.fixture(scope="module")
def ref(hard):
    vid, src, dst, g = hard
    d = R.RefDuckDB(threads=4)
    d.load_table("person", {"p_personid": vid})
    d.load_table("knows", {"k_person1id": src, "k_person2id": dst})
    yield d
    d.close()


def as_sql_rows(rows, sources):
    """(source id, vertex id, walks) sorted; `sources` distinct, so a lane is an id"""
    return sorted((int(sources[i]), int(v), int(w)) for i, v, w in zip(rows[0].tolist(), rows[1].tolist(), rows[2]))


@needs_reference
@pytest.mark.parametrize("with_targets", [False, True])
@pytest.mark.parametrize("h", [1, 2])
def test_against_the_reference_hash_aggregate_plan(hard, ref, h, with_targets):
    vid, src, dst, g = hard
    S = list(dict.fromkeys(listed(g).tolist()))  # distinct, first occurrence first: an IN list does not multiply
    targets = sorted({int(x) for x in g.vid[[3, 40, 7, 100, 200]].tolist()} | {S[0], -999}) if with_targets else None
    want = P.pair_counts(g, h, S, targets)["rows"][h]
    assert len(want[2]) > 0
    got = sorted((int(a), int(b), int(c)) for a, b, c in ref.query_text(P.sql_pair_counts(h, S, targets)))
    assert got == as_sql_rows(want, S)
