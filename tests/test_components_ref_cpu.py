"""The components restatement (tests/components_ref.py) pinned against a brute-force breadth-first labelling on random
graphs, against hand-checked small cases and, where the compiled reference is present, against the reference's own UNION
recursive CTE under an aggregate.  One test needs the built library but no GPU: the C-ABI exports the entry points."""
import ctypes as C
import time

import numpy as np
import pytest

from oracle import ref_duckdb as R
from tests import components_ref as K


def check_tables(vid, src, dst):
    got = K.components(vid, src, dst)
    V = len(vid)
    su, dv = K.dense_edges(vid, src, dst)
    root = K.brute_force_roots(V, su, dv)
    assert np.array_equal(got["vertex"], np.asarray(vid, np.int64))
    assert np.array_equal(got["component"], np.asarray(vid, np.int64)[root] if V else got["component"])
    count = np.bincount(root, minlength=V) if V else np.empty(0, np.int64)
    assert np.array_equal(got["size"].astype(np.int64), count[root] if V else count)
    reps = [v for v in range(V) if root[v] == v]
    assert got["components"].tolist() == [int(vid[r]) for r in reps]  # ascending by the representative's position
    assert got["sizes"].tolist() == [int(count[r]) for r in reps]
    st = got["stats"]
    assert st["vertices"] == V and st["components"] == len(reps) and st["hooks"] == V - len(reps)
    assert int(got["sizes"].sum()) == V and st["largest"] == (max(count[reps]) if V else 0)
    assert st["singletons"] == sum(1 for r in reps if count[r] == 1) and st["entries_read"] == su.size
    return got


@pytest.mark.parametrize("seed", range(12))
def test_restatement_equals_a_breadth_first_labelling_on_random_graphs(seed):
    rng = np.random.RandomState(seed)
    V = int(rng.randint(1, 201))
    vid = (rng.permutation(4 * V)[:V] - V).astype(np.int64)  # distinct, some negative, not in order
    rows = int(rng.randint(0, 2 * V))  # sparse enough for several components
    pool = np.concatenate([vid, np.array([-10_000, 10_000], np.int64)])  # dangling endpoints among them
    src, dst = pool[rng.randint(0, pool.size, rows)], pool[rng.randint(0, pool.size, rows)]
    got = check_tables(vid, src, dst)
    if seed == 0:
        assert got["stats"]["components"] > 1
    # direction and order of the rows do not matter
    flipped = K.components(vid, dst[::-1], src[::-1])
    for key in ("component", "size", "components", "sizes"):
        assert np.array_equal(flipped[key], got[key])


def test_small_cases_by_hand():
    none = np.empty(0, np.int64)
    got = K.components(none, none, none)
    assert got["stats"] == {"vertices": 0, "components": 0, "largest": 0, "singletons": 0, "entries_read": 0, "hooks": 0}
    assert got["vertex"].size == got["components"].size == 0
    one = np.array([42], np.int64)
    for s, d in ((none, none), (one, one)):
        got = K.components(one, s, d)
        assert got["component"].tolist() == [42] and got["size"].tolist() == [1] and got["stats"]["singletons"] == 1
    vid = np.array([9, 4, 6, 1], np.int64)
    for s, d in (([9], [6]), ([6], [9])):  # one row, either way round: 9 is first in the table
        got = K.components(vid, np.array(s), np.array(d))
        assert got["component"].tolist() == [9, 4, 9, 1] and got["size"].tolist() == [2, 1, 2, 1]
        assert got["components"].tolist() == [9, 4, 1] and got["sizes"].tolist() == [2, 1, 1]
    got = K.components(vid, np.array([4, 1, 77]), np.array([88, 99, 9]))  # every row dangles
    assert got["stats"]["components"] == 4 and got["stats"]["entries_read"] == 0
    for shape in (K.straddling(), K.late_merge(64), K.ring_with_chords(65), K.islands(), K.star(50, False), K.pairs(40)):
        check_tables(*shape)
    assert K.components(*K.late_merge(64))["stats"]["components"] == 1
    isl = K.components(*K.islands())["stats"]
    assert isl["largest"] == 200 and isl["singletons"] > 10 and isl["components"] > isl["singletons"] + 3


def test_a_chain_of_2_17_edges_takes_well_under_a_second():
    n = (1 << 17) + 1
    for order in ("forward", "reverse", "shuffle"):
        vid, src, dst = K.path(n, order, 9)
        t0 = time.perf_counter()
        got = K.components(vid, src, dst)
        took = time.perf_counter() - t0
        print(order, f"{took:.3f} s")
        assert got["stats"]["components"] == 1 and got["stats"]["largest"] == n and got["stats"]["hooks"] == n - 1
        assert (got["component"] == vid[0]).all()
        assert took < 1.0


def test_the_library_exports_the_entry_points_and_the_binding_has_the_methods():
    import duckdb_pgq_amd as pkg
    from duckdb_pgq_amd import gg as binding

    lib = C.CDLL(binding.LIB_PATH)
    for name in ("gg_components", "gg_components_rows", "gg_components_fetch", "gg_components_fetch_sizes",
                 "gg_debug_components"):
        assert hasattr(lib, name) and name in binding.SYMBOLS
    assert callable(getattr(pkg.GG, "components", None)) and callable(getattr(pkg.GG, "debug_components", None))
    assert C.sizeof(binding.CcStats) == 8 * 7


needs_reference = pytest.mark.skipif(not R.available(), reason="reference build not present")


@needs_reference
def test_against_the_reference_recursive_cte():
    vid, src, dst = K.islands()
    want = K.min_id_partition(K.components(vid, src, dst))
    d = R.RefDuckDB(threads=4)
    try:
        d.load_table("person", {"p_personid": vid})
        d.load_table("knows", {"k_person1id": src, "k_person2id": dst})
        d.execute(K.sql_und())
        rows = d.query_text(K.sql_components())
    finally:
        d.close()
    got = {int(v): (int(m), int(c)) for v, m, c in rows}
    assert len(rows) == len(vid) == len(got)
    assert got == want
