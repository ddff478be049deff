"""The model k_expand_mid2's staging is written from (no GPU): tests/offset_runs.py restates how a tile of 768 reverse
entries finds its runs from the offsets alone — the 16-way search for the tile's first row, the window walked in chunks
of 256 rows, the run table, the mask of run starts and an entry's row by population count.  Here the model is held
against np.repeat(np.arange(V), deg), which is the row index the kernel no longer reads, and its khop(1, 2) figures
against the C oracle's, on the tables of the GPU tests (tests/test_gpu_offset_runs.py)."""
import numpy as np
import pytest

from tests import offset_runs as R
from tests.test_gpu_derived_reverse import reverse_reference

TABLES = R.tables()


@pytest.fixture(scope="module")
def graphs(orc):
    """name -> forward CSR, reverse CSR and khop(1, 2) of the oracle: computed once, shared, never changed."""
    out = {}
    for name, (vid, src, dst) in TABLES.items():
        rc, g = orc.csr_build(vid, src, dst)
        assert rc == 0
        try:
            off, nbr, _, o_vid = g.arrays()
            assert np.array_equal(o_vid, vid)  # dense index = position: the tables place their rows by it
            roff, rnbr, rrow = reverse_reference(o_vid, src, dst)
            out[name] = {"V": g.V, "E": g.E, "off": off.astype(np.int64), "nbr": nbr, "roff": roff, "rnbr": rnbr,
                         "rrow": rrow, "khop12": g.khop(1, 2)}
        finally:
            g.close()
    return out


def test_tables_are_what_they_claim(graphs):
    for E in R.EDGE_COUNTS:
        assert graphs[f"plain_{E}"]["E"] == E and graphs[f"mirrored_{E}"]["E"] == E
    g = graphs["plain_769"]
    assert np.any(g["nbr"] == np.repeat(np.arange(g["V"]), np.diff(g["off"])))  # self-loops
    pairs = g["rrow"] * g["V"] + g["rnbr"]
    assert np.unique(pairs).size < pairs.size  # duplicate rows
    s = graphs["star"]
    assert s["roff"][R.MT] == R.MT and s["roff"][R.MT + 1] - s["roff"][R.MT] == R.STAR_DEGREE
    for name in ("gaps_mirrored", "gaps_plain"):
        deg = np.diff(graphs[name]["roff"])
        live = np.flatnonzero(deg)
        assert live[0] >= R.GAP > 2 * R.XT and graphs[name]["V"] - 1 - live[-1] >= R.GAP
        assert np.max(np.diff(live)) > R.GAP


@pytest.mark.parametrize("name", sorted(TABLES))
def test_entry_rows_equal_the_row_index(graphs, name):
    g = graphs[name]
    x, tiles = R.entry_rows(g["off"], g["roff"], g["V"])
    assert np.array_equal(x, np.repeat(np.arange(g["V"]), np.diff(g["roff"]))) and np.array_equal(x, g["rrow"])
    assert len(tiles) == (g["E"] + R.MT - 1) // R.MT
    for t in tiles:
        assert t["rounds"] <= 5  # 19 bits of V: five rounds of 15 probes
        assert t["run"][0] == 0 and np.all(np.diff(t["run"]) > 0)  # the first run starts the tile; none is empty
        assert int(R.popcount64(t["mask"]).sum()) == t["run"].size - 1 <= R.MT


@pytest.mark.parametrize("name", sorted(TABLES))
def test_figures_equal_the_oracle(graphs, name):
    g = graphs[name]
    want = g["khop12"]
    got = R.khop12(g["off"], g["nbr"], g["roff"], g["rnbr"], g["V"])
    assert got == (want["rows"][1], want["rows"][2], want["digest"][1], want["digest"][2])


@pytest.mark.parametrize("name", ["plain_2309", "star", "gaps_plain"])
def test_both_search_widths_find_the_row(graphs, name):
    g = graphs[name]
    rng = np.random.default_rng(5)
    for p in np.concatenate([[0, g["E"] - 1], rng.integers(0, g["E"], 200)]):
        want = int(g["rrow"][p])
        for ways, most in ((16, 5), (64, 4)):
            x, rounds = R.find_row(g["roff"], g["V"], int(p), ways)
            assert x == want and rounds <= most


def test_star_tiles_meet_every_row_boundary_case(graphs):
    g = graphs["star"]
    _, tiles = R.entry_rows(g["off"], g["roff"], g["V"])
    assert tiles[0]["run"].size - 1 == R.MT                          # 768 rows of one entry: every position starts a run
    assert tiles[1]["x0"] == R.MT and tiles[1]["run"].tolist() == [0, R.MT]  # the hub's row starts where the tile does
    assert tiles[2]["run"].tolist() == [0, R.MT] and tiles[3]["run"].tolist() == [0, R.MT]  # whole tiles inside it
    assert tiles[5]["run"][1] == 3 and tiles[5]["run_x"][0] == R.MT  # ... and it ends three entries into a tile
    assert tiles[-1]["run"][-1] == (2 * R.STAR_DEGREE) % R.MT         # the last tile is short


def test_gaps_take_more_than_two_window_chunks(graphs):
    for name in ("gaps_mirrored", "gaps_plain"):
        g = graphs[name]
        _, tiles = R.entry_rows(g["off"], g["roff"], g["V"])
        assert max(t["chunks"] for t in tiles) >= 3   # the gap in the middle is crossed inside one tile
        assert tiles[0]["x0"] >= R.GAP                # the search skips the gap at the start
        assert tiles[-1]["chunks"] == 1               # the gap at the end is never walked: roff[x] >= p1 ends the window


def test_middle_ranges_add_up(graphs):
    """Ranges that begin on an empty row, inside a tile, and end at V."""
    g = graphs["gaps_plain"]
    V, want = g["V"], g["khop12"]
    cuts = [0, 5, R.GAP + 7, R.GAP + 40, 2 * R.GAP + 50, V]
    parts = [R.khop12(g["off"], g["nbr"], g["roff"], g["rnbr"], V, lo, hi) for lo, hi in zip(cuts, cuts[1:])]
    assert sum(p[0] for p in parts) == want["rows"][1] and sum(p[1] for p in parts) == want["rows"][2]
    assert sum(p[2] for p in parts) & R.M32 == want["digest"][1]
    assert sum(p[3] for p in parts) & R.M32 == want["digest"][2]
