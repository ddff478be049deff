"""The bind step of every gg table function (duckdb_pgq_amd/host/gg_duckdb_extension.cpp and the gg_*.cpp beside it), CPU
part: the result columns of a well-formed call, the description EXPLAIN prints, and every refusal the bind makes, with
the values literal here.  Binding fixes the schema and checks the arguments; the base tables are scanned and the device
is touched when the scan opens, at execution time (GGFunctionData::open), so DESCRIBE, EXPLAIN and a failing bind need
no GPU — tests/test_plan_rule.py relies on the same.  gg_graph_pin is the one function that is not covered: its bind
builds the graph.  Result parity of the functions is in tests/test_gpu_*_sql.py (-m gpu)."""
import os
import re

import pytest

from oracle import ref_duckdb as R

EXT = R.EXTENSION

pytestmark = pytest.mark.skipif(
    not (R.available() and os.path.exists(EXT) and bool(R.rules_route())),
    reason="reference build / extension / plan hook not present")

MAX_HOPS = 8  # GG_MAX_HOPS, include/gg.h
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


@pytest.fixture(scope="module")
def db():
    d = R.RefDuckDB(threads=2)
    d.execute("CREATE TABLE person (p_personid BIGINT PRIMARY KEY, p_score BIGINT)")
    d.execute("CREATE TABLE knows (k_person1id BIGINT NOT NULL, k_person2id BIGINT NOT NULL, k_weight INTEGER)")
    d.execute("CREATE TABLE message (m_messageid BIGINT NOT NULL, m_creatorid BIGINT NOT NULL, m_date BIGINT)")
    d.execute("INSERT INTO person VALUES (1, 10), (2, 20), (3, 30)")
    d.execute("INSERT INTO knows VALUES (1, 2, 1), (2, 3, 2), (3, 1, 3)")
    d.execute("INSERT INTO message VALUES (10, 1, 100), (11, 2, 200), (12, 3, 300)")
    d.execute(f"LOAD '{EXT}'")
    yield d
    d.close()


G = "'person', 'p_personid', 'knows', 'k_person1id', 'k_person2id'"
X = "'message', 'm_creatorid', 'm_messageid'"
SRC = "'SELECT 1'"
PAIRS = "'SELECT 1, 2'"


def big(*names):
    return [(n, "BIGINT") for n in names]


def v(hops):
    return big(*[f"v{i}" for i in range(hops + 1)])


def edge_filter(fn="gg_khop_edge_filter", hops=2, frm=2, to=0, mode="'inner'", sources="NULL"):
    return f"{fn}({G}, {sources}, {hops}, {frm}, {to}, {mode})"


def extend(fn="gg_khop_extend", hops=2, frm=2, tail="", ext=X, sources="NULL"):
    return f"{fn}({G}, {sources}, {hops}, {ext}, {frm}{tail})"


def group(hops=2, frm=2, key=3, n=10, ext=X):
    return extend("gg_khop_extend_group", hops, frm, f", {key}, {n}", ext)


def value_rows(fn="gg_khop_extend_filter", hops=2, frm=2, column="'m_date'", of=3, lo=100, hi=200, negate="false",
               top="", ext=X):
    return extend(fn, hops, frm, f", {column}, {of}, {lo}, {hi}, {negate}{top}", ext)


def top_rows(hops=2, frm=2, of=3, desc="true", tie=3, n=20, **kw):
    return value_rows("gg_khop_extend_top", hops, frm, of=of, top=f", {desc}, {tie}, {n}", **kw)


def distinct(fn="gg_khop_extend_distinct", hops=2, frm=2, columns="'0, 3'", ext=X):
    return extend(fn, hops, frm, f", {columns}", ext)


NO_EXT = "NULL, NULL, NULL"


def aggregate(hops=2, group_by="'start'", weight="'p_score'"):
    return f"gg_khop_aggregate({G}, NULL, {hops}, {group_by}, {weight})"


def aggregate_top(hops=2, group_by="'start'", weight="'p_score'", order="'total'", desc="true", bias="'p_score'", n=5):
    return f"gg_khop_aggregate_top({G}, NULL, {hops}, {group_by}, {weight}, {order}, {desc}, {bias}, {n})"


WALKS2 = "2-hop walks of knows"
JOINED2 = WALKS2 + " joined with message on v2 = m_creatorid"

# (id, the call, its result columns, the description under the operator's name in EXPLAIN — None: the function sets none)
CALLS = [
    ("khop_1", f"gg_khop({G}, 1, 1)", [("hops", "INTEGER")] + v(1), None),
    ("khop_max", f"gg_khop({G}, 2, {MAX_HOPS})", [("hops", "INTEGER")] + v(MAX_HOPS), None),
    ("khop_count", f"gg_khop_count({G}, 1, {MAX_HOPS})",
     [("hops", "INTEGER")] + big("rows", "digest", "traversed_edges"), None),
    ("shortest_path", f"gg_shortest_path({G}, {SRC}, 3)",
     [("startPerson", "BIGINT"), ("friend", "BIGINT"), ("hopCount", "INTEGER")], None),
    ("shortest_path_rows", f"gg_shortest_path_rows({G}, {PAIRS}, 3)",
     [("src", "BIGINT"), ("dst", "BIGINT"), ("step", "INTEGER"), ("vertex", "BIGINT"), ("edge_rowid", "BIGINT")], None),
    ("all_shortest_path_rows", f"gg_all_shortest_path_rows({G}, {PAIRS}, 3, 0)",
     [("src", "BIGINT"), ("dst", "BIGINT"), ("path", "BIGINT"), ("step", "INTEGER"), ("vertex", "BIGINT"),
      ("edge_rowid", "BIGINT")], None),
    ("shortest_path_counts", f"gg_shortest_path_counts({G}, {PAIRS}, -1)",
     [("src", "BIGINT"), ("dst", "BIGINT"), ("hops", "INTEGER"), ("paths", "HUGEINT")], None),
    ("same_neighbour_1", "gg_same_neighbour_paths('SELECT p_personid FROM person', 'SELECT 1', 'knows', 'k_person1id', "
     "'k_person2id', 'knows', 'k_person2id', 'k_person1id', 1)", big("w") + v(1), None),
    ("same_neighbour_max", "gg_same_neighbour_paths('SELECT p_personid FROM person', 'SELECT 1', 'knows', 'k_person1id', "
     f"'k_person2id', 'knows', 'k_person2id', 'k_person1id', {MAX_HOPS - 1})", big("w") + v(MAX_HOPS - 1), None),
    ("graph_pins", "gg_graph_pins()", big("pinned"), None),
    ("graph_unpin", "gg_graph_unpin()", big("unpinned"), None),
    ("triangle_count", f"gg_triangle_count({G}, true)", big("rows", "digest", "wedges"), "ordered triangles of knows"),
    ("triangles", f"gg_triangles({G}, false)", v(2), "triangles of knows"),
    ("triangles_ordered_null", f"gg_triangles({G}, NULL::BOOLEAN)", v(2), "triangles of knows"),
    ("triangle_edges", f"gg_triangle_edges({G}, true)", v(2) + big("e1", "e2", "e3"),
     "ordered triangles of knows with edge rowids"),
    ("edge_filter_1", edge_filter(hops=1, frm=1, to=0), v(1), "inner edge v1 -> v0 over 1-hop walks of knows"),
    ("edge_filter_max", edge_filter(hops=MAX_HOPS, frm=0, to=MAX_HOPS, mode="'anti'", sources=SRC), v(MAX_HOPS),
     f"anti edge v0 -> v{MAX_HOPS} over {MAX_HOPS}-hop walks of knows"),
    ("edge_filter_count", edge_filter("gg_khop_edge_filter_count", mode="'semi'"), big("rows", "walks", "matches"),
     "semi edge v2 -> v0 over " + WALKS2),
    ("extend_1", extend(hops=1, frm=1), v(1) + big("w", "ext_rowid"),
     "1-hop walks of knows joined with message on v1 = m_creatorid"),
    ("extend_max", extend(hops=MAX_HOPS - 1, frm=0, sources=SRC), v(MAX_HOPS - 1) + big("w", "ext_rowid"),
     f"{MAX_HOPS - 1}-hop walks of knows joined with message on v0 = m_creatorid"),
    ("extend_count", extend("gg_khop_extend_count"), big("rows", "walks", "matched"), JOINED2),
    ("extend_group", group(), big("rank", "key", "rows"), "top 10 by count of " + JOINED2 + ", grouped by column 3"),
    ("extend_group_all", group(hops=MAX_HOPS - 1, frm=0, key=MAX_HOPS, n="NULL"), big("rank", "key", "rows"),
     f"every group by count of {MAX_HOPS - 1}-hop walks of knows joined with message on v0 = m_creatorid, "
     f"grouped by column {MAX_HOPS}"),
    ("extend_filter_1", value_rows(hops=1, frm=1, of=2), v(1) + big("w", "ext_rowid"),
     "1-hop walks of knows joined with message on v1 = m_creatorid, m_date of column 2 in [100, 200]"),
    ("extend_filter_max", value_rows(hops=MAX_HOPS - 1, frm=0, column="'p_score'", of=0, lo="NULL", hi="NULL",
                                     negate="true"), v(MAX_HOPS - 1) + big("w", "ext_rowid"),
     f"{MAX_HOPS - 1}-hop walks of knows joined with message on v0 = m_creatorid, p_score of column 0 outside "
     f"[{I64_MIN}, {I64_MAX}]"),
    ("extend_filter_count", value_rows("gg_khop_extend_filter_count", negate="NULL::BOOLEAN"), big("rows", "walks", "valued"),
     JOINED2 + ", m_date of column 3 in [100, 200]"),
    ("extend_top", top_rows(), big("rank") + v(2) + big("w", "ext_rowid"),
     JOINED2 + ", m_date of column 3 in [100, 200], ordered descending"),
    ("extend_top_max", top_rows(hops=MAX_HOPS - 1, frm=1, of=MAX_HOPS, desc="NULL::BOOLEAN", tie="NULL", n="NULL"),
     big("rank") + v(MAX_HOPS - 1) + big("w", "ext_rowid"),
     f"{MAX_HOPS - 1}-hop walks of knows joined with message on v1 = m_creatorid, m_date of column {MAX_HOPS} in "
     "[100, 200], ordered"),
    ("distinct_one", distinct(columns="'3'"), big("c0"), "distinct columns 3 of " + JOINED2),
    ("distinct_several", distinct(columns="' 3, 0 ,1'"), big("c0", "c1", "c2"), "distinct columns  3, 0 ,1 of " + JOINED2),
    ("distinct_no_extension", distinct(hops=MAX_HOPS, frm="NULL", columns=f"'{MAX_HOPS}'", ext=NO_EXT), big("c0"),
     f"distinct columns {MAX_HOPS} of {MAX_HOPS}-hop walks of knows"),
    ("distinct_empty_extension", distinct(frm=7, columns="'2'", ext="'', NULL, NULL"), big("c0"),
     "distinct columns 2 of " + WALKS2),
    ("distinct_count", distinct("gg_khop_extend_distinct_count"), big("rows", "walks"), "distinct columns 0, 3 of " + JOINED2),
    ("aggregate", aggregate(), [("vertex", "BIGINT"), ("walks", "BIGINT"), ("total", "HUGEINT")],
     "count, sum(p_score) by start over " + WALKS2),
    ("aggregate_counts", aggregate(hops=MAX_HOPS, group_by="'end'", weight="NULL"),
     [("vertex", "BIGINT"), ("walks", "BIGINT"), ("total", "HUGEINT")],
     f"count by end over {MAX_HOPS}-hop walks of knows"),
    ("aggregate_top", aggregate_top(),
     [("rank", "BIGINT"), ("vertex", "BIGINT"), ("walks", "BIGINT"), ("total", "HUGEINT")],
     "top 5 by p_score + total desc of count, sum(p_score) by start over " + WALKS2),
    ("aggregate_top_walks", aggregate_top(hops=1, group_by="'end'", weight="NULL", order="'walks'", desc="false",
                                          bias="NULL", n=0),
     [("rank", "BIGINT"), ("vertex", "BIGINT"), ("walks", "BIGINT"), ("total", "HUGEINT")],
     "top 0 by walks of count by end over 1-hop walks of knows"),
    ("pair_counts", f"gg_khop_pair_counts({G}, NULL, NULL, {MAX_HOPS})", big("source", "vertex", "walks"),
     f"count by (source, end) over {MAX_HOPS}-hop walks of knows"),
    ("components", f"gg_components({G})", big("vertex", "component", "size"), "components of knows"),
    ("component_sizes", f"gg_component_sizes({G})", big("component", "size"), "component sizes of knows"),
    ("cheapest_path", f"gg_cheapest_path({G}, 'k_weight', NULL, NULL, 3)",
     [("source", "BIGINT"), ("vertex", "BIGINT"), ("cost", "BIGINT"), ("hops", "INTEGER")],
     "cheapest walks of at most 3 hops over knows weighted by k_weight"),
    ("cheapest_path_any", f"gg_cheapest_path({G}, 'k_weight', {SRC}, {SRC}, NULL)",
     [("source", "BIGINT"), ("vertex", "BIGINT"), ("cost", "BIGINT"), ("hops", "INTEGER")],
     "cheapest walks of any length over knows weighted by k_weight"),
    ("cheapest_path_rows", f"gg_cheapest_path_rows({G}, 'k_weight', {PAIRS})",
     [("src", "BIGINT"), ("dst", "BIGINT"), ("step", "INTEGER"), ("vertex", "BIGINT"), ("edge_rowid", "BIGINT"),
      ("cost", "BIGINT")], "cheapest paths over knows weighted by k_weight"),
]


@pytest.mark.parametrize("call,columns", [pytest.param(c[1], c[2], id=c[0]) for c in CALLS])
def test_result_columns(db, call, columns):
    described = db.execute_text(f"DESCRIBE SELECT * FROM {call}")
    assert [(row[0], row[1]) for row in described] == columns


def squeezed(text):
    return "".join(text.split())


def shown(plan):
    """What EXPLAIN's box shows, as patterns over text without blanks: (the operator's name, the description under it).
    The box breaks the description into lines wherever it is full and cuts a line that is still too wide, ending it in
    '...'."""
    lines = [line.strip("│ ") for line in plan.splitlines()]
    rules = [i for i, line in enumerate(lines) if line and not line.strip("─ └┘")]
    assert rules and rules[0] == 2, plan  # (the rule under the name, or the box's bottom where nothing is described)
    patterns = []
    for part in (lines[1:2], lines[3:rules[1]] if len(rules) > 1 else []):
        pattern = ""
        for line in part:
            cut = line.endswith("...")
            pattern += re.escape(squeezed(line[:-3] if cut else line)) + (".*" if cut else "")
        patterns.append(pattern)
    return patterns


@pytest.mark.parametrize("call,description", [pytest.param(c[1], c[3], id=c[0]) for c in CALLS])
def test_explain_text(db, call, description):
    plan = db.explain(f"SELECT * FROM {call}")
    name, text = shown(plan)
    assert re.fullmatch(name, call[:call.index("(")].upper()), plan
    assert re.fullmatch(text, squeezed(description or "")), plan


BINDER, INVALID = "Binder Error", "Invalid Input Error"
H, HX = f"need 1 <= hops <= {MAX_HOPS}", f"need 1 <= hops <= {MAX_HOPS - 1}"  # without / with an extension

EDGE_FILTER_NULL = "hops, from_col, to_col and mode must not be NULL"
EXTEND_NULL = "hops, ext_table, ext_key_col, ext_next_col and from_col must not be NULL"
GROUP_NULL = "hops, ext_table, ext_key_col, ext_next_col, from_col and key_col must not be NULL"
VALUE_NULL = "hops, ext_table, ext_key_col, ext_next_col, from_col, value_column and value_of must not be NULL"
DISTINCT_EXT_NULL = "ext_key_col, ext_next_col and from_col must not be NULL where ext_table is given"
TOP_NULL = "hops, group_by, order_by, descending and n must not be NULL"

# (id, the call, the exception's class, the function the message names, the fragment that names the argument)
REFUSALS = [
    ("khop_k_min_0", f"gg_khop({G}, 0, 2)", BINDER, "gg", f"need 1 <= k_min <= k_max <= {MAX_HOPS}"),
    ("khop_k_max_past", f"gg_khop({G}, 1, {MAX_HOPS + 1})", BINDER, "gg", f"need 1 <= k_min <= k_max <= {MAX_HOPS}"),
    ("khop_count_k_min_above", f"gg_khop_count({G}, 3, 2)", BINDER, "gg", f"need 1 <= k_min <= k_max <= {MAX_HOPS}"),
    ("same_neighbour_hops_0", "gg_same_neighbour_paths('SELECT 1', 'SELECT 1', 'knows', 'k_person1id', 'k_person2id', "
     "'knows', 'k_person2id', 'k_person1id', 0)", BINDER, "gg_same_neighbour_paths", HX),
    ("same_neighbour_hops_past", "gg_same_neighbour_paths('SELECT 1', 'SELECT 1', 'knows', 'k_person1id', 'k_person2id', "
     f"'knows', 'k_person2id', 'k_person1id', {MAX_HOPS})", BINDER, "gg_same_neighbour_paths", HX),
    ("all_shortest_path_limit_negative", f"gg_all_shortest_path_rows({G}, {PAIRS}, 3, -1)", INVALID,
     "gg_all_shortest_path_rows", "path_limit must be >= 0 (0: every path)"),
    # gg_khop_edge_filter
    ("edge_filter_hops_null", edge_filter(hops="NULL"), BINDER, "gg_khop_edge_filter", EDGE_FILTER_NULL),
    ("edge_filter_from_null", edge_filter(frm="NULL"), BINDER, "gg_khop_edge_filter", EDGE_FILTER_NULL),
    ("edge_filter_to_null", edge_filter(to="NULL"), BINDER, "gg_khop_edge_filter", EDGE_FILTER_NULL),
    ("edge_filter_mode_null", edge_filter(mode="NULL"), BINDER, "gg_khop_edge_filter", EDGE_FILTER_NULL),
    ("edge_filter_count_hops_null", edge_filter("gg_khop_edge_filter_count", hops="NULL"), BINDER,
     "gg_khop_edge_filter_count", EDGE_FILTER_NULL),
    ("edge_filter_hops_0", edge_filter(hops=0, frm=0), BINDER, "gg_khop_edge_filter", H),
    ("edge_filter_hops_past", edge_filter(hops=MAX_HOPS + 1), BINDER, "gg_khop_edge_filter", H),
    ("edge_filter_count_hops_past", edge_filter("gg_khop_edge_filter_count", hops=MAX_HOPS + 1), BINDER,
     "gg_khop_edge_filter_count", H),
    ("edge_filter_from_negative", edge_filter(frm=-1), BINDER, "gg_khop_edge_filter", "from_col and to_col must lie in 0..2"),
    ("edge_filter_from_past", edge_filter(frm=3), BINDER, "gg_khop_edge_filter", "from_col and to_col must lie in 0..2"),
    ("edge_filter_to_negative", edge_filter(to=-1), BINDER, "gg_khop_edge_filter", "from_col and to_col must lie in 0..2"),
    ("edge_filter_to_past", edge_filter(to=3), BINDER, "gg_khop_edge_filter", "from_col and to_col must lie in 0..2"),
    ("edge_filter_mode_unknown", edge_filter(mode="'outer'"), BINDER, "gg_khop_edge_filter",
     "mode 'outer' (one of 'inner', 'semi', 'anti')"),
    ("edge_filter_count_mode_unknown", edge_filter("gg_khop_edge_filter_count", mode="''"), BINDER,
     "gg_khop_edge_filter_count", "mode '' (one of 'inner', 'semi', 'anti')"),
    # gg_khop_extend
    ("extend_hops_null", extend(hops="NULL"), BINDER, "gg_khop_extend", EXTEND_NULL),
    ("extend_table_null", extend(ext="NULL, 'm_creatorid', 'm_messageid'"), BINDER, "gg_khop_extend", EXTEND_NULL),
    ("extend_key_null", extend(ext="'message', NULL, 'm_messageid'"), BINDER, "gg_khop_extend", EXTEND_NULL),
    ("extend_next_null", extend(ext="'message', 'm_creatorid', NULL"), BINDER, "gg_khop_extend", EXTEND_NULL),
    ("extend_from_null", extend(frm="NULL"), BINDER, "gg_khop_extend", EXTEND_NULL),
    ("extend_count_from_null", extend("gg_khop_extend_count", frm="NULL"), BINDER, "gg_khop_extend_count", EXTEND_NULL),
    ("extend_hops_0", extend(hops=0, frm=0), BINDER, "gg_khop_extend", HX),
    ("extend_hops_past", extend(hops=MAX_HOPS), BINDER, "gg_khop_extend", HX),
    ("extend_count_hops_past", extend("gg_khop_extend_count", hops=MAX_HOPS), BINDER, "gg_khop_extend_count", HX),
    ("extend_from_negative", extend(frm=-1), BINDER, "gg_khop_extend", "from_col must lie in 0..2"),
    ("extend_from_past", extend(frm=3), BINDER, "gg_khop_extend", "from_col must lie in 0..2"),
    ("extend_count_from_past", extend("gg_khop_extend_count", hops=1, frm=2), BINDER, "gg_khop_extend_count",
     "from_col must lie in 0..1"),
    # gg_khop_extend_group
    ("group_hops_null", group(hops="NULL"), BINDER, "gg_khop_extend_group", GROUP_NULL),
    ("group_table_null", group(ext="NULL, 'm_creatorid', 'm_messageid'"), BINDER, "gg_khop_extend_group", GROUP_NULL),
    ("group_key_col_null_ext", group(ext="'message', NULL, 'm_messageid'"), BINDER, "gg_khop_extend_group", GROUP_NULL),
    ("group_next_null", group(ext="'message', 'm_creatorid', NULL"), BINDER, "gg_khop_extend_group", GROUP_NULL),
    ("group_from_null", group(frm="NULL"), BINDER, "gg_khop_extend_group", GROUP_NULL),
    ("group_key_null", group(key="NULL"), BINDER, "gg_khop_extend_group", GROUP_NULL),
    ("group_hops_0", group(hops=0, frm=0, key=0), BINDER, "gg_khop_extend_group", HX),
    ("group_hops_past", group(hops=MAX_HOPS), BINDER, "gg_khop_extend_group", HX),
    ("group_from_negative", group(frm=-1), BINDER, "gg_khop_extend_group", "from_col must lie in 0..2"),
    ("group_from_past", group(frm=3), BINDER, "gg_khop_extend_group", "from_col must lie in 0..2"),
    ("group_key_negative", group(key=-1), BINDER, "gg_khop_extend_group", "key_col must lie in 0..3"),
    ("group_key_past", group(key=4), BINDER, "gg_khop_extend_group", "key_col must lie in 0..3"),
    ("group_n_negative", group(n=-1), BINDER, "gg_khop_extend_group", "n must not be negative"),
    # gg_khop_extend_filter / _filter_count / _top
    ("filter_hops_null", value_rows(hops="NULL"), BINDER, "gg_khop_extend_filter", VALUE_NULL),
    ("filter_table_null", value_rows(ext="NULL, 'm_creatorid', 'm_messageid'"), BINDER, "gg_khop_extend_filter", VALUE_NULL),
    ("filter_key_null", value_rows(ext="'message', NULL, 'm_messageid'"), BINDER, "gg_khop_extend_filter", VALUE_NULL),
    ("filter_next_null", value_rows(ext="'message', 'm_creatorid', NULL"), BINDER, "gg_khop_extend_filter", VALUE_NULL),
    ("filter_from_null", value_rows(frm="NULL"), BINDER, "gg_khop_extend_filter", VALUE_NULL),
    ("filter_column_null", value_rows(column="NULL"), BINDER, "gg_khop_extend_filter", VALUE_NULL),
    ("filter_value_of_null", value_rows(of="NULL"), BINDER, "gg_khop_extend_filter", VALUE_NULL),
    ("filter_count_value_of_null", value_rows("gg_khop_extend_filter_count", of="NULL"), BINDER,
     "gg_khop_extend_filter_count", VALUE_NULL),
    ("top_column_null", top_rows(column="NULL"), BINDER, "gg_khop_extend_top", VALUE_NULL),
    ("filter_hops_0", value_rows(hops=0, frm=0, of=0), BINDER, "gg_khop_extend_filter", HX),
    ("filter_hops_past", value_rows(hops=MAX_HOPS), BINDER, "gg_khop_extend_filter", HX),
    ("filter_count_hops_past", value_rows("gg_khop_extend_filter_count", hops=MAX_HOPS), BINDER,
     "gg_khop_extend_filter_count", HX),
    ("top_hops_0", top_rows(hops=0, frm=0, of=0, tie=0), BINDER, "gg_khop_extend_top", HX),
    ("filter_from_negative", value_rows(frm=-1), BINDER, "gg_khop_extend_filter", "from_col must lie in 0..2"),
    ("filter_from_past", value_rows(frm=3), BINDER, "gg_khop_extend_filter", "from_col must lie in 0..2"),
    ("top_from_past", top_rows(frm=3), BINDER, "gg_khop_extend_top", "from_col must lie in 0..2"),
    ("filter_value_of_negative", value_rows(of=-1), BINDER, "gg_khop_extend_filter", "value_of must lie in 0..3"),
    ("filter_value_of_past", value_rows(of=4), BINDER, "gg_khop_extend_filter", "value_of must lie in 0..3"),
    ("filter_count_value_of_past", value_rows("gg_khop_extend_filter_count", of=4), BINDER,
     "gg_khop_extend_filter_count", "value_of must lie in 0..3"),
    ("top_value_of_negative", top_rows(of=-1), BINDER, "gg_khop_extend_top", "value_of must lie in 0..3"),
    ("top_tie_negative", top_rows(tie=-1), BINDER, "gg_khop_extend_top", "tie_col must be NULL or lie in 0..3"),
    ("top_tie_past", top_rows(tie=4), BINDER, "gg_khop_extend_top", "tie_col must be NULL or lie in 0..3"),
    ("top_n_negative", top_rows(n=-1), BINDER, "gg_khop_extend_top", "n must not be negative"),
    # gg_khop_extend_distinct
    ("distinct_hops_null", distinct(hops="NULL"), BINDER, "gg_khop_extend_distinct", "hops must not be NULL"),
    ("distinct_count_hops_null", distinct("gg_khop_extend_distinct_count", hops="NULL"), BINDER,
     "gg_khop_extend_distinct_count", "hops must not be NULL"),
    ("distinct_key_null", distinct(ext="'message', NULL, 'm_messageid'"), BINDER, "gg_khop_extend_distinct", DISTINCT_EXT_NULL),
    ("distinct_next_null", distinct(ext="'message', 'm_creatorid', NULL"), BINDER, "gg_khop_extend_distinct", DISTINCT_EXT_NULL),
    ("distinct_from_null", distinct(frm="NULL"), BINDER, "gg_khop_extend_distinct", DISTINCT_EXT_NULL),
    ("distinct_hops_0", distinct(hops=0, frm=0, columns="'0'"), BINDER, "gg_khop_extend_distinct", HX),
    ("distinct_hops_past_extended", distinct(hops=MAX_HOPS), BINDER, "gg_khop_extend_distinct", HX),
    ("distinct_hops_0_plain", distinct(hops=0, columns="'0'", ext=NO_EXT), BINDER, "gg_khop_extend_distinct", H),
    ("distinct_hops_past_plain", distinct(hops=MAX_HOPS + 1, ext=NO_EXT), BINDER, "gg_khop_extend_distinct", H),
    ("distinct_count_hops_past_plain", distinct("gg_khop_extend_distinct_count", hops=MAX_HOPS + 1, ext=NO_EXT), BINDER,
     "gg_khop_extend_distinct_count", H),
    ("distinct_from_negative", distinct(frm=-1), BINDER, "gg_khop_extend_distinct", "from_col must lie in 0..2"),
    ("distinct_from_past", distinct(frm=3), BINDER, "gg_khop_extend_distinct", "from_col must lie in 0..2"),
    ("distinct_columns_null", distinct(columns="NULL"), INVALID, "gg_khop_extend_distinct", "columns must not be NULL"),
    ("distinct_columns_empty", distinct(columns="' '"), INVALID, "gg_khop_extend_distinct", "columns: an empty list"),
    ("distinct_columns_no_number", distinct(columns="'0, x'"), INVALID, "gg_khop_extend_distinct",
     "columns: a column number is expected at position 3 of '0, x'"),
    ("distinct_columns_no_comma", distinct(columns="'0 1'"), INVALID, "gg_khop_extend_distinct",
     "columns: a comma is expected at position 2 of '0 1'"),
    ("distinct_columns_trailing_comma", distinct(columns="'0,'"), INVALID, "gg_khop_extend_distinct",
     "columns: a column number is expected at position 2 of '0,'"),
    ("distinct_columns_repeated", distinct(columns="'1, 3, 1'"), INVALID, "gg_khop_extend_distinct",
     "columns: column 1 is listed twice in '1, 3, 1'"),
    ("distinct_columns_past_extended", distinct(columns="'4'"), INVALID, "gg_khop_extend_distinct",
     "columns: a column outside 0..3 in '4'"),
    ("distinct_columns_past_plain", distinct(columns="'3'", ext=NO_EXT), INVALID, "gg_khop_extend_distinct",
     "columns: a column outside 0..2 in '3'"),
    ("distinct_count_columns_repeated", distinct("gg_khop_extend_distinct_count", columns="'2,2'"), INVALID,
     "gg_khop_extend_distinct_count", "columns: column 2 is listed twice in '2,2'"),
    # gg_khop_aggregate / _top
    ("aggregate_hops_null", aggregate(hops="NULL"), BINDER, "gg_khop_aggregate", "hops and group_by must not be NULL"),
    ("aggregate_group_null", aggregate(group_by="NULL"), BINDER, "gg_khop_aggregate", "hops and group_by must not be NULL"),
    ("aggregate_hops_0", aggregate(hops=0), BINDER, "gg_khop_aggregate", H),
    ("aggregate_hops_past", aggregate(hops=MAX_HOPS + 1), BINDER, "gg_khop_aggregate", H),
    ("aggregate_group_unknown", aggregate(group_by="'middle'"), BINDER, "gg_khop_aggregate",
     "group_by 'middle' (one of 'start', 'end')"),
    ("aggregate_top_hops_null", aggregate_top(hops="NULL"), BINDER, "gg_khop_aggregate_top", TOP_NULL),
    ("aggregate_top_group_null", aggregate_top(group_by="NULL"), BINDER, "gg_khop_aggregate_top", TOP_NULL),
    ("aggregate_top_order_null", aggregate_top(order="NULL"), BINDER, "gg_khop_aggregate_top", TOP_NULL),
    ("aggregate_top_descending_null", aggregate_top(desc="NULL::BOOLEAN"), BINDER, "gg_khop_aggregate_top", TOP_NULL),
    ("aggregate_top_n_null", aggregate_top(n="NULL"), BINDER, "gg_khop_aggregate_top", TOP_NULL),
    ("aggregate_top_hops_0", aggregate_top(hops=0), BINDER, "gg_khop_aggregate_top", H),
    ("aggregate_top_hops_past", aggregate_top(hops=MAX_HOPS + 1), BINDER, "gg_khop_aggregate_top", H),
    ("aggregate_top_n_negative", aggregate_top(n=-1), BINDER, "gg_khop_aggregate_top", "n must not be negative"),
    ("aggregate_top_group_unknown", aggregate_top(group_by="'both'"), BINDER, "gg_khop_aggregate_top",
     "group_by 'both' (one of 'start', 'end')"),
    ("aggregate_top_order_unknown", aggregate_top(order="'size'"), BINDER, "gg_khop_aggregate_top",
     "order_by 'size' (one of 'total', 'walks')"),
    ("aggregate_top_bias_by_walks", aggregate_top(order="'walks'"), BINDER, "gg_khop_aggregate_top",
     "a bias_column is added to the total only"),
    # gg_khop_pair_counts
    ("pair_counts_hops_null", f"gg_khop_pair_counts({G}, NULL, NULL, NULL)", BINDER, "gg_khop_pair_counts",
     "hops must not be NULL"),
    ("pair_counts_hops_0", f"gg_khop_pair_counts({G}, NULL, NULL, 0)", BINDER, "gg_khop_pair_counts", H),
    ("pair_counts_hops_past", f"gg_khop_pair_counts({G}, {SRC}, {SRC}, {MAX_HOPS + 1})", BINDER, "gg_khop_pair_counts", H),
    # gg_cheapest_path / _rows
    ("cheapest_weight_null", f"gg_cheapest_path({G}, NULL, NULL, NULL, 3)", BINDER, "gg_cheapest_path",
     "weight_column must not be NULL"),
    ("cheapest_rows_weight_null", f"gg_cheapest_path_rows({G}, NULL, {PAIRS})", BINDER, "gg_cheapest_path_rows",
     "weight_column and pairs_sql must not be NULL"),
    ("cheapest_rows_pairs_null", f"gg_cheapest_path_rows({G}, 'k_weight', NULL)", BINDER, "gg_cheapest_path_rows",
     "weight_column and pairs_sql must not be NULL"),
]
# gg_components / gg_component_sizes: every one of the five names
for _fn in ("gg_components", "gg_component_sizes"):
    for _i, _name in enumerate(("vertex_table", "vertex_key", "edge_table", "src_col", "dst_col")):
        _args = G.split(", ")
        _args[_i] = "NULL"
        REFUSALS.append((f"{_fn[3:]}_{_name}_null", f"{_fn}({', '.join(_args)})", BINDER, _fn,
                         "table and column names must not be NULL"))


@pytest.mark.parametrize("call,kind,fn,fragment", [pytest.param(*r[1:], id=r[0]) for r in REFUSALS])
def test_bind_refusals(db, call, kind, fn, fragment):
    with pytest.raises(RuntimeError) as raised:  # (EXPLAIN binds like the statement itself and never opens the scan)
        db.explain(f"SELECT * FROM {call}")
    assert f"{kind}: {fn}: {fragment}" in str(raised.value)
