"""The bind step of gg_khop_extend_group_columns (duckdb_pgq_amd/host/gg_group_tuples.cpp), CPU part, in the manner of
tests/test_table_function_binds.py: the result columns of a well-formed call, the description EXPLAIN prints, and every
refusal the bind makes.  DESCRIBE, EXPLAIN and a failing bind need no GPU; result parity is in
tests/test_gpu_group_tuples_sql.py (-m gpu)."""
import os
import re

import pytest

from oracle import ref_duckdb as R
from tests.test_table_function_binds import (BINDER, DISTINCT_EXT_NULL, G, H, HX, INVALID, JOINED2, MAX_HOPS, NO_EXT, WALKS2, X,
                                             big, extend, shown, squeezed)

EXT = R.EXTENSION

pytestmark = pytest.mark.skipif(
    not (R.available() and os.path.exists(EXT) and bool(R.rules_route())),
    reason="reference build / extension / plan hook not present")

FN = "gg_khop_extend_group_columns"
AGGREGATES = big("rows", "valued") + [("sum", "HUGEINT")] + big("min", "max")


@pytest.fixture(scope="module")
def db():
    d = R.RefDuckDB(threads=2)
    d.execute("CREATE TABLE person (p_personid BIGINT PRIMARY KEY, p_score BIGINT)")
    d.execute("CREATE TABLE knows (k_person1id BIGINT NOT NULL, k_person2id BIGINT NOT NULL, k_weight INTEGER)")
    d.execute("CREATE TABLE message (m_messageid BIGINT NOT NULL, m_creatorid BIGINT NOT NULL, m_date BIGINT)")
    d.execute(f"LOAD '{EXT}'")
    yield d
    d.close()


def group_columns(hops=2, frm=2, columns="'0, 3'", column="'m_date'", of=3, ext=X):
    return extend(FN, hops, frm, f", {columns}, {column}, {of}", ext)


# (id, the call, its result columns, the description under the operator's name in EXPLAIN)
CALLS = [
    ("valued", group_columns(), big("k0", "k1") + AGGREGATES, "groups by columns 0, 3 of " + JOINED2 + ", m_date of column 3"),
    ("one_column", group_columns(columns="'3'", column="'p_score'", of=0), big("k0") + AGGREGATES,
     "groups by columns 3 of " + JOINED2 + ", p_score of column 0"),
    ("count_form", group_columns(columns="' 3, 0 ,1'", column="NULL", of="NULL"), big("k0", "k1", "k2") + AGGREGATES,
     "groups by columns  3, 0 ,1 of " + JOINED2 + ", counted"),
    ("count_form_value_of_ignored", group_columns(column="NULL", of=99), big("k0", "k1") + AGGREGATES,
     "groups by columns 0, 3 of " + JOINED2 + ", counted"),
    ("no_extension", group_columns(hops=MAX_HOPS, frm="NULL", columns=f"'{MAX_HOPS}, 0'", column="'p_score'", of=MAX_HOPS, ext=NO_EXT),
     big("k0", "k1") + AGGREGATES,
     f"groups by columns {MAX_HOPS}, 0 of {MAX_HOPS}-hop walks of knows, p_score of column {MAX_HOPS}"),
    ("empty_extension", group_columns(frm=7, columns="'2'", column="NULL", of="NULL", ext="'', NULL, NULL"), big("k0") + AGGREGATES,
     "groups by columns 2 of " + WALKS2 + ", counted"),
    ("all_columns", group_columns(hops=MAX_HOPS - 1, frm=0, columns="'" + ", ".join(str(c) for c in range(MAX_HOPS + 1)) + "'"),
     big(*[f"k{c}" for c in range(MAX_HOPS + 1)]) + AGGREGATES, None),
]


@pytest.mark.parametrize("call,columns", [pytest.param(c[1], c[2], id=c[0]) for c in CALLS])
def test_result_columns(db, call, columns):
    described = db.execute_text(f"DESCRIBE SELECT * FROM {call}")
    assert [(row[0], row[1]) for row in described] == columns


@pytest.mark.parametrize("call,description", [pytest.param(c[1], c[3], id=c[0]) for c in CALLS if c[3]])
def test_explain_text(db, call, description):
    plan = db.explain(f"SELECT * FROM {call}")
    name, text = shown(plan)
    assert re.fullmatch(name, FN.upper()), plan
    assert re.fullmatch(text, squeezed(description)), plan


# (id, the call, the exception's class, the fragment that names the argument)
REFUSALS = [
    ("hops_null", group_columns(hops="NULL"), BINDER, "hops must not be NULL"),
    ("key_null", group_columns(ext="'message', NULL, 'm_messageid'"), BINDER, DISTINCT_EXT_NULL),
    ("next_null", group_columns(ext="'message', 'm_creatorid', NULL"), BINDER, DISTINCT_EXT_NULL),
    ("from_null", group_columns(frm="NULL"), BINDER, DISTINCT_EXT_NULL),
    ("hops_0", group_columns(hops=0, frm=0, columns="'0'", of=0), BINDER, HX),
    ("hops_past_extended", group_columns(hops=MAX_HOPS), BINDER, HX),
    ("hops_0_plain", group_columns(hops=0, columns="'0'", of=0, ext=NO_EXT), BINDER, H),
    ("hops_past_plain", group_columns(hops=MAX_HOPS + 1, ext=NO_EXT), BINDER, H),
    ("from_negative", group_columns(frm=-1), BINDER, "from_col must lie in 0..2"),
    ("from_past", group_columns(frm=3), BINDER, "from_col must lie in 0..2"),
    ("columns_null", group_columns(columns="NULL"), INVALID, "columns must not be NULL"),
    ("columns_empty", group_columns(columns="' '"), INVALID, "columns: an empty list"),
    ("columns_no_number", group_columns(columns="'0, x'"), INVALID, "columns: a column number is expected at position 3 of '0, x'"),
    ("columns_no_comma", group_columns(columns="'0 1'"), INVALID, "columns: a comma is expected at position 2 of '0 1'"),
    ("columns_repeated", group_columns(columns="'1, 3, 1'"), INVALID, "columns: column 1 is listed twice in '1, 3, 1'"),
    ("columns_past_extended", group_columns(columns="'4'"), INVALID, "columns: a column outside 0..3 in '4'"),
    ("columns_past_plain", group_columns(columns="'3'", of=2, ext=NO_EXT), INVALID, "columns: a column outside 0..2 in '3'"),
    ("value_of_null", group_columns(of="NULL"), BINDER, "value_of must not be NULL where value_column is given"),
    ("value_of_negative", group_columns(of=-1), BINDER, "value_of must lie in 0..3"),
    ("value_of_past_extended", group_columns(of=4), BINDER, "value_of must lie in 0..3"),
    ("value_of_past_plain", group_columns(columns="'0'", of=3, ext=NO_EXT), BINDER, "value_of must lie in 0..2"),
]


@pytest.mark.parametrize("call,kind,fragment", [pytest.param(*r[1:], id=r[0]) for r in REFUSALS])
def test_bind_refusals(db, call, kind, fragment):
    with pytest.raises(RuntimeError) as raised:  # (EXPLAIN binds like the statement itself and never opens the scan)
        db.explain(f"SELECT * FROM {call}")
    assert f"{kind}: {FN}: {fragment}" in str(raised.value)
