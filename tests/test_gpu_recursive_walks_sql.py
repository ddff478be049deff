"""UNION ALL recursive CTEs run as GG_RECURSIVE_WALKS (the walk closure on the GPU) and give the relation the
reference's PhysicalRecursiveCTE gives: the shipped bi-9.sql and interactive-short-6.sql texts over a populated LDBC
database with comment chains (m_c_parentcommentid) more than 12 deep, their CTEs alone, a depth-counter CTE with
`hop < K`, and a chain that ends in a NULL m_c_replyof.  Statements with ORDER BY are compared in order.

In tests/ldbc_shapes.py `message` is the schema's VIEW, a UNION ALL of post and comment; the reference refuses to run
a recursive arm over it ("UNIONS are not supported in recursive CTEs yet").  The rules-off runs therefore read a database
where `message` is a table with the view's rows; the device plan runs over both, and its result over the view is
compared with the reference's over the table."""
import os

import pytest

from oracle import ref_duckdb as R
from tests import ldbc_shapes
from tests.test_plan_rule import _ldbc_texts

EXT = R.EXTENSION

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not (R.available() and os.path.exists(EXT) and R.rules_route() == "shim"),
                       reason="reference build / extension / interposition shim not present"),
]

POST = 5000                 # a post of June 2012 with comment chains under it
SHORT6_COMMENT = 687194767741  # the comment interactive-short-6.sql starts from
JUNE = "2012-06-15 10:00:00"


def _populate(d, message_table):
    ids = ldbc_shapes.populate(d)
    creator = [int(ids[i % len(ids)]) for i in range(64)]
    d.execute(f"INSERT INTO post VALUES ('{JUNE}', {POST}, NULL, 'ip', 'br', 'en', 'thread', 6, {creator[0]}, 1000, 1)")
    rows = []

    def chain(first_id, parent_post, parent_comment, depth, k):
        prev_post, prev_comment = parent_post, parent_comment
        for j in range(depth):
            cid = first_id + j
            rows.append(f"('{JUNE}', {cid}, 'ip', 'br', 'reply', 5, {creator[(k + j) % 64]}, 1, "
                        f"{'NULL' if prev_post is None else prev_post}, {'NULL' if prev_comment is None else prev_comment})")
            prev_post, prev_comment = None, cid
        return first_id + depth - 1

    last = chain(700000, POST, None, 13, 1)        # 13 deep
    chain(710000, None, 700003, 15, 2)             # 19 deep, branching off the first chain
    chain(720000, None, 700003, 4, 3)              # a second branch at the same comment
    chain(730000, 10_000, None, 12, 4)             # under a post of the populated tables (any month)
    rows.append(f"('{JUNE}', {SHORT6_COMMENT}, 'ip', 'br', 'start', 5, {creator[5]}, 1, NULL, {last})")
    d.execute("INSERT INTO comment VALUES " + ", ".join(rows))
    if message_table:
        d.execute("CREATE TABLE message_rows AS SELECT * FROM message")
        d.execute("DROP VIEW message")
        d.execute("ALTER TABLE message_rows RENAME TO message")


def _open(message_table):
    d = R.RefDuckDB(threads=4)
    _populate(d, message_table)
    d.execute(f"LOAD '{EXT}'")
    return d


@pytest.fixture(scope="module")
def db():
    d = _open(True)
    yield d
    d.execute("PRAGMA disable_gpu_graph")
    d.close()


@pytest.fixture(scope="module")
def db_view():
    d = _open(False)
    yield d
    d.execute("PRAGMA disable_gpu_graph")
    d.close()


def _text(name):
    return _ldbc_texts()["queries"][name].strip().rstrip(";")


def _cte_alone(name, cte):
    text = _text(name)
    head = text[:text.index("\n)\n") + 3] if "\n)\n" in text else text[:text.rindex(")") + 1] + "\n"
    return head + f"SELECT * FROM {cte}"


STATEMENTS = {
    "bi-9": (_text("bi-9.sql"), True),
    "interactive-short-6": (_text("interactive-short-6.sql"), False),
    "post_all alone": (None, False),
    "chain alone (ends in a NULL m_c_replyof)": (None, False),
    "chained pair of recursive CTEs": ("WITH RECURSIVE a(id) AS (SELECT m_messageid FROM message WHERE m_messageid = "
                                       f"{POST} UNION ALL SELECT m_messageid FROM message, a WHERE m_c_replyof = a.id), "
                                       "b(id, hop) AS (SELECT id, 0 FROM a UNION ALL SELECT m_messageid, b.hop + 1 "
                                       "FROM message, b WHERE m_c_replyof = b.id) SELECT * FROM b", False),
    "anchor another rule would take": ("WITH RECURSIVE r(id, hop) AS (SELECT k2.k_person2id, 0 FROM knows k1, knows k2 "
                                       f"WHERE k1.k_person1id = {ldbc_shapes.PERSON_A} AND k1.k_person2id = k2.k_person1id "
                                       "UNION ALL SELECT k.k_person2id, r.hop + 1 FROM knows k, r "
                                       "WHERE k.k_person1id = r.id AND r.hop < 1) SELECT * FROM r", False),
    "depth counter": ("WITH RECURSIVE r(root, hop, id) AS (SELECT m_messageid, 0, m_messageid FROM message "
                      f"WHERE m_messageid = {POST} UNION ALL SELECT r.root, r.hop + 1, m_messageid FROM message, r "
                      "WHERE m_c_replyof = r.id AND r.hop < 9) SELECT * FROM r", False),
    "depth counter, seeds from every post": ("WITH RECURSIVE r(root, hop, id) AS (SELECT m_messageid, 0, m_messageid "
                                             "FROM post UNION ALL SELECT r.root, r.hop + 1, m_messageid FROM message, r "
                                             "WHERE m_c_replyof = r.id AND r.hop < 16) "
                                             "SELECT hop, count(*), sum(id) FROM r GROUP BY hop ORDER BY hop", True),
}


def _sql(name):
    sql, ordered = STATEMENTS[name]
    if name == "post_all alone":
        sql = _cte_alone("bi-9.sql", "post_all")
    elif name.startswith("chain alone"):
        sql = _cte_alone("interactive-short-6.sql", "chain")
    return sql, ordered


@pytest.mark.parametrize("name", list(STATEMENTS))
def test_rules_off_and_on_give_the_same_relation(db, name):
    sql, ordered = _sql(name)
    db.execute("PRAGMA disable_gpu_graph")
    assert "GG_RECURSIVE_WALKS" not in db.explain(sql)
    cpu = db.execute_text(sql)
    db.execute("PRAGMA enable_gpu_graph")
    assert "GG_RECURSIVE_WALKS" in db.explain(sql), name
    gpu = db.execute_text(sql)
    db.execute("PRAGMA disable_gpu_graph")
    assert len(cpu) > 0, name
    if ordered:
        assert gpu == cpu, name
    else:
        key = lambda row: tuple("" if v is None else v for v in row)  # noqa: E731
        assert sorted(gpu, key=key) == sorted(cpu, key=key), name


# (the chained pair's first CTE is planned under the walk sinks with the rules suspended: it stays the reference's
#  recursive CTE, which refuses the view in its arm — as it does with the rules off)
@pytest.mark.parametrize("name", [n for n in STATEMENTS if not n.startswith("chained")])
def test_over_the_message_view(db, db_view, name):
    """the arm's table is the VIEW (a UNION ALL of two projected scans, the date filter pushed into both): planned by
    the reference's planner under the table sink, the closure gives what the reference gives over the same rows"""
    sql, ordered = _sql(name)
    db.execute("PRAGMA disable_gpu_graph")
    cpu = db.execute_text(sql)
    db_view.execute("PRAGMA enable_gpu_graph")
    assert "GG_RECURSIVE_WALKS" in db_view.explain(sql), name
    gpu = db_view.execute_text(sql)
    db_view.execute("PRAGMA disable_gpu_graph")
    if ordered:
        assert gpu == cpu, name
    else:
        key = lambda row: tuple("" if v is None else v for v in row)  # noqa: E731
        assert sorted(gpu, key=key) == sorted(cpu, key=key), name


def test_the_data_has_the_depths_it_claims(db):
    """the chains reach more than 12 levels below their post, and the chain of interactive-short-6 ends in a NULL"""
    sql, _ = _sql("depth counter")
    db.execute("PRAGMA disable_gpu_graph")
    assert max(int(r[1]) for r in db.execute_text(sql)) >= 9
    rows = db.execute_text(_sql("chain alone (ends in a NULL m_c_replyof)")[0])
    assert len(rows) >= 14 and any(r[0] is None for r in rows)
    rows = db.execute_text("WITH RECURSIVE r(hop, id) AS (SELECT 0, m_messageid FROM message WHERE m_messageid = "
                           f"{POST} UNION ALL SELECT r.hop + 1, m_messageid FROM message, r WHERE m_c_replyof = r.id) "
                           "SELECT max(hop) FROM r")
    assert int(rows[0][0]) >= 12
