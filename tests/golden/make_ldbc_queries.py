#!/usr/bin/env python3
"""Extract the reference's LDBC texts — benchmark/ldbc/schema.sql and every benchmark/ldbc/queries/*.sql — into
tests/golden/ldbc_queries.json, so that tests/test_plan_rule.py::test_the_references_ldbc_queries_get_gpu_operators
plans the query files as shipped without reading the reference tree.

The texts are DATA: stored byte for byte, keyed by file name.

    python3 tests/golden/make_ldbc_queries.py [REFERENCE_ROOT]     (rewrites the json)
"""
import json
import os
import sys

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ldbc_queries.json")


def main():
    ldbc = os.path.join(REF, "benchmark", "ldbc")
    qdir = os.path.join(ldbc, "queries")
    data = {"source": "benchmark/ldbc/schema.sql and benchmark/ldbc/queries/*.sql of the reference",
            "schema.sql": open(os.path.join(ldbc, "schema.sql")).read(),
            "queries": {name: open(os.path.join(qdir, name)).read() for name in sorted(os.listdir(qdir))
                        if name.endswith(".sql")}}
    with open(OUT, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{OUT}: schema + {len(data['queries'])} queries")


if __name__ == "__main__":
    main()
