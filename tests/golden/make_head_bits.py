"""Record tests/golden/head_bits.json: the SHA-256 of every output of every case of tests/test_gpu_head_bits.py,
computed by the built library on an MI355X. The cases are run through the test's own functions (run_case), so
each is also held to the oracle and to its bitwise identities while it is recorded.

The table pins the 1x1 head kernels bit for bit across a refactor: record it from the library of the commit
before the change, and tests/test_gpu_head_bits.py holds every later library to it. The kernels are deterministic
(fixed summation orders), so two recordings in separate processes must be identical.

Run (after building the library):  python tests/golden/make_head_bits.py [OUT.json]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
TABLE = os.path.join(HERE, "head_bits.json")


def record():
    sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
    import test_gpu_head_bits as t
    return {name: t.run_case(name) for name in t.CASES}


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else TABLE
    table = record()
    with open(out, "w") as fh:
        fh.write("{\n" + ",\n".join('"%s": %s' % (k, json.dumps(v, sort_keys=True)) for k, v in table.items()) + "\n}\n")
    print(len(table), "cases ->", out)
