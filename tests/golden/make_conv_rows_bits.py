"""Record tests/golden/conv_rows_bits.json: the SHA-256 of every output of every case of
tests/test_gpu_conv_rows.py, computed by the built library on an MI355X. The cases are run through the test's
own functions (run_case), so each is also held to the oracle and to its bitwise identities while it is recorded.

The table is self-referential ("pinned_to"): it pins the row-streaming conv kernels bit for bit across a
refactor -- record it from the library of the commit before the change, and tests/test_gpu_conv_rows.py holds
every later library to it. The kernels are deterministic (fixed summation orders), so two recordings in separate
processes must be identical. "stats_41_equal_44" records whether the statistics of k_conv_rows<4,1,0,0,1> (summed
through LDS) came out bitwise those of <4,4,0,0,1> (summed from registers) over the same channels; the test does
not assert it.

Run (after building the library):  python tests/golden/make_conv_rows_bits.py [OUT.json]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
TABLE = os.path.join(HERE, "conv_rows_bits.json")


def record():
    sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
    import test_gpu_conv_rows as t
    cases = {name: t.run_case(name) for name in t.CASES}
    return {"pinned_to": "self: the library that recorded it (tests/golden/make_conv_rows_bits.py)",
            "stats_41_equal_44": t.stats_41_equal_44, "cases": cases}


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else TABLE
    table = record()
    with open(out, "w") as fh:
        fh.write('{\n"pinned_to": %s,\n"stats_41_equal_44": %s,\n"cases": {\n' % (
            json.dumps(table["pinned_to"]), json.dumps(table["stats_41_equal_44"])))
        fh.write(",\n".join('"%s": %s' % (k, json.dumps(v, sort_keys=True)) for k, v in table["cases"].items()))
        fh.write("\n}\n}\n")
    print(len(table["cases"]), "cases ->", out)
