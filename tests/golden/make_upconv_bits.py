"""Record tests/golden/upconv_bits.json: the SHA-256 of every output of every case of
tests/test_gpu_upconv_forms.py, computed by the built library on an MI355X. The cases are run through the test's
own functions (run_case), so each is also held to the oracle and to its bitwise identities while it is recorded.

The table is self-referential ("pinned_to"): it pins the upconv3 kernels, forward and gradients, bit for bit
across a refactor -- record it from the library of the commit before the change, and
tests/test_gpu_upconv_forms.py holds every later library to it. The kernels are deterministic (fixed summation
orders, no atomics), so two recordings in separate processes must be identical. "identities" records, for the
cases whose c_a is no whole number of staging chunks, whether the pooled call came out bitwise the call on the
dense pulled map ("dense") and on the materialised concat ("concat"); the test does not assert either.

Run (after building the library):  python tests/golden/make_upconv_bits.py [OUT.json]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
TABLE = os.path.join(HERE, "upconv_bits.json")


def record():
    sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
    import test_gpu_upconv_forms as t
    cases = {name: t.run_case(name) for name in t.CASES}
    return {"pinned_to": "self: the library that recorded it (tests/golden/make_upconv_bits.py)",
            "identities": dict(t.IDENT), "cases": cases}


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else TABLE
    table = record()
    with open(out, "w") as fh:
        fh.write('{\n"pinned_to": %s,\n"identities": %s,\n"cases": {\n' % (
            json.dumps(table["pinned_to"]), json.dumps(table["identities"], sort_keys=True)))
        fh.write(",\n".join('"%s": %s' % (k, json.dumps(v, sort_keys=True)) for k, v in table["cases"].items()))
        fh.write("\n}\n}\n")
    print(len(table["cases"]), "cases ->", out)
