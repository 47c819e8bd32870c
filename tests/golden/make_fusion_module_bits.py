"""Record tests/golden/fusion_module_bits.json: the SHA-256 of every output, gradient and moving statistic of every
case of tests/test_gpu_fusion_modules.py, and the backward's schedule of its switch cases, computed by the built
library and the package's Python on an MI355X. The cases are run through the test's own functions (run_case,
identities), so each is also held to its bitwise identities while it is recorded.

The table is self-referential ("pinned_to"): it pins the fusion modules bit for bit across a refactor of their
Python -- record it from the commit before the change, and tests/test_gpu_fusion_modules.py holds every later
commit to it. The kernels are deterministic, so two recordings in separate processes must be identical.
"identities" lists the identities that did not hold when the table was recorded, each with a one-line reason
(the test's NOT_HELD; one found here without a reason there is written with "?" and fails the test until it is
explained); the test asserts every other one.

Run (after building the library):  python tests/golden/make_fusion_module_bits.py [OUT.json]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
TABLE = os.path.join(HERE, "fusion_module_bits.json")


def record():
    sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
    import test_gpu_fusion_modules as t
    cases = {name: t.run_case(name) for name in t.CASES}
    not_held = {}
    for name in t.CASES:
        for what, held in t.identities(name).items():
            if not held:
                not_held[what] = t.NOT_HELD.get(what, "?")
    return {"pinned_to": "self: the commit that recorded it (tests/golden/make_fusion_module_bits.py)",
            "identities": not_held,
            "schedule": {k: v["schedule"] for k, v in cases.items() if "schedule" in v},
            "cases": {k: v["bits"] for k, v in cases.items()}}


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else TABLE
    table = record()
    with open(out, "w") as fh:
        fh.write('{\n"pinned_to": %s,\n"identities": %s,\n"schedule": {\n' % (
            json.dumps(table["pinned_to"]), json.dumps(table["identities"], sort_keys=True)))
        fh.write(",\n".join('"%s": %s' % (k, json.dumps(v)) for k, v in table["schedule"].items()))
        fh.write('\n},\n"cases": {\n')
        fh.write(",\n".join('"%s": %s' % (k, json.dumps(v, sort_keys=True)) for k, v in table["cases"].items()))
        fh.write("\n}\n}\n")
    print(len(table["cases"]), "cases,", len(table["identities"]), "identities not held ->", out)
