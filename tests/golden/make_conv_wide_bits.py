"""Record tests/golden/conv_wide_bits.json: per case of tests/test_gpu_conv_wide.py,
{"pinned_to": "oracle" | "gpu", "digests": {output name: SHA-256 of its bf16 bytes}}.

The exact cases' digests are those of the CPU oracle's result rounded to bf16 ("oracle"): they are written
without a GPU, and tests/test_conv_wide_cases.py re-derives them. The float cases' digests are the built
library's on an MI355X ("gpu"), recorded through the test's own run_case, so each case is held to its form,
its determinism, its bitwise identities and the oracle while it is recorded; there the exact cases run too
and must give the oracle's digests. Without a GPU the float rows of the existing table are kept as they are.

Run (after building the library):  python tests/golden/make_conv_wide_bits.py [OUT.json]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
TABLE = os.path.join(HERE, "conv_wide_bits.json")


def record():
    sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
    import torch
    import test_gpu_conv_wide as t
    gpu = torch.cuda.is_available()
    old = {}
    if os.path.exists(TABLE):
        with open(TABLE) as fh:
            old = json.load(fh)
    table = {}
    for name, c in t.CASES.items():
        if c.data == "x":
            row = {"pinned_to": "oracle", "digests": {k: t.sha(v) for k, v in t.oracle_bits(c).items()}}
            if gpu:
                assert t.run_case(name) == row["digests"], name
        elif gpu:
            row = {"pinned_to": "gpu", "digests": t.run_case(name)}
        else:
            row = old.get(name, {"pinned_to": "gpu", "digests": {}})
        table[name] = row
    return table


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else TABLE
    table = record()
    with open(out, "w") as fh:
        fh.write("{\n" + ",\n".join('"%s": %s' % (k, json.dumps(v, sort_keys=True)) for k, v in table.items()) + "\n}\n")
    print(len(table), "cases ->", out)
