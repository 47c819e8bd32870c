"""The conv / BatchNorm host code without a GPU: the built library reproduces, exactly,
tests/golden/conv_host_plan.json -- workspace sizes, the row-streaming and the wide predicate and the status of calls
rejected before the first HIP call (so the order of the argument checks), as recorded by
tests/golden/make_conv_host_plan.py. Fake device pointers are never dereferenced."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_conv_host_plan", os.path.join(GOLDEN, "make_conv_host_plan.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(gen.TABLE) as _fh:
    TABLE = json.load(_fh)


@pytest.mark.parametrize("kind", ["workspace", "rows_form", "wide_form", "rejected"])
def test_library_reproduces_the_recorded_table(kind):
    from sparse_pooling_amd import _lib as L
    lib = L.lib()
    rows = TABLE[kind]
    assert len(rows) >= (20 if kind == "wide_form" else 50)
    bad = []
    for r in rows:
        if kind == "rejected":  # a row that gets through would launch on fake pointers: never replay one
            assert r["status"] not in (L.OK, L.ERR_HIP), r
        got = gen.replay(lib, L, r["fn"], r["args"])
        if got != (r["status"], r["out"]):
            bad.append((r["fn"], r["args"], (r["status"], r["out"]), got))
    assert not bad, bad[:5]


def test_table_covers_the_generator():
    """The committed table is the one the generator's call lists describe (none added or dropped)."""
    for kind, calls in (("workspace", gen.workspace_calls), ("rows_form", gen.rows_form_calls),
                        ("wide_form", gen.wide_form_calls), ("rejected", gen.rejected_calls)):
        want = json.loads(json.dumps([[fn, args] for fn, args in calls()]))
        assert [[r["fn"], r["args"]] for r in TABLE[kind]] == want
