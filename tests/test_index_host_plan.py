"""The index and CSR builders' host code without a GPU: the built library reproduces, exactly,
tests/golden/index_host_plan.json -- the three workspace sizes and the status of calls rejected before the
first HIP call (so the order of the argument checks), as recorded by tests/golden/make_index_host_plan.py.
Fake device pointers are never dereferenced."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_index_host_plan", os.path.join(GOLDEN, "make_index_host_plan.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(gen.TABLE) as _fh:
    TABLE = json.load(_fh)

KINDS = (("workspace", gen.workspace_calls), ("rejected", gen.rejected_calls))
REJECTED_FNS = {"shpl_build_index", "shpl_build_index_buckets", "shpl_gen_index", "shpl_produce_index",
                "shpl_build_csr_path", "shpl_build_csr_buckets", "shpl_bucket_workspace_reset"}


@pytest.mark.parametrize("kind", [k for k, _ in KINDS])
def test_library_reproduces_the_recorded_table(kind):
    from sparse_pooling_amd import _lib as L
    lib = L.lib()
    rows = TABLE[kind]
    assert len(rows) >= 50
    bad = []
    for r in rows:
        if kind == "rejected":  # a row that gets through would launch on fake pointers: never replay one
            assert r["status"] not in (L.OK, L.ERR_HIP), r
        got = gen.replay(lib, L, r["fn"], r["args"])
        if got != (r["status"], r["out"]):
            bad.append((r["fn"], r["args"], (r["status"], r["out"]), got))
    assert not bad, bad[:5]


def test_table_covers_the_generator():
    """The committed table is the one the generator's call lists describe (none added or dropped), and every
    function with argument checks has rejected rows."""
    for kind, calls in KINDS:
        want = json.loads(json.dumps([[fn, args] for fn, args in calls()]))
        assert [[r["fn"], r["args"]] for r in TABLE[kind]] == want
    assert {r["fn"] for r in TABLE["rejected"]} == REJECTED_FNS
