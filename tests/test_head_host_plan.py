"""The 1x1 heads' host code without a GPU: the built library reproduces, exactly, tests/golden/head_host_plan.json
-- the four workspace sizes over a grid of shapes and the status of calls that end before the first HIP call (so
the order of the argument checks), as recorded by tests/golden/make_head_host_plan.py, whose generators are the
list of calls. Fake device pointers are never dereferenced."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_head_host_plan", os.path.join(GOLDEN, "make_head_host_plan.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(gen.TABLE) as _fh:
    TABLE = json.load(_fh)

GRID = 2 * 10 * 4 * 3 * 3  # the shapes of the workspace grid per query


@pytest.mark.parametrize("kind", [k for k, _ in gen.KINDS])
def test_library_reproduces_the_recorded_table(kind):
    from sparse_pooling_amd import _lib as L
    lib = L.lib()
    assert TABLE["calls_sha256"][kind] == gen.calls_sha256(kind), "the generator changed: record the table again"
    calls = gen.calls_of(kind)
    assert sorted(calls) == sorted(TABLE[kind])
    bad = []
    for fn, rows in calls.items():
        want = TABLE[kind][fn]
        assert len(want) == len(rows)
        for args, w in zip(rows, want):  # a call that gets through would launch on fake pointers: never send one
            assert gen.reaches_no_launch(L, kind, fn, args, L.OK if kind == "workspace" else w), (fn, args, w)
            rc, out = gen.replay(lib, L, fn, args)
            got = gen.answer(rc, out) if kind == "workspace" else rc
            if got != w:
                bad.append((fn, args, w, got))
    assert not bad, (len(bad), bad[:5])


def test_table_covers_every_call_and_status():
    """All four queries, all six calls and the mask have rows; every status a check can give is recorded; every
    shape of the grid has a size."""
    from sparse_pooling_amd import _lib as L
    assert set(TABLE["workspace"]) == set(gen.QUERIES)
    assert set(TABLE["rejected"]) == set(gen.CALLS) | {"shpl_dropout_mask"}
    for fn in gen.CALLS:
        assert set(TABLE["rejected"][fn]) == {L.ERR_ARG, L.ERR_BAD_SHAPE, L.ERR_WORKSPACE}, fn
        assert len(TABLE["rejected"][fn]) >= 60
    for fn, vals in TABLE["workspace"].items():
        assert len(vals) > GRID and all(v > 0 for v in vals[:GRID]), fn
        assert {v for v in vals if v < 0} == {-L.ERR_ARG, -L.ERR_BAD_SHAPE}, fn
    assert all(v == L.OK for vals in TABLE["no_rows"].values() for v in vals)
