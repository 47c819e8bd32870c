"""The frame producers' host code without a GPU: the built library reproduces, exactly,
tests/golden/frames_host_plan.json -- the BEV voxelizer's, the MV3D producer's and the velodyne loader's
workspace sizes, and the status of calls rejected before the first HIP call (so the order of the argument
checks), as recorded by tests/golden/make_frames_host_plan.py. Fake device pointers are never dereferenced."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_frames_host_plan",
                                               os.path.join(GOLDEN, "make_frames_host_plan.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(gen.TABLE) as _fh:
    TABLE = json.load(_fh)

KINDS = (("workspace", gen.workspace_calls), ("rejected", gen.rejected_calls))
WORKSPACE_FNS = {"shpl_bev_workspace_bytes", "shpl_mv3d_workspace_bytes", "shpl_velo_workspace_bytes"}
REJECTED_FNS = {"shpl_bev_slices", "shpl_bev_maps", "shpl_bev_input", "shpl_mv3d_voxels", "shpl_mv3d_voxels_aug",
                "shpl_mv3d_augment_points", "shpl_velo_to_cam"}


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
    assert {r["fn"] for r in TABLE["workspace"]} == WORKSPACE_FNS
    assert {r["fn"] for r in TABLE["rejected"]} == REJECTED_FNS


def test_the_recorded_order_of_the_bev_checks():
    """The pair the three BEV entry points answer differently: a short workspace with a geometry they would also
    refuse is SHPL_ERR_WORKSPACE from shpl_bev_slices and SHPL_ERR_BAD_SHAPE from shpl_bev_maps / shpl_bev_input;
    an f32 cloud with null maps is SHPL_ERR_ARG from shpl_bev_slices."""
    from sparse_pooling_amd import _lib as L
    status = {json.dumps([r["fn"], r["args"]]): r["status"] for r in TABLE["rejected"]}
    look = lambda call: status[json.dumps(list(call))]  # noqa: E731
    for g in gen.BAD_GEOMS:
        assert look(gen.bev_slices(ws_bytes=0, **g)) == L.ERR_WORKSPACE
        assert look(gen.bev_slices(ws_bytes=gen.BIG, **g)) == L.ERR_BAD_SHAPE
        assert look(gen.bev_maps(ws_bytes=0, **g)) == L.ERR_BAD_SHAPE
        assert look(gen.bev_input(ws_bytes=0, **g)) == L.ERR_BAD_SHAPE
    assert look(gen.bev_slices(pdt=gen.F32, hm=None, dm=None, ws_bytes=gen.BIG)) == L.ERR_ARG
