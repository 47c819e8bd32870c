"""The plain MV3D producer (shpl_mv3d_voxels) over a ragged batch with number_buffer (MI355X): every frame of
tests/mv3d_cases.py, every output, bitwise against the oracle -- with img_index2 handed in, with P projected on
the device, and with augment_fv's index transform per frame."""
import numpy as np
import pytest
import torch

import mv3d_cases as mc
from oracle import shpl_oracle as orc
from sparse_pooling_amd import mv3d

pytestmark = pytest.mark.gpu

DEV = "cuda"
FORMS = ("img_index2", "P", "fv_aug")


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


@pytest.fixture(scope="module")
def expected():
    """Per form and frame: the oracle's (img_index, bv_index, M_val, number_buffer)."""
    b = mc.batch()
    want = {form: [] for form in FORMS}
    for f in range(len(mc.NAMES)):
        s = slice(b["off"][f], b["off"][f + 1])
        pts = b["points"][s]
        given = orc.mv3d_voxels(pts, b["img_index2"][:, s], mc.RANGES, mc.RES, mc.ZRES, mc.CAP)
        want["img_index2"].append(given)
        want["P"].append(orc.mv3d_voxels(pts, mc.project_round(b["P"][f], pts), mc.RANGES, mc.RES, mc.ZRES, mc.CAP))
        aug = orc.augment_fv_index(given[0].astype(np.int64), *b["fv_aug"][f]).astype(np.float64)
        want["fv_aug"].append((aug, *given[1:]))
    return b, want


@pytest.mark.parametrize("form", FORMS)
def test_ragged_batch_equals_the_oracle(expected, form):
    b, want = expected
    assert mv3d.PED_RANGES == mc.RANGES
    kw = {"P": _dev(b["P"])} if form == "P" else {"img_index2": _dev(b["img_index2"])}
    if form == "fv_aug":
        kw["fv_aug"] = b["fv_aug"]
    out = mv3d.mv3d_voxels_batch(_dev(b["points"]), _dev(b["off"]), number_buffer=True, **kw)
    fn, nvx = _np(out["frame_n"]), _np(out["frame_nvox"])
    assert fn.shape == nvx.shape == (len(mc.NAMES),)
    for f, (img, bv, mv, nb) in enumerate(want[form]):
        k, nv, p0 = bv.shape[0], nb.shape[0], int(b["off"][f])
        assert (int(fn[f]), int(nvx[f])) == (k, nv), mc.NAMES[f]
        np.testing.assert_array_equal(_np(out["img_index"][:, p0:p0 + k]), img, mc.NAMES[f])
        np.testing.assert_array_equal(_np(out["bv_index"][p0:p0 + k]), bv, mc.NAMES[f])
        np.testing.assert_array_equal(_np(out["M_val"][p0:p0 + k]), mv, mc.NAMES[f])
        np.testing.assert_array_equal(_np(out["number_buffer"][p0:p0 + nv]), nb, mc.NAMES[f])
