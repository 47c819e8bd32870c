"""The CPU oracle, called per frame with the frame's OWN image size, against the reference run of a batch of mixed
image sizes (tests/golden/index_ragged.npz, written by tests/golden/make_ragged_golden.py): KITTI's four image
sizes and a half-size frame, strides (4, 4) and (8, 8). CPU only. The GPU tests of the ragged index builder take
their expectations from the same per-frame oracle calls (tests/ragged_cases.py)."""
import numpy as np
import pytest

import ragged_cases as rc
from oracle import shpl_oracle as orc


@pytest.mark.parametrize("stride", [4, 8])
def test_oracle_per_frame_own_size_matches_reference(stride):
    g = rc.golden()
    sizes = g["sizes"]
    assert [tuple(s) for s in sizes[:4]] == rc.KITTI_SIZES and sizes.shape == (5, 2)
    differs = 0
    for f, size in enumerate(sizes):
        ref = rc.oracle_index(g[f"points_{f}"], g[f"voxels_{f}"], g["P"], size, g["bv_size"], (stride, stride))
        np.testing.assert_array_equal(ref["Mij_pool"], g[f"mij_{stride}_{f}"].reshape(-1, 2))
        np.testing.assert_array_equal(ref["img_index_flip_pool"], g[f"flip_{stride}_{f}"].reshape(-1, 3))
        np.testing.assert_array_equal(ref["M_size"], g[f"msize_{stride}_{f}"])
        # the clamp is the frame's own: no index at or past floor(own size / stride)
        flip = g[f"flip_{stride}_{f}"].reshape(-1, 3)
        assert (flip[:, 1] < np.floor(size[1] / stride)).all() and (flip[:, 2] < np.floor(size[0] / stride)).all()
        padded = rc.oracle_index(g[f"points_{f}"], g[f"voxels_{f}"], g["P"], g["padded"], g["bv_size"],
                                 (stride, stride))
        differs += padded["Mij_pool"].shape != ref["Mij_pool"].shape or not np.array_equal(
            padded["img_index_flip_pool"], ref["img_index_flip_pool"])
    assert differs >= 3  # the fixture can tell a frame's own size from the padded one


def test_fixture_is_small_and_data_only():
    import os
    assert os.path.getsize(rc.GOLDEN) < 100 * 1024
    g = np.load(rc.GOLDEN, allow_pickle=False)  # plain arrays: no pickled objects
    assert all(g[k].dtype.kind in "fiu" for k in g.files)


def test_produce_is_called_on_a_fresh_gen(monkeypatch):
    """oracle_index never hands produce an img_index another call has already strided (produce mutates it)."""
    g = rc.golden()
    a = rc.oracle_index(g["points_1"], g["voxels_1"], g["P"], g["sizes"][1], g["bv_size"], (4, 4))
    b = rc.oracle_index(g["points_1"], g["voxels_1"], g["P"], g["sizes"][1], g["bv_size"], (4, 4))
    np.testing.assert_array_equal(a["img_index_flip_pool"], b["img_index_flip_pool"])
    assert orc.gen_sparse_pooling_input_avod(g["points_1"], g["voxels_1"], g["P"], list(g["sizes"][1]),
                                             tuple(g["bv_size"]))["img_index"].max() > g["sizes"][1][0] / 4
