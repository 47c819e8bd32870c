"""The MV3D batch cases (tests/mv3d_cases.py) without a GPU: on the oracle's outputs, every frame reaches the
path of k_mv3d_frame it is named for."""
import numpy as np
import pytest

import mv3d_cases as mc
from oracle import shpl_oracle as orc


@pytest.fixture(scope="module")
def frames():
    out = {}
    for name, pts in zip(mc.NAMES, mc.frames()):
        img2 = np.arange(2 * pts.shape[0], dtype=np.int64).reshape(2, -1)
        img, bv, mv, nb = orc.mv3d_voxels(pts, img2, mc.RANGES, mc.RES, mc.ZRES, mc.CAP)
        key, length, start = mc.voxel_runs(pts)
        # the numpy restatement of the sorted words agrees with the oracle: one count per voxel, capped
        np.testing.assert_array_equal(nb, np.minimum(length, mc.CAP))
        assert bv.shape[0] == mv.shape[0] == img.shape[1] == int(np.minimum(length, mc.CAP).sum())
        out[name] = dict(pts=pts, img=img, bv=bv, mv=mv, nb=nb, length=length, start=start)
    return out


def test_sizes_and_order():
    fr = mc.frames()
    assert [f.shape[0] for f in fr] == [0, 1, 3000, 1100, 1500, 0] and all(f.shape[1] == 4 for f in fr)
    b = mc.batch()
    assert b["off"].tolist() == [0, 0, 1, 3001, 4101, 5601, 5601]
    assert b["img_index2"].shape == (2, 5601) and b["P"].shape == (6, 12) and b["fv_aug"].shape == (6, 3)
    assert len({tuple(r) for r in b["fv_aug"]}) == 6 and len({tuple(r) for r in b["P"]}) == 6


def test_empty_frames_and_the_one_point(frames):
    for name in ("empty_first", "empty_last"):
        assert frames[name]["bv"].shape == (0, 2) and frames[name]["nb"].shape == (0,)
    one = frames["one"]
    assert one["bv"].shape == (1, 2) and one["mv"].tolist() == [1.0] and one["nb"].tolist() == [1]


def test_many_voxels_carries_the_base_across_a_block(frames):
    f = frames["many_voxels"]
    assert f["nb"].shape[0] > mc.BLOCK               # voxels, so run starts, in more than one pass
    assert (f["start"] >= mc.BLOCK).sum() > 1000     # and most of them behind the first
    assert f["length"].sum() > 2 * mc.BLOCK and f["length"].sum() < 3000  # some points outside the ranges


def test_block_1024_is_exactly_one_pass(frames):
    f = frames["block_1024"]
    assert f["length"].sum() == mc.BLOCK and f["length"].max() < mc.CAP  # 1024 words
    assert f["bv"].shape[0] == mc.BLOCK                                  # exactly 1024 kept, of 1100 points
    assert f["pts"].shape[0] > mc.BLOCK


def test_capped_has_runs_over_the_cap_and_one_over_word_1024(frames):
    f = frames["capped"]
    assert (f["nb"] == mc.CAP).sum() == 6 and (f["length"] > mc.CAP).sum() == 6  # counts equal to 45
    assert sorted(f["length"][f["length"] > mc.CAP]) == [60, 65, 70, 75, 80, 150]
    over = (f["start"] < mc.BLOCK) & (f["start"] + f["length"] > mc.BLOCK)
    assert over.sum() == 1 and f["length"][over][0] == 150 and f["start"][over][0] == 950
    assert (f["mv"] == 1 / 45).sum() == 6 * mc.CAP and f["bv"].shape[0] < f["length"].sum() < 1500
    # the capped voxels' points are not in order in memory: the first 45 in point order are not the first 45 planted
    assert (np.diff(f["pts"][:, 0]) < 0).sum() > 500
