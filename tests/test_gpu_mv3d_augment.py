"""MV3D's augment_voxel on the device (MI355X), bitwise against the reference-
generated fixtures tests/golden/mv3d_augment_*.npz: the materialised cloud and
img_index2, the fused producer's outputs, fused against the existing producer
over the materialised cloud, the chain to the pooling, and the bounded gather.

Every comparison is against stored data or between two device results: no live
np.dot on this host (its BLAS may order the 2 x 2 product differently).
"""
import glob
import os

import numpy as np
import pytest
import torch

from oracle import shpl_oracle as orc
from sparse_pooling_amd import mv3d, synth

pytestmark = pytest.mark.gpu

DEV = "cuda"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(glob.glob(os.path.join(GOLD, "mv3d_augment_*.npz")))
IDS = [os.path.basename(p)[len("mv3d_augment_"):-len(".npz")] for p in CASES]


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _frame(g):
    """One fixture as the device calls' arguments: the cloud in its own dtype, offsets, P, vox_aug, the gather."""
    pts = _dev(g["points"])
    off = _dev([0, g["points"].shape[0]], np.int64)
    P = _dev(g["P"].reshape(1, 12))
    vox = np.array([[*g["params"][:3], *g["rot"].reshape(4), 0.0]])
    remain = roff = None
    if g["augment_pc"]:
        remain = _dev(g["remain_index"], np.int64)
        roff = _dev([0, g["remain_index"].shape[0]], np.int64)
    return pts, off, P, vox, remain, roff


@pytest.mark.parametrize("path", CASES, ids=IDS)
def test_materialised_cloud_and_img_index2_equal_the_fixture(path):
    g = np.load(path)
    pts, off, P, vox, remain, roff = _frame(g)
    out = mv3d.augment_points(pts, off, P, vox, remain, roff)
    assert out["points"].dtype == torch.float64 and out["img_index2"].dtype == torch.int64
    np.testing.assert_array_equal(_np(out["points"]), g["aug_points"].astype(np.float64))
    np.testing.assert_array_equal(_np(out["img_index2"]), g["img_index2"])
    assert int(out["err"].item()) == 0


@pytest.mark.parametrize("path", CASES, ids=IDS)
def test_fused_producer_equals_the_fixture(path):
    g = np.load(path)
    pts, off, P, vox, remain, roff = _frame(g)
    out = mv3d.mv3d_voxels_batch(pts, off, P=P, number_buffer=True, vox_aug=vox, remain_index=remain,
                                 remain_offsets=roff)
    k, nv = int(out["frame_n"][0].item()), int(out["frame_nvox"][0].item())
    assert k == g["bv_index"].shape[0] and nv == g["number_buffer"].shape[0]
    np.testing.assert_array_equal(_np(out["img_index"][:, :k]), g["img_index"])
    np.testing.assert_array_equal(_np(out["bv_index"][:k]), g["bv_index"].reshape(-1, 2))
    np.testing.assert_array_equal(_np(out["M_val"][:k]), g["M_val"])
    np.testing.assert_array_equal(_np(out["number_buffer"][:nv]), g["number_buffer"])
    assert int(out["err"].item()) == 0
    # the one-frame wrapper
    img, bv, mv = mv3d.mv3d_sparse_pooling_input(g["points"], P=g["P"], vox_aug=vox[0],
                                                 remain_index=g["remain_index"] if g["augment_pc"] else None)
    np.testing.assert_array_equal(_np(img), g["img_index"])
    np.testing.assert_array_equal(_np(bv), g["bv_index"].reshape(-1, 2))
    np.testing.assert_array_equal(_np(mv), g["M_val"])


def test_augment_voxel_has_the_references_signature_and_results():
    """Seeded like the generator's call: (blobs, cloud, img_index2) with the boxes augmented in place."""
    g = np.load(os.path.join(GOLD, "mv3d_augment_f32_pc.npz"))
    blobs = {"gt_boxes_3d": g["boxes_before"].copy(), "gt_rys": g["rys_before"].copy()}
    np.random.seed(int(g["seed"]))
    out, cloud, img2 = mv3d.augment_voxel(blobs, scale=float(g["scale"]), lidar_pc=g["points"], calib=g["calib"],
                                          augment_pc=True)
    assert out is blobs
    np.testing.assert_array_equal(blobs["gt_boxes_3d"], g["boxes_after"])
    np.testing.assert_array_equal(blobs["gt_rys"], g["rys_after"])
    np.testing.assert_array_equal(_np(cloud), g["aug_points"].astype(np.float64))
    np.testing.assert_array_equal(_np(img2), g["img_index2"])


# ---------------------------------------------------------------- fused vs materialised, a ragged batch

@pytest.fixture(scope="module")
def ragged():
    """5 frames of f64 points: 2500, none, one, 1800 redrawn with replacement to 1700 (AUGMENT_PC), 3000
    clustered over the 45-point cap; the other frames' gather is the identity. Per-frame draws in
    augment_voxel's ranges from a seeded generator (the rotation formed on the host, as the reference forms it)."""
    rng = np.random.default_rng(77)
    sizes = [2500, 0, 1, 1800, 3000]
    frames = []
    for n in sizes:
        p = np.stack([rng.uniform(-21, 21, n), rng.uniform(-1.2, 3.2, n), rng.uniform(-0.5, 49, n),
                      rng.uniform(0, 1, n)], axis=1)
        frames.append(p)
    frames[2][0] = [1.5, 0.5, 11.0, 0.2]
    centers = np.stack([rng.uniform(-15, 15, 30), rng.uniform(0, 2, 30), rng.uniform(5, 40, 30)], 1)
    frames[4][:, :3] = centers[rng.integers(0, 30, 3000)] + rng.normal(0, 0.05, (3000, 3))
    remain = [np.arange(n) for n in sizes]
    remain[3] = rng.integers(0, 1800, 1700)
    vox = []
    for _ in sizes:
        a = rng.uniform(-np.pi / 10, np.pi / 10)
        vox.append([rng.uniform(-0.8, 0.8), rng.uniform(-0.8, 0.8), rng.uniform(0.95, 1.05), np.cos(a), np.sin(a),
                    -np.sin(a), np.cos(a), 0.0])
    P = np.stack([synth.KITTI_P2.reshape(12)] * len(sizes))
    P[1:, 3] += np.arange(1, len(sizes)) * 0.25  # a camera matrix of its own per frame
    return dict(points=_dev(np.concatenate(frames)), off=_dev(np.cumsum([0] + sizes), np.int64), P=_dev(P),
                vox=np.array(vox), remain=_dev(np.concatenate(remain), np.int64),
                roff=_dev(np.cumsum([0] + [len(r) for r in remain]), np.int64),
                fv=np.array([[1.0312, 3.7, 8.25], [1.0, 0.0, 0.0], [0.9514, 0.0, 9.99], [1.02, 5.5, 0.5],
                             [0.97, 9.0, 2.0]]))


@pytest.mark.parametrize("with_fv", [False, True], ids=["plain", "fv_aug"])
def test_fused_equals_the_producer_over_the_materialised_cloud(ragged, with_fv):
    """The fused form against the comparator the issue names: shpl_mv3d_voxels over augment_points' cloud and
    img_index2. f64 clouds: there both routes key the voxels in f64 (an f32 cloud is keyed in f32 by the fused
    form, as the reference does, and in f64 over the widened cloud -- the planted fixture holds the difference)."""
    r = ragged
    fv = r["fv"] if with_fv else None
    mat = mv3d.augment_points(r["points"], r["off"], r["P"], r["vox"], r["remain"], r["roff"])
    ref = mv3d.mv3d_voxels_batch(mat["points"], r["roff"], img_index2=mat["img_index2"], number_buffer=True, fv_aug=fv)
    fused = mv3d.mv3d_voxels_batch(r["points"], r["off"], P=r["P"], number_buffer=True, fv_aug=fv, vox_aug=r["vox"],
                                   remain_index=r["remain"], remain_offsets=r["roff"])
    assert int(mat["err"].item()) == 0 and int(fused["err"].item()) == 0
    fn, nvx, roff = _np(ref["frame_n"]), _np(ref["frame_nvox"]), _np(r["roff"])
    np.testing.assert_array_equal(_np(fused["frame_n"]), fn)
    np.testing.assert_array_equal(_np(fused["frame_nvox"]), nvx)
    assert fn[1] == 0 and fn[2] == 1 and fn[0] > 1500 and fn[3] > 1000
    assert (_np(ref["M_val"][roff[4]:roff[4] + fn[4]]) < 1 / 40).any()  # voxels over the cap
    for f in range(5):
        s = slice(roff[f], roff[f] + fn[f])
        np.testing.assert_array_equal(_np(fused["img_index"][:, s]), _np(ref["img_index"][:, s]))
        np.testing.assert_array_equal(_np(fused["bv_index"][s]), _np(ref["bv_index"][s]))
        np.testing.assert_array_equal(_np(fused["M_val"][s]), _np(ref["M_val"][s]))
        v = slice(roff[f], roff[f] + nvx[f])
        np.testing.assert_array_equal(_np(fused["number_buffer"][v]), _np(ref["number_buffer"][v]))


def test_fused_reads_the_originals_img_index2_through_the_gather(ragged):
    """img_index2 of the ORIGINAL points handed in instead of P: the fused form indexes it by source point."""
    r = ragged
    same = mv3d.augment_points(r["points"], r["off"], r["P"], np.tile([0, 0, 1, 1, 0, 0, 1, 0.0], (5, 1)))
    a = mv3d.mv3d_voxels_batch(r["points"], r["off"], P=r["P"], vox_aug=r["vox"], remain_index=r["remain"],
                               remain_offsets=r["roff"])
    b = mv3d.mv3d_voxels_batch(r["points"], r["off"], img_index2=same["img_index2"], vox_aug=r["vox"],
                               remain_index=r["remain"], remain_offsets=r["roff"])
    fn, roff = _np(a["frame_n"]), _np(r["roff"])
    np.testing.assert_array_equal(_np(b["frame_n"]), fn)
    for f in range(5):
        s = slice(roff[f], roff[f] + fn[f])
        np.testing.assert_array_equal(_np(b["img_index"][:, s]), _np(a["img_index"][:, s]))


# ---------------------------------------------------------------- chain to the pooling

def test_fused_chain_to_pooling_matches_the_oracle_on_the_fixture():
    """Fused producer -> produce_sparse_pooling_input(stride [8, 2], M_val = 1/count) -> sparse_pool against the
    oracle chain on the FIXTURE's indices (the dense, image-visible case: voxels over the 45-point cap)."""
    from sparse_pooling_amd.sparse_pool_utils import SparseTensor
    g = np.load(os.path.join(GOLD, "mv3d_augment_dense.npz"))
    pts, off, P, vox, remain, roff = _frame(g)
    out = mv3d.mv3d_voxels_batch(pts, off, P=P, vox_aug=vox, remain_index=remain, remain_offsets=roff)
    k = int(out["frame_n"][0].item())
    img, bv, mv = out["img_index"][:, :k], out["bv_index"][:k], out["M_val"][:k]
    np.testing.assert_array_equal(_np(img), g["img_index"])
    assert (g["M_val"] < 1).any() and g["M_val"].min() == 1 / 45
    Mij, M_val, M_size, flip = mv3d.produce_sparse_pooling_input(img.clone(), np.array([1280, 384]), bv, [200, 240],
                                                                 M_val=mv, stride=[8, 2])
    ref = orc.produce_sparse_pooling_input({"img_index": g["img_index"].astype(np.float64),
                                            "bv_index": g["bv_index"], "img_size": np.array([1280, 384]),
                                            "bv_size": np.array([200, 240])}, M_val=g["M_val"], stride=(8, 2))
    np.testing.assert_array_equal(_np(Mij), ref["Mij_pool"])
    np.testing.assert_array_equal(_np(flip), ref["img_index_flip_pool"])
    feat = synth.make_features((1, 48, 160, 8), 5)
    pooled = mv3d.sparse_pool([SparseTensor(Mij, M_val, M_size), torch.from_numpy(feat).to(DEV), flip],
                              [1, 100, 120, 8])
    e = orc.sparse_pool_op(ref["Mij_pool"], ref["M_val"], ref["M_size"], feat, ref["img_index_flip_pool"])
    np.testing.assert_array_equal(_np(pooled).astype(np.float32), e.reshape(1, 100, 120, 8).astype(np.float32))


# ---------------------------------------------------------------- the gather is bounded

def test_out_of_frame_remain_index_is_reported_and_skipped(monkeypatch):
    """remain_index entries outside their frame -- negative, one past the frame, far past the whole cloud --
    are never dereferenced: SHPL_EBIT_GATHER in the error word, the materialised row is NaN with pixel (0, 0),
    the fused form drops the point, and every other point comes out as from the gather without those entries."""
    from sparse_pooling_amd import _lib as L
    g = np.load(os.path.join(GOLD, "mv3d_augment_f32_pc.npz"))
    pts, off, P, vox, remain, roff = _frame(g)
    n = g["points"].shape[0]
    bad_at = np.array([0, 7, 1000])
    bad = g["remain_index"].copy()
    bad[bad_at] = [-1, n, 1 << 40]
    keep = np.ones(len(bad), bool)
    keep[bad_at] = False
    bad_d = _dev(bad, np.int64)
    mat = mv3d.augment_points(pts, off, P, vox, bad_d, roff)
    assert int(mat["err"].item()) == L.EBIT_GATHER
    cloud = _np(mat["points"])
    assert np.isnan(cloud[bad_at]).all() and (_np(mat["img_index2"])[:, bad_at] == 0).all()
    np.testing.assert_array_equal(cloud[keep], g["aug_points"].astype(np.float64)[keep])
    np.testing.assert_array_equal(_np(mat["img_index2"])[:, keep], g["img_index2"][:, keep])
    out = mv3d.mv3d_voxels_batch(pts, off, P=P, number_buffer=True, vox_aug=vox, remain_index=bad_d,
                                 remain_offsets=roff)
    assert int(out["err"].item()) == L.EBIT_GATHER
    ref = mv3d.mv3d_voxels_batch(pts, off, P=P, number_buffer=True, vox_aug=vox, remain_index=_dev(bad[keep], np.int64),
                                 remain_offsets=_dev([0, int(keep.sum())], np.int64))
    assert int(ref["err"].item()) == 0
    k, nv = int(ref["frame_n"][0].item()), int(ref["frame_nvox"][0].item())
    assert k > 1500 and int(out["frame_n"][0].item()) == k and int(out["frame_nvox"][0].item()) == nv
    for name in ("bv_index", "M_val"):
        np.testing.assert_array_equal(_np(out[name][:k]), _np(ref[name][:k]))
    np.testing.assert_array_equal(_np(out["img_index"][:, :k]), _np(ref["img_index"][:, :k]))
    np.testing.assert_array_equal(_np(out["number_buffer"][:nv]), _np(ref["number_buffer"][:nv]))
    # augment_voxel raises what the reference's lidar_pc[remain_index] raises
    monkeypatch.setattr(np.random, "choice", lambda a, size: bad)
    with pytest.raises(IndexError):
        mv3d.augment_voxel({"gt_boxes_3d": g["boxes_before"].copy(), "gt_rys": g["rys_before"].copy()},
                           lidar_pc=g["points"], calib=g["calib"], augment_pc=True)


def test_frame_offsets_outside_the_arrays_make_the_frame_empty():
    """Offsets live on the device too: decreasing or past the cloud, they set SHPL_EBIT_GATHER and the frame
    comes out empty instead of being read."""
    from sparse_pooling_amd import _lib as L
    g = np.load(os.path.join(GOLD, "mv3d_augment_f64.npz"))
    pts, off, P, vox, _, _ = _frame(g)
    n = g["points"].shape[0]
    for bad in ([0, n + 5], [n, 0], [-3, n]):
        out = mv3d.mv3d_voxels_batch(pts, _dev(bad, np.int64), P=P, vox_aug=vox)
        assert int(out["err"].item()) == L.EBIT_GATHER, bad
        assert int(out["frame_n"][0].item()) == 0
