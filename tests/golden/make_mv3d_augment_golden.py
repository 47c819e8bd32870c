"""Generate the MV3D voxel-augmentation fixtures by RUNNING the reference's own
``augment_voxel`` and ``point_cloud_2_top_sparse`` (make_golden.py's rules: the
reference checkout is needed here and nowhere else; the fixtures are data only).

Reference functions executed (file:line, relative to the reference checkout):

* ``augment_voxel``            MV3D_TF_release/lib/roi_data_layer/minibatch_mv3d_img.py:132-189
* ``point_cloud_2_top_sparse`` MV3D_TF_release/lib/utils/construct_voxel.py:37-162

``fast_rcnn.config`` and ``utils.blob`` are stubbed in ``sys.modules`` (the
module imports them for get_minibatch; augment_voxel reads only
``cfg.TRAIN.AUGMENT_PC``). Each case seeds ``np.random``, calls the reference,
then re-seeds and repeats the reference's draws to record them.

Every ``mv3d_augment_<case>.npz`` holds the inputs (points, calib, P, seed,
scale, augment_pc, the boxes before), the drawn parameters (params = sx, sz,
ratio, angle; rot; remain_index), the augmented cloud and img_index2, the
producer's img_index / bv_index / M_val / number_buffer over it, and the boxes
after.

Run:  python tests/golden/make_mv3d_augment_golden.py
"""
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import _install_stubs  # noqa: E402

from sparse_pooling_amd import synth  # noqa: E402

SCALE = 0.8  # get_minibatch's call (minibatch_mv3d_img.py:85)
PLANTED_MIN = 8  # planted points per coordinate


def _reference():
    _install_stubs()
    cfg = types.SimpleNamespace(TRAIN=types.SimpleNamespace(AUGMENT_PC=False))
    fr = types.ModuleType("fast_rcnn")
    frc = types.ModuleType("fast_rcnn.config")
    frc.cfg = cfg
    fr.config = frc
    sys.modules["fast_rcnn"] = fr
    sys.modules["fast_rcnn.config"] = frc
    blob = types.ModuleType("utils.blob")
    blob.prep_im_for_blob = blob.im_list_to_blob = None
    sys.modules["utils.blob"] = blob
    mb = importlib.import_module("roi_data_layer.minibatch_mv3d_img")
    cv = importlib.import_module("utils.construct_voxel")
    return mb, cv, cfg


def _draws(seed, scale, n, augment_pc):
    """The reference's draws, in its order (minibatch_mv3d_img.py:134-136, :171-172)."""
    np.random.seed(seed)
    sx, sz = np.random.uniform(-scale, scale, 2)
    ratio = np.random.uniform(0.95, 1.05, 1)
    angle = np.random.uniform(-np.pi / 10, np.pi / 10, 1)
    remain = np.zeros(0, dtype=np.int64)
    if augment_pc:
        rate = np.random.uniform(0.9, 1.0, 1)
        remain = np.random.choice(n, int(n * rate[0]))
    rot = np.array([[np.cos(angle), np.sin(angle)], [-np.sin(angle), np.cos(angle)]]).reshape(2, 2)
    return np.array([sx, sz, ratio[0], angle[0]]), rot, np.asarray(remain, dtype=np.int64)


def _cloud(rng, n, dense=False):
    # camera frame: x side, y height (down), z forward; some points outside the ranges
    pts = np.stack([rng.uniform(-21, 21, n), rng.uniform(-1.2, 3.2, n), rng.uniform(-0.5, 49, n),
                    rng.uniform(0, 1, n)], axis=1)
    if dense:
        centers = np.stack([rng.uniform(-15, 15, 40), rng.uniform(0, 2, 40), rng.uniform(5, 40, 40)], 1)
        pts[:, :3] = centers[rng.integers(0, 40, n)] + rng.normal(0, 0.05, (n, 3))
        # image-visible points only, like MV3D's FOV-filtered minibatches: the dense case also feeds the chain
        # to produce_sparse_pooling_input and sparse_pool, which take pixels inside the 1280 x 384 image
        uvw = synth.KITTI_P2 @ np.vstack((pts[:, :3].astype(np.float32).T, np.ones(n)))
        u, v = np.round(uvw[0] / uvw[2]), np.round(uvw[1] / uvw[2])
        pts = pts[(uvw[2] > 0) & (u >= 0) & (u < 1280) & (v >= 0) & (v < 384)]
    return pts


def _boxes(rng, k=5):
    b = np.concatenate([rng.uniform(-15, 15, (k, 1)), rng.uniform(0.5, 2, (k, 1)), rng.uniform(3, 45, (k, 1)),
                        rng.uniform(0.5, 4, (k, 3)), rng.integers(1, 4, (k, 1))], axis=1).astype(np.float32)
    return b, rng.uniform(-np.pi, np.pi, (k, 1))


def _case(ref, name, pts, seed, augment_pc, rng):
    mb, cv, cfg = ref
    calib = np.zeros((4, 12))
    calib[0] = synth.KITTI_P2.reshape(-1)
    boxes, rys = _boxes(rng)
    blobs = {"gt_boxes_3d": boxes.copy(), "gt_rys": rys.copy()}
    cfg.TRAIN.AUGMENT_PC = bool(augment_pc)
    np.random.seed(seed)
    blobs, aug, img_index2 = mb.augment_voxel(blobs, scale=SCALE, lidar_pc=pts.copy(), calib=calib.copy())
    assert aug.dtype == pts.dtype
    vd, full, img_index, bv_index, M_val = cv.point_cloud_2_top_sparse(
        aug.copy(), points_in_cam=True, calib=calib.copy(), img_index2=img_index2.copy())
    params, rot, remain = _draws(seed, SCALE, pts.shape[0], augment_pc)
    out = os.path.join(HERE, f"mv3d_augment_{name}.npz")
    np.savez_compressed(out, points=pts, calib=calib, P=synth.KITTI_P2, seed=np.array(seed), scale=np.array(SCALE),
                        augment_pc=np.array(bool(augment_pc)), params=params, rot=rot, remain_index=remain,
                        aug_points=aug, img_index2=np.asarray(img_index2, dtype=np.int64),
                        voxel_full_size=np.asarray(full), img_index=img_index, bv_index=bv_index, M_val=M_val,
                        number_buffer=vd["number_buffer"], boxes_before=boxes, rys_before=rys,
                        boxes_after=blobs["gt_boxes_3d"], rys_after=blobs["gt_rys"])
    print(f"mv3d_augment_{name}: N={pts.shape[0]} {pts.dtype} pc={augment_pc} n_out={aug.shape[0]} "
          f"kept={bv_index.shape[0]} voxels={vd['number_buffer'].shape[0]} "
          f"capped={(vd['number_buffer'] >= 45).sum()} bytes={os.path.getsize(out)}")
    return aug, bv_index


# ------------------------------------------------------------------ planted set

RANGES = {"x": (-20.0, 20 - 0.01, 0.2), "y": (-1.0, 3 - 0.01, 0.4), "z": (0.0, 48 - 0.01, 0.2)}


def _augment_f32(p, params, rot):
    """augment_voxel's cloud half on an f32 cloud (this machine's numpy), and the
    same steps carried in f64 with no rounding to f32 in between."""
    sx, sz, ratio = params[:3]
    a = p.copy()
    a[:, 0] += np.float64(sx)
    a[:, 2] += np.float64(sz)
    a[:, 0:3] *= np.array([ratio])
    a[:, [0, 2]] = np.dot(rot, a[:, [0, 2]].transpose()).transpose()
    u = p.astype(np.float64)
    u[:, 0] += sx
    u[:, 2] += sz
    u[:, 0:3] *= ratio
    u[:, [0, 2]] = np.dot(rot, u[:, [0, 2]].transpose()).transpose()
    return a, u


def _cell(v, lo, hi, res):
    """(inside the strict range, voxel index) of coordinate values v, evaluated as
    construct_voxel.py:89-118 does for v's dtype (python-float bounds)."""
    inside = np.logical_and(v > lo, v < hi)
    return inside, ((v - lo) / res).astype(np.int32)


def _planted(params, rot, rng):
    """f32 points whose augmented coordinate, rounded to f32 as the reference rounds
    it, falls in another voxel or on the other side of a strict range bound than
    the unrounded f64 value: found by walking the f32 neighbours of points aimed at
    voxel boundaries and range bounds. At least PLANTED_MIN per coordinate."""
    sx, sz, ratio = params[:3]
    found = {"x": [], "y": [], "z": []}
    for c, col in (("x", 0), ("y", 1), ("z", 2)):
        lo, hi, res = RANGES[c]
        nb = int((hi - lo) / res)
        tries = 0
        while len(found[c]) < PLANTED_MIN + 4 and tries < 4000:
            tries += 1
            k = int(rng.integers(0, nb + 1))
            target = (lo + k * res, lo, hi, lo + k * res)[tries % 4]  # voxel boundaries and both range bounds
            # a point whose augmented coordinate c is the target: invert rotation, scale and shift
            t = np.array([rng.uniform(-15, 15), rng.uniform(-0.5, 2.5), rng.uniform(3, 44)])
            t[col] = target
            x2, z2 = rot.T @ np.array([t[0], t[2]])
            p0 = np.array([x2 / ratio - sx, t[1] / ratio, z2 / ratio - sz, 0.5], dtype=np.float32)
            cand = np.repeat(p0[None], 65, axis=0)
            steps = np.arange(-32, 33)
            v = cand[:, col].copy()
            for _ in range(32):
                v = np.where(steps < 0, np.nextafter(v, np.float32(-np.inf)), v)
                v = np.where(steps > 0, np.nextafter(v, np.float32(np.inf)), v)
                steps = steps - np.sign(steps)
            cand[:, col] = v
            a, u = _augment_f32(cand, params, rot)
            ia, ca = _cell(a[:, col], lo, hi, res)
            iu, cu = _cell(u[:, col], lo, hi, res)
            bad = np.logical_or(ia != iu, np.logical_and(ia, ca != cu))
            for j in np.nonzero(bad)[0][:2]:
                found[c].append(cand[j])
    counts = {c: len(v) for c, v in found.items()}
    assert all(n >= PLANTED_MIN for n in counts.values()), counts
    return np.array(found["x"] + found["y"] + found["z"], dtype=np.float32), counts


def _one_point_f64(seed, rng):
    """A one-point f64 cloud whose rotation tells np.dot's one-column order from its
    many-column order and from two products and one add."""
    params, rot, _ = _draws(seed, SCALE, 1, False)
    sx, sz, ratio = params[:3]
    while True:
        p = np.array([[rng.uniform(-15, 15), rng.uniform(0, 2), rng.uniform(3, 40), 0.3]])
        a = p.copy()
        a[:, 0] += sx
        a[:, 2] += sz
        a[:, 0:3] *= ratio
        col = a[:, [0, 2]].transpose()
        one = np.dot(rot, col)[:, 0]
        many = np.dot(rot, np.repeat(a[:, [0, 2]], 2, axis=0).transpose())[:, 0]
        plain = rot[:, 0] * col[0, 0] + rot[:, 1] * col[1, 0]
        if (one != many).any() and (one != plain).any():
            return p


def main():
    ref = _reference()
    rng = np.random.default_rng(41)
    n = 3000
    _case(ref, "f64", _cloud(rng, n), 101, False, rng)
    _case(ref, "f64_pc", _cloud(rng, n), 102, True, rng)
    _case(ref, "f32", _cloud(rng, n).astype(np.float32), 103, False, rng)
    _case(ref, "f32_pc", _cloud(rng, n).astype(np.float32), 104, True, rng)
    _case(ref, "dense", _cloud(rng, 7000, dense=True).astype(np.float32), 105, True, rng)
    _case(ref, "one_f64", _one_point_f64(106, rng), 106, False, rng)
    _case(ref, "one_f32", np.array([[-3.3, 1.1, 20.7, 0.3]], dtype=np.float32), 107, False, rng)
    far = _cloud(rng, 500).astype(np.float32)
    far[:, 2] += 60.0
    aug, bv = _case(ref, "none", far, 108, True, rng)
    assert bv.shape[0] == 0
    # planted: the draws do not depend on the cloud without AUGMENT_PC, so they are known before it is built
    params, rot, _ = _draws(109, SCALE, 0, False)
    planted, counts = _planted(params, rot, rng)
    cloud = _cloud(rng, 2000).astype(np.float32)
    at = rng.choice(cloud.shape[0], planted.shape[0], replace=False)
    cloud[at] = planted
    aug, _ = _case(ref, "planted", cloud, 109, False, rng)
    # the reference's own cloud shows the planted property
    _, u = _augment_f32(cloud, params, rot)
    for c, col in (("x", 0), ("y", 1), ("z", 2)):
        lo, hi, res = RANGES[c]
        ia, ca = _cell(aug[:, col], lo, hi, res)
        iu, cu = _cell(u[:, col], lo, hi, res)
        nbad = int(np.logical_or(ia != iu, np.logical_and(ia, ca != cu)).sum())
        print(f"planted {c}: {nbad} points (searched {counts[c]})")
        assert nbad >= PLANTED_MIN, (c, nbad)


if __name__ == "__main__":
    main()
