"""MV3D_TF's SHPL entry points on MI355X.

* ``produce_sparse_pooling_input`` mirrors
  ``fusion_voxel_train.produce_sparse_pooling_input``
  (MV3D_TF_release/lib/networks/MV3D_voxel_train.py:89-91): same argument
  order, default stride ``[8, 2]`` (``_feat_stride_pool``: image stride 8,
  BEV stride 2, :14), returns ``(Mij, M_val, M_size, img_index_flip)``.
* ``sparse_pool`` mirrors the ``@layer sparse_pool`` of
  MV3D_TF_release/lib/networks/network.py:243-246:
  ``input = [M, img_features, img_index_flip]``.
* ``calib_to_P`` / ``calib_to_L2C`` mirror MV3D_TF_release/lib/utils/
  transform.py:13-30: the camera matrix the minibatch projects with
  (minibatch_mv3d_img.py:89) from the imdb's 4x12 calib rows.

* ``augment_voxel`` mirrors the training minibatch's augmentation of that name
  (MV3D_TF_release/lib/roi_data_layer/minibatch_mv3d_img.py:132-189, on by
  default through cfg.TRAIN.AUGMENT_BV): ``draw_voxel_aug`` repeats its draws,
  ``augment_voxel_boxes`` its ground-truth half on the host, and the cloud half
  runs on the device -- written out (``augment_points``) or fused into the
  producer (``mv3d_voxels_batch(vox_aug=...)``).

M_val here is the MV3D voxel weight 1/count (construct_voxel.py:160); it is
carried unchanged to the pull kernels, which then compute per-voxel means
summed over the z-voxels of a BEV cell.
"""
from . import sparse_pool_utils as spu

_feat_stride_pool = [8, 2]  # 0 is img, 1 is bv (MV3D_voxel_train.py:14)


def produce_sparse_pooling_input(img_index, im_size, bv_index, bv_size, M_val=None,
                                 stride=_feat_stride_pool):
    out = spu.produce_sparse_pooling_input({'img_index': img_index, 'img_size': im_size,
                                            'bv_index': bv_index, 'bv_size': bv_size},
                                           M_val=M_val, stride=stride)
    return out['Mij_pool'], out['M_val'], out['M_size'], out['img_index_flip_pool']


def sparse_pool(input, pooled_size):  # noqa: A002 (reference signature)
    """0 is the sparse matrix M, 1 the source feature map, 2 the pooling index."""
    return spu._sparse_pool_op(input[0], input[1], input[2], pooled_size)


def calib_to_P(calib, from_camera=False):
    """Lidar (or camera, from_camera=True) coordinates -> image: the 3x4 P with
    uvw = P [X; Y; Z; 1]. calib rows (imdb layout): 0 = P2 (3x4), 2 = R0 read
    as 4x3 and closed by the column [0, 0, 0, 1], 3 = Tr_velo_to_cam (3x4)
    closed by the row [0, 0, 0, 1]; P = (P2 . R0) . C2V, evaluated in that
    association (numpy matmul) like transform.py:22-23."""
    import numpy as np
    calib = np.asarray(calib, dtype=np.float64)
    p2 = calib[0].reshape(3, 4)
    if from_camera:
        return p2
    return np.matmul(np.matmul(p2, _r0_4x4(calib)), _c2v_4x4(calib))


def calib_to_L2C(calib):
    """Lidar -> camera frame: R0 . C2V (transform.py:26-30), both closed to 4x4."""
    import numpy as np
    calib = np.asarray(calib, dtype=np.float64)
    return np.matmul(_r0_4x4(calib), _c2v_4x4(calib))


def _r0_4x4(calib):
    import numpy as np
    return np.concatenate([calib[2].reshape(4, 3), np.array([[0.0], [0.0], [0.0], [1.0]])], axis=1)


def _c2v_4x4(calib):
    import numpy as np
    return np.concatenate([calib[3].reshape(3, 4), np.array([[0.0, 0.0, 0.0, 1.0]])], axis=0)


# MV3D voxel config (MV3D_TF_release/lib/utils/config_voxels.py:49-59, DETECT_OBJ != 'Car')
# and the ranges construct_voxel.py:11-13 derives from it.
PED_RANGES = (0.0, 48 - 0.01, -20.0, 20 - 0.01, -1.0, 3 - 0.01)   # fwd, side, height
CAR_RANGES = (0.0, 70.4 - 0.01, -40.0, 40 - 0.01, -1.0, 3 - 0.01)


def draw_voxel_aug(scale, n_points=None, augment_pc=False):
    """augment_voxel's draws from the global np.random, in its order (minibatch_mv3d_img.py:134-136, :171-172):
    uniform(-scale, scale, 2), uniform(0.95, 1.05, 1), uniform(-pi/10, pi/10, 1) and, with augment_pc
    (cfg.TRAIN.AUGMENT_PC), uniform(0.9, 1.0, 1) then choice(n, int(n * rate)) -- a seeded script draws what the
    reference draws. Returns dict(sx, sz, ratio [1], angle [1], rot [2,2] = [[cos, sin], [-sin, cos]],
    remain_index (i64 [n'] or None))."""
    import numpy as np
    sx, sz = np.random.uniform(-scale, scale, 2)
    ratio = np.random.uniform(0.95, 1.05, 1)
    angle = np.random.uniform(-np.pi / 10, np.pi / 10, 1)
    remain = None
    if augment_pc:
        if n_points is None:
            raise ValueError("augment_pc redraws the cloud: n_points is needed")
        rate = np.random.uniform(0.9, 1.0, 1)
        remain = np.asarray(np.random.choice(int(n_points), int(n_points * rate[0])), dtype=np.int64)
    c, sn = np.cos(angle[0]), np.sin(angle[0])
    return {"sx": sx, "sz": sz, "ratio": ratio, "angle": angle, "rot": np.array([[c, sn], [-sn, c]]),
            "remain_index": remain}


def vox_aug_rows(params):
    """The device's per-frame parameters [F, 8] f64 (sx, sz, ratio, r00, r01, r10, r11, 0) from one
    draw_voxel_aug dict per frame."""
    import numpy as np
    return np.array([[q["sx"], q["sz"], np.asarray(q["ratio"]).reshape(-1)[0], *np.asarray(q["rot"]).reshape(4), 0.0]
                     for q in params], dtype=np.float64).reshape(-1, 8)


def augment_voxel_boxes(blobs, params):
    """augment_voxel's ground-truth half (minibatch_mv3d_img.py:138-147), in place on the host:
    blobs['gt_boxes_3d'] [k, 7] (x, y, z, l, w, h, cls) is shifted by (sx, sz) in x and z, its first six columns
    are scaled by the ratio, (x, z) is rotated by rot; blobs['gt_rys'] gains the angle. The operands are numpy
    f64 scalars and arrays, as the reference's draws are, so the rounding to the boxes' dtype is numpy's own."""
    import numpy as np
    boxes = blobs["gt_boxes_3d"]
    boxes[:, 0] += np.float64(params["sx"])
    boxes[:, 2] += np.float64(params["sz"])
    boxes[:, 0:6] *= np.asarray(params["ratio"], dtype=np.float64).reshape(1)
    xz = np.dot(np.asarray(params["rot"], dtype=np.float64), boxes[:, [0, 2]].transpose())
    boxes[:, [0, 2]] = xz.transpose()
    blobs["gt_rys"] += np.asarray(params["angle"], dtype=np.float64).reshape(1)
    return blobs


def _aug_args(points, point_offsets, vox_aug, remain_index, remain_offsets):
    """Device tensors of the augmented calls: (points f32/f64, offsets, vox_aug [F,8], remain, roff, dtype code, N_out)."""
    import torch

    from . import _lib as L
    dev = points.device
    if points.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"augment_voxel's cloud is float32 or float64, got {points.dtype}")
    points = points.contiguous()
    point_offsets = point_offsets.to(torch.int64).contiguous()
    F = int(point_offsets.numel()) - 1
    vox_aug = torch.as_tensor(vox_aug, dtype=torch.float64).to(dev).reshape(-1, 8).contiguous()
    if vox_aug.shape[0] != F:
        raise ValueError(f"vox_aug has {vox_aug.shape[0]} rows for {F} frames")
    if (remain_index is None) != (remain_offsets is None):
        raise ValueError("remain_index and remain_offsets go together")
    n_out = int(points.shape[0])
    if remain_index is not None:
        remain_index = torch.as_tensor(remain_index, dtype=torch.int64).to(dev).contiguous()
        remain_offsets = torch.as_tensor(remain_offsets, dtype=torch.int64).to(dev).contiguous()
        if remain_offsets.numel() != F + 1:
            raise ValueError(f"remain_offsets has {remain_offsets.numel()} entries for {F} frames")
        n_out = int(remain_index.numel())
    code = L.F32 if points.dtype == torch.float32 else L.F64
    return points, point_offsets, vox_aug, remain_index, remain_offsets, code, n_out


def augment_points(points, point_offsets, P, vox_aug, remain_index=None, remain_offsets=None):
    """augment_voxel's cloud half for a batch of frames, written out (shpl_mv3d_augment_points): points [N, >=4]
    f32 or f64 device tensor, P [F,3,4], vox_aug [F,8] (vox_aug_rows), optional remain_index / remain_offsets
    (frame-local i64 indices and their [F+1] offsets). Returns dict(points [N_out,4] f64, img_index2 [2,N_out]
    i64, offsets [F+1], err [1] i32 device word: _lib.EBIT_GATHER)."""
    import torch

    from . import _lib as L
    dev = points.device
    points, point_offsets, vox_aug, remain_index, remain_offsets, code, n_out = _aug_args(
        points, point_offsets, vox_aug, remain_index, remain_offsets)
    P = torch.as_tensor(P, dtype=torch.float64).to(dev).contiguous()
    F = int(point_offsets.numel()) - 1
    cap = max(n_out, 1)
    cloud = torch.empty((cap, 4), dtype=torch.float64, device=dev)
    img2 = torch.empty((2, cap), dtype=torch.int64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    L.check(L.lib().shpl_mv3d_augment_points(F, L.ptr(point_offsets), int(points.shape[0]), L.ptr(points), code,
                                             int(points.stride(0)), L.ptr(P), L.ptr(vox_aug), L.ptr(remain_index),
                                             L.ptr(remain_offsets), n_out, L.ptr(cloud), L.ptr(img2), cap, L.ptr(err),
                                             L.stream_of(dev)), "shpl_mv3d_augment_points")
    return {"points": cloud[:n_out], "img_index2": img2[:, :n_out],
            "offsets": point_offsets if remain_offsets is None else remain_offsets, "err": err}


def augment_voxel(blobs, scale=0.5, lidar_pc=None, calib=None, augment_pc=False):
    """augment_voxel (minibatch_mv3d_img.py:132-189) with the reference's signature and return value; augment_pc
    stands for cfg.TRAIN.AUGMENT_PC. The draws come from the global np.random in the reference's order, the boxes
    are augmented on the host in place, and with a cloud (numpy or tensor [N, >=4], f32 or f64, camera frame)
    the return is (blobs, cloud [N',4] f64 device tensor, img_index2 [2,N'] i64 device tensor) from the device
    kernel; without one, blobs. A cloud of another dtype is taken as f64."""
    import numpy as np
    import torch

    from . import _lib as L
    n = None if lidar_pc is None else int(lidar_pc.shape[0])
    params = draw_voxel_aug(scale, n, augment_pc and lidar_pc is not None)
    augment_voxel_boxes(blobs, params)
    if lidar_pc is None:
        return blobs
    dev = torch.device("cuda", torch.cuda.current_device())
    pts = lidar_pc if isinstance(lidar_pc, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(lidar_pc))
    if pts.dtype not in (torch.float32, torch.float64):
        pts = pts.to(torch.float64)
    pts = pts.to(dev)
    off = torch.tensor([0, n], dtype=torch.int64, device=dev)
    remain = params["remain_index"]
    roff = None if remain is None else torch.tensor([0, len(remain)], dtype=torch.int64, device=dev)
    out = augment_points(pts, off, np.asarray(calib_to_P(calib, from_camera=True)).reshape(1, 12), vox_aug_rows([params]),
                         remain, roff)
    if int(out["err"].item()) & L.EBIT_GATHER:
        raise IndexError("augment_voxel: a remain_index entry lies outside the cloud")
    return blobs, out["points"], out["img_index2"]


def mv3d_voxels_batch(points, point_offsets, img_index2=None, P=None, ranges=PED_RANGES, res=0.2, zres=0.4,
                      voxel_point_count=45, number_buffer=False, fv_aug=None, vox_aug=None, remain_index=None,
                      remain_offsets=None):
    """The SHPL outputs of point_cloud_2_top_sparse (construct_voxel.py:37-162)
    for a batch of frames on the device. points [N, >=3] f64 camera frame;
    img_index2 [2, N] i64 (or P [F,3,4] f64 to project on the device);
    fv_aug [F,3] f64 (expansion_ratio, sx, sy): augment_fv's index transform
    (minibatch_mv3d_img.py:191-209) applied to img_index.
    vox_aug [F,8] f64 (vox_aug_rows), with optional remain_index / remain_offsets: augment_voxel fused in -- the
    voxels are keyed on the augmented coordinates, the image index comes from the original points, and neither
    the augmented cloud nor its img_index2 is written. points is then an f32 or f64 tensor and keeps its type
    (the reference rounds to it); the outputs are laid out by out point (offsets = remain_offsets), and the dict
    gains offsets [F+1] and err [1] i32 (_lib.EBIT_GATHER: a remain_index entry outside its frame, skipped).
    Returns dict(img_index [3,N] f64, bv_index [N,2] i64, M_val [N] f64,
    frame_n [F]; number_buffer [N] i32 + frame_nvox [F]), capacity layout."""
    import ctypes

    import numpy as np
    import torch

    from . import _lib as L
    dev = points.device
    if vox_aug is None:
        if remain_index is not None or remain_offsets is not None:
            raise ValueError("remain_index is augment_voxel's redraw: it needs vox_aug")
        points = points.to(torch.float64).contiguous()
        point_offsets = point_offsets.to(torch.int64).contiguous()
        n_out = int(points.shape[0])
    else:
        points, point_offsets, vox_aug, remain_index, remain_offsets, code, n_out = _aug_args(
            points, point_offsets, vox_aug, remain_index, remain_offsets)
    if img_index2 is not None:
        img_index2 = img_index2.to(torch.int64).contiguous()
    if P is not None:
        P = P.to(torch.float64).contiguous()
    if fv_aug is not None:
        fv_aug = torch.as_tensor(fv_aug, dtype=torch.float64).to(dev).reshape(-1, 3).contiguous()
    F = int(point_offsets.numel()) - 1
    N = int(points.shape[0])
    cap = max(n_out, 1)
    img = torch.empty((3, cap), dtype=torch.float64, device=dev)
    bv = torch.empty((cap, 2), dtype=torch.int64, device=dev)
    mv = torch.empty(cap, dtype=torch.float64, device=dev)
    fn = torch.empty(F, dtype=torch.int64, device=dev)
    nb = torch.empty(cap, dtype=torch.int32, device=dev) if number_buffer else None
    nvox = torch.empty(F, dtype=torch.int64, device=dev) if number_buffer else None
    ws = L.workspace(L.ws_bytes("shpl_mv3d", n_out), dev)
    rng = np.ascontiguousarray(ranges, dtype=np.float64)
    out = {"img_index": img, "bv_index": bv, "M_val": mv, "frame_n": fn, "number_buffer": nb, "frame_nvox": nvox}
    # what the two C calls share; the augmented one has its dtype, draws, gather and error word in between
    head = (F, L.ptr(point_offsets), N, L.ptr(points))
    source = (int(points.stride(0)), L.ptr(img_index2), L.ptr(P), L.ptr(fv_aug))
    grid = (rng.ctypes.data_as(ctypes.c_void_p), float(res), float(zres), int(voxel_point_count))
    outputs = (L.ptr(img), cap, L.ptr(bv), L.ptr(mv), L.ptr(fn), L.ptr(nb), L.ptr(nvox))
    tail = (L.ptr(ws), ws.numel(), L.stream_of(dev))
    if vox_aug is None:
        L.check(L.lib().shpl_mv3d_voxels(*head, *source, *grid, *outputs, *tail), "shpl_mv3d_voxels")
        return out
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    L.check(L.lib().shpl_mv3d_voxels_aug(*head, code, *source, L.ptr(vox_aug), L.ptr(remain_index),
                                         L.ptr(remain_offsets), n_out, *grid, *outputs, L.ptr(err), *tail),
            "shpl_mv3d_voxels_aug")
    out["offsets"] = point_offsets if remain_offsets is None else remain_offsets
    out["err"] = err
    return out


def mv3d_sparse_pooling_input(points, img_index2=None, P=None, ranges=PED_RANGES, res=0.2, zres=0.4,
                              voxel_point_count=45, fv_aug=None, vox_aug=None, remain_index=None):
    """One frame: (img_index [3,n'], bv_index [n',2], M_val [n']) as
    point_cloud_2_top_sparse returns them (construct_voxel.py:156-162).
    vox_aug [8] (vox_aug_rows of one draw), optional remain_index: augment_voxel fused in; an f32 cloud stays
    f32 then (other dtypes are taken as f64)."""
    import numpy as np
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    points = np.asarray(points)
    keep32 = vox_aug is not None and points.dtype == np.float32
    pts = torch.as_tensor(np.ascontiguousarray(points, dtype=np.float32 if keep32 else np.float64)).to(dev)
    off = torch.tensor([0, pts.shape[0]], dtype=torch.int64, device=dev)
    i2 = None if img_index2 is None else torch.as_tensor(np.ascontiguousarray(img_index2, dtype=np.int64)).to(dev)
    Pd = None if P is None else torch.as_tensor(np.asarray(P, dtype=np.float64).reshape(1, 12)).to(dev)
    roff = None if remain_index is None else torch.tensor([0, len(remain_index)], dtype=torch.int64, device=dev)
    out = mv3d_voxels_batch(pts, off, i2, Pd, ranges, res, zres, voxel_point_count,
                            fv_aug=None if fv_aug is None else np.asarray(fv_aug, dtype=np.float64).reshape(1, 3),
                            vox_aug=None if vox_aug is None else np.asarray(vox_aug, dtype=np.float64).reshape(1, 8),
                            remain_index=remain_index, remain_offsets=roff)
    k = int(out["frame_n"][0].item())
    return out["img_index"][:, :k], out["bv_index"][:k], out["M_val"][:k]
