"""Times MV3D's training augmentation augment_voxel (minibatch_mv3d_img.py:132-189) in front of the producer
point_cloud_2_top_sparse, at a training batch's size: 8 frames of 120 k f32 points already on the device (the
KITTI loader's output), the camera matrices and the per-frame draws. Three routes, alternated in one process
after a warm-up, each repeat between two host clock readings around work that ends in a device synchronise
(route a has host work, so device events alone would not be comparable):

  host          what a caller could do before the device kernels: the cloud back to the host, numpy's
                project / shift / scale / rotate per frame, the augmented cloud and img_index2 uploaded, then
                mv3d_voxels_batch(img_index2=...);
  materialised  mv3d.augment_points (one streaming launch writing the cloud and img_index2), then the same producer;
  fused         mv3d_voxels_batch(vox_aug=...): the producer reads the original points and augments in registers.

One JSON line per route: every repeat's time, their median and spread, the points kept, whether the route's
outputs equal the fused route's, and the library's hash. --augment-pc adds cfg.TRAIN.AUGMENT_PC's redraw
(a gather through remain_index on the device, fancy indexing on the host). SHPL_LIB selects a variant build.

    python scripts/time_mv3d_augment.py [--frames 8] [--points 120000] [--reps 10] [--augment-pc]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparse_pooling_amd import _lib as L, mv3d, synth  # noqa: E402


def lib_sha256():
    with open(L.LIB_PATH, "rb") as fh:
        return hashlib.sha256(fh.read()).hexdigest()[:16]


def host_augment(pc, P, q):
    """One frame on the host in numpy, as a caller without the device kernels would write it."""
    if q["remain_index"] is not None:
        pc = pc[q["remain_index"]]
    else:
        pc = pc.copy()
    uvw = np.dot(P, np.vstack((pc[:, 0:3].transpose(), np.ones((1, pc.shape[0])))))
    img2 = np.round(uvw[0:2] / uvw[2]).astype(np.int64)
    pc[:, 0] += q["sx"]
    pc[:, 2] += q["sz"]
    pc[:, 0:3] *= q["ratio"]
    pc[:, [0, 2]] = np.dot(q["rot"], pc[:, [0, 2]].transpose()).transpose()
    return pc, img2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--augment-pc", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_mv3d_augment.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    F, n = args.frames, args.points
    rng = np.random.default_rng(5)
    cloud = np.stack([rng.uniform(-21, 21, F * n), rng.uniform(-1.2, 3.2, F * n), rng.uniform(-0.5, 49, F * n),
                      rng.uniform(0, 1, F * n)], axis=1).astype(np.float32)
    np.random.seed(5)
    draws = [mv3d.draw_voxel_aug(0.8, n, args.augment_pc) for _ in range(F)]
    P_host = np.stack([synth.KITTI_P2] * F)
    pts = torch.from_numpy(cloud).to(dev)
    off = torch.arange(F + 1, dtype=torch.int64, device=dev) * n
    P = torch.from_numpy(P_host.reshape(F, 12)).to(dev)
    vox = torch.from_numpy(mv3d.vox_aug_rows(draws)).to(dev)
    remain = roff = None
    if args.augment_pc:
        remain = torch.from_numpy(np.concatenate([q["remain_index"] for q in draws])).to(dev)
        roff = torch.from_numpy(np.cumsum([0] + [len(q["remain_index"]) for q in draws])).to(dev)

    def host():
        pc = pts.cpu().numpy()
        out = [host_augment(pc[f * n:(f + 1) * n], P_host[f], draws[f]) for f in range(F)]
        o = np.cumsum([0] + [a.shape[0] for a, _ in out])
        return mv3d.mv3d_voxels_batch(torch.from_numpy(np.concatenate([a for a, _ in out])).to(dev),
                                      torch.from_numpy(o).to(dev),
                                      img_index2=torch.from_numpy(np.concatenate([i for _, i in out], axis=1)).to(dev))

    def materialised():
        m = mv3d.augment_points(pts, off, P, vox, remain, roff)
        return mv3d.mv3d_voxels_batch(m["points"], m["offsets"], img_index2=m["img_index2"])

    def fused():
        return mv3d.mv3d_voxels_batch(pts, off, P=P, vox_aug=vox, remain_index=remain, remain_offsets=roff)

    routes = {"host": host, "materialised": materialised, "fused": fused}
    ooff = (off if roff is None else roff).cpu().numpy()

    def kept_rows(o):
        fn = o["frame_n"].cpu().numpy()
        rows = [np.concatenate([o["img_index"][:2, ooff[f]:ooff[f] + fn[f]].cpu().numpy().T,
                                o["bv_index"][ooff[f]:ooff[f] + fn[f]].cpu().numpy().astype(np.float64),
                                o["M_val"][ooff[f]:ooff[f] + fn[f], None].cpu().numpy()], axis=1) for f in range(F)]
        return fn, np.concatenate(rows)

    for _ in range(args.warmup):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    ref_n, ref_rows = kept_rows(fused())
    same = {}
    for k, fn in routes.items():
        kn, rows = kept_rows(fn())
        same[k] = bool(np.array_equal(kn, ref_n) and np.array_equal(rows, ref_rows))
    ms = {k: [] for k in routes}
    for _ in range(args.reps):  # alternated: every route sees the same machine state
        for k, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    sha = lib_sha256()
    for k in routes:
        print(json.dumps({"step": "mv3d_augment_voxel", "route": k, "frames": F, "points_per_frame": n,
                          "cloud": "f32", "augment_pc": args.augment_pc, "kept": int(ref_n.sum()),
                          "ms_median": round(statistics.median(ms[k]), 4), "ms_min": round(min(ms[k]), 4),
                          "ms_max": round(max(ms[k]), 4), "ms": [round(v, 4) for v in ms[k]],
                          "equals_fused": same[k], "lib_sha256": sha, "lib": os.environ.get("SHPL_LIB", "default")}),
              flush=True)


if __name__ == "__main__":
    main()
