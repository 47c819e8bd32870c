"""The ragged index build (shpl_build_index_ragged / shpl_build_index_buckets_ragged) against the uniform entry
points it stands beside, at two shapes:

  config3   4 frames x 20 k points, stride 8, bucketed, the one-launch k_index1
  config2   64 frames x 20 k points, stride 1, the two launches k_count + k_compact

Points are drawn inside the padded image 1242 x 376. Per shape three forms of FusedPipeline.build_index over the
same batch, alternated in one process over --repeats rounds:
  uniform       the existing entry at the padded size (the parent's kernels unchanged: the yardstick)
  ragged_equal  the ragged entry, every frame's size the padded size (the same M)
  ragged_kitti  the ragged entry, KITTI's four image sizes cycled over the frames
Each form is a captured graph of --inner index builds (no host launch gaps), timed with HIP events around --reps
replays after a warm-up replay. One JSON line per (shape, form): every round's us per build, min / median / max,
and for the ragged forms whether the median sits inside the uniform form's min-max spread. ragged_equal's index
arrays are compared with uniform's bit for bit.

    python scripts/time_ragged_index.py [--repeats 10] [--reps 40] [--inner 50] [--shape config3|config2|both]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparse_pooling_amd import _lib as L, pipeline, synth  # noqa: E402

PADDED = (1242, 376)
KITTI_SIZES = [(1242, 375), (1224, 370), (1238, 374), (1241, 376)]
SHAPES = {"config3": dict(frames=4, stride=(8, 8), kw=dict(rows=True, buckets=True)),
          "config2": dict(frames=64, stride=(1, 1), kw=dict(rows=False, buckets=False))}


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def run_shape(name, dev, repeats, reps, inner):
    sh = SHAPES[name]
    B, stride = sh["frames"], sh["stride"]
    spec = synth.FrameSpec(20000, PADDED, (704, 800), stride)
    dual = bool(sh["kw"]["buckets"])  # the bucketed step is the dual layer's (config 3)
    frames = [synth.make_frame(spec, seed=s, n_outside=200) for s in range(B)]
    pts, vox, off, P, maxp, N = pipeline.stack_frames(frames, dev)
    sizes = {"ragged_equal": [PADDED] * B, "ragged_kitti": [KITTI_SIZES[f % 4] for f in range(B)]}
    pls, graphs = {}, {}
    for form in ("uniform", "ragged_equal", "ragged_kitti"):
        pl = pipeline.FusedPipeline(B, maxp, N, PADDED, (704, 800), stride, 8, 8, device=dev, dual=dual,
                                    ragged=form != "uniform", **sh["kw"])
        if form != "uniform":
            pl.set_image_sizes(torch.tensor(sizes[form], dtype=torch.float64, device=dev))
        pl.build_index(pts, vox, off, P)
        torch.cuda.synchronize()
        gs = torch.cuda.Stream(device=dev)
        gs.wait_stream(torch.cuda.current_stream(dev))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=gs):
            for _ in range(inner):
                pl.build_index(pts, vox, off, P)
        g.replay()
        torch.cuda.synchronize()
        pl.check()
        pls[form], graphs[form] = pl, g
    us = {form: [] for form in graphs}
    for _ in range(repeats):  # alternated: every form sees the same machine state
        for form, g in graphs.items():
            us[form].append(timed(g.replay, reps) * 1e3 / inner)
    same = all(torch.equal(getattr(pls["uniform"], k), getattr(pls["ragged_equal"], k))
               for k in ("cell", "pix", "val", "frame_nnz", "frame_off"))
    lo, hi = min(us["uniform"]), max(us["uniform"])
    sha = hashlib.sha256(open(L.LIB_PATH, "rb").read()).hexdigest()[:16]
    for form, v in us.items():
        med = statistics.median(v)
        rec = {"shape": name, "form": form, "frames": B, "stride": stride[0], "points_per_frame": 20000,
               "bucketed": pls[form].buckets, "us_per_build": round(med, 3), "min": round(min(v), 3),
               "max": round(max(v), 3), "rounds": [round(x, 3) for x in v], "reps": reps, "inner": inner,
               "nnz": int(pls[form].frame_nnz.sum().item()), "lib_sha256": sha}
        if form != "uniform":
            rec["inside_uniform_spread"] = bool(lo <= med <= hi)
            rec["median_over_uniform"] = round(med / statistics.median(us["uniform"]), 4)
        if form == "ragged_equal":
            rec["equals_uniform"] = bool(same)
        print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--shape", choices=("config3", "config2", "both"), default="both")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_ragged_index.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    for name in ("config3", "config2") if args.shape == "both" else (args.shape,):
        run_shape(name, dev, args.repeats, args.reps, args.inner)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
