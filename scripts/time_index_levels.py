"""The index build for several fusion levels in one pass (shpl_build_index_levels) against the yardstick it stands
beside -- the unchanged shpl_build_index, called once per level -- for the AVOD pair (stride 1 over BEV 700 x 800,
stride 8 over the BEV input padded to 704 rows) at two shapes:

  avod      1 frame x 20 k points
  config2   64 frames x 20 k points

Points are drawn inside the image 1242 x 375 (200 more per frame outside it). Two forms over the same batch and the
same preallocated outputs, alternated in one process over --repeats rounds:
  per_level   one shpl_build_index call per level (the parent's kernels: k_count + k_compact, twice)
  levels      one shpl_build_index_levels call (k_count_levels + k_compact_levels)
Each form is a captured graph of --inner builds (no host launch gaps), timed with HIP events around --reps replays
after a warm-up replay. One JSON line per (shape, form): every round's us per frame batch, min / median / max, and
for `levels` whether its median lies outside per_level's min-max spread on the fast side. The two forms' arrays are
compared bit for bit.

    python scripts/time_index_levels.py [--repeats 10] [--reps 40] [--inner 50] [--shape avod|config2|both]
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

IM_SIZE = (1242, 375)
PAIR = [((1, 1), (700, 800)), ((8, 8), (704, 800))]
SHAPES = {"avod": 1, "config2": 64}


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


class Outputs:
    def __init__(self, N, B, dev):
        self.cell = torch.empty(N, dtype=torch.int32, device=dev)
        self.pix = torch.empty(N, dtype=torch.int32, device=dev)
        self.val = torch.empty(N, dtype=torch.float32, device=dev)
        self.nnz = torch.empty(B, dtype=torch.int64, device=dev)

    def tensors(self):
        return (self.cell, self.pix, self.val, self.nnz)


def run_shape(name, dev, repeats, reps, inner):
    B = SHAPES[name]
    spec = synth.FrameSpec(20000, IM_SIZE, (704, 800), (1, 1))
    frames = [synth.make_frame(spec, seed=s, n_outside=200) for s in range(B)]
    pts, vox, off, P, maxp, N = pipeline.stack_frames(frames, dev)
    outs = {form: [Outputs(N, B, dev) for _ in PAIR] for form in ("per_level", "levels")}
    fo = torch.empty(B + 1, dtype=torch.int64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    ws1 = L.workspace(L.index_ws_bytes(B, maxp), dev)
    wsl = L.workspace(L.index_levels_ws_bytes(B, maxp, len(PAIR)), dev)
    lib = L.lib()

    def per_level():
        for (stride, bv_size), o in zip(PAIR, outs["per_level"]):
            lead = L.index_args(B, off, None, maxp, pts, vox, P, IM_SIZE, bv_size, stride, None, o.cell, o.pix, o.val)
            L.check(lib.shpl_build_index(*lead, None, None, L.ptr(o.nnz), L.ptr(fo), L.ptr(err), L.ptr(ws1),
                                         ws1.numel(), L.stream_of(dev)), "shpl_build_index")

    arr = L.index_levels([(s, b, o.cell, o.pix, o.val, None, None, o.nnz) for (s, b), o in zip(PAIR, outs["levels"])])
    lead = L.index_args(B, off, None, maxp, pts, vox, P, IM_SIZE, (0, 0), (1, 1), None, None, None, None)

    def levels():
        L.check(lib.shpl_build_index_levels(*lead[:12], None, len(PAIR), arr, L.ptr(fo), L.ptr(err), L.ptr(wsl),
                                            wsl.numel(), L.stream_of(dev)), "shpl_build_index_levels")

    graphs = {}
    for form, fn in (("per_level", per_level), ("levels", levels)):
        fn()
        torch.cuda.synchronize()
        gs = torch.cuda.Stream(device=dev)
        gs.wait_stream(torch.cuda.current_stream(dev))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=gs):
            for _ in range(inner):
                fn()
        g.replay()
        torch.cuda.synchronize()
        graphs[form] = g
    assert int(err.item()) == 0
    us = {form: [] for form in graphs}
    for _ in range(repeats):  # alternated: every form sees the same machine state
        for form, g in graphs.items():
            us[form].append(timed(g.replay, reps) * 1e3 / inner)
    same = all(torch.equal(a.view(torch.uint8), b.view(torch.uint8))
               for oa, ob in zip(outs["per_level"], outs["levels"]) for a, b in zip(oa.tensors(), ob.tensors()))
    lo, hi = min(us["per_level"]), max(us["per_level"])
    sha = hashlib.sha256(open(L.LIB_PATH, "rb").read()).hexdigest()[:16]
    for form, v in us.items():
        med = statistics.median(v)
        rec = {"shape": name, "form": form, "frames": B, "points_per_frame": 20000,
               "levels": [[list(s), list(b)] for s, b in PAIR], "us_per_batch": round(med, 3), "min": round(min(v), 3),
               "max": round(max(v), 3), "rounds": [round(x, 3) for x in v], "reps": reps, "inner": inner,
               "nnz": [int(o.nnz.sum().item()) for o in outs[form]], "lib_sha256": sha}
        if form == "levels":
            rec["faster_than_per_level_spread"] = bool(med < lo)
            rec["inside_per_level_spread"] = bool(lo <= med <= hi)
            rec["median_over_per_level"] = round(med / statistics.median(us["per_level"]), 4)
            rec["equals_per_level"] = bool(same)
        print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--shape", choices=("avod", "config2", "both"), default="both")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_index_levels.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    for name in ("avod", "config2") if args.shape == "both" else (args.shape,):
        run_shape(name, dev, args.repeats, args.reps, args.inner)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
