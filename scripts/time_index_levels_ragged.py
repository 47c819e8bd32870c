"""The index build for several fusion levels over a batch of mixed image sizes (shpl_build_index_levels_ragged)
against the only correct route without it -- the unchanged shpl_build_index_ragged, called once per level -- and
against the uniform shpl_build_index_levels, for the AVOD pair (stride 1 over BEV 700 x 800, stride 8 over the BEV
input padded to 704 rows) at two shapes:

  avod      1 frame x 20 k points
  config2   64 frames x 20 k points

Points are drawn inside the padded image 1242 x 376 (200 more per frame outside it); KITTI's four image sizes are
cycled over the frames. Four forms over the same batch and preallocated outputs, alternated in one process over
--repeats rounds:
  per_level        (a) one shpl_build_index_ragged call per level (4 launches), the frames' own sizes
  levels_ragged    (b) one shpl_build_index_levels_ragged call (2 launches), the frames' own sizes
  levels_ragged_eq     (b) with every size equal to the padded size
  levels_uniform   (c) shpl_build_index_levels at the padded size: what raggedness costs is (b, equal) - (c)
Each form is a captured graph of --inner builds (no host launch gaps), timed with HIP events around --reps replays
after a warm-up replay. One JSON line per (shape, form): every round's us per frame batch, min / median / max;
for levels_ragged whether its median lies outside per_level's min-max spread on the fast side and whether its
arrays equal per_level's bit for bit; for levels_ragged_eq the same against levels_uniform.

    python scripts/time_index_levels_ragged.py [--repeats 10] [--reps 40] [--inner 50] [--shape avod|config2|both]
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
PAIR = [((1, 1), (700, 800)), ((8, 8), (704, 800))]
MAPS = [(int(PADDED[1] // s[0]), int(PADDED[0] // s[0])) for s, _ in PAIR]
SHAPES = {"avod": 1, "config2": 64}
FORMS = ("per_level", "levels_ragged", "levels_ragged_eq", "levels_uniform")


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


def same(a, b):
    return all(torch.equal(x.view(torch.uint8), y.view(torch.uint8))
               for oa, ob in zip(a, b) for x, y in zip(oa.tensors(), ob.tensors()))


def run_shape(name, dev, repeats, reps, inner):
    B = SHAPES[name]
    spec = synth.FrameSpec(20000, PADDED, (704, 800), (1, 1))
    frames = [synth.make_frame(spec, seed=s, n_outside=200) for s in range(B)]
    pts, vox, off, P, maxp, N = pipeline.stack_frames(frames, dev)
    own = torch.tensor([KITTI_SIZES[f % 4] for f in range(B)], dtype=torch.float64, device=dev)
    equal = torch.tensor([PADDED] * B, dtype=torch.float64, device=dev)
    outs = {form: [Outputs(N, B, dev) for _ in PAIR] for form in FORMS}
    fo = torch.empty(B + 1, dtype=torch.int64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    ws1 = L.workspace(L.index_ws_bytes(B, maxp), dev)
    wsl = L.workspace(L.index_levels_ws_bytes(B, maxp, len(PAIR)), dev)
    lib = L.lib()
    tail = (L.ptr(fo), L.ptr(err), L.ptr(wsl), wsl.numel())  # (the stream is read per call: the capturing one)

    def per_level():
        for (stride, bv_size), hw, o in zip(PAIR, MAPS, outs["per_level"]):
            lead = L.index_args_ragged(B, off, None, maxp, pts, vox, P, own, hw, bv_size, stride, None, o.cell, o.pix,
                                       o.val)
            L.check(lib.shpl_build_index_ragged(*lead, None, None, L.ptr(o.nnz), L.ptr(fo), L.ptr(err), L.ptr(ws1),
                                                ws1.numel(), L.stream_of(dev)), "shpl_build_index_ragged")

    arrs = {form: L.index_levels([(s, b, o.cell, o.pix, o.val, None, None, o.nnz)
                                  for (s, b), o in zip(PAIR, outs[form])]) for form in FORMS[1:]}
    maps = L.index_level_maps(MAPS)
    lead = L.index_args(B, off, None, maxp, pts, vox, P, PADDED, (0, 0), (1, 1), None, None, None, None)

    def ragged(form, sizes):
        def fn():
            L.check(lib.shpl_build_index_levels_ragged(*lead[:10], L.ptr(sizes), None, len(PAIR), arrs[form], maps,
                                                       *tail, L.stream_of(dev)), "shpl_build_index_levels_ragged")
        return fn

    def uniform():
        L.check(lib.shpl_build_index_levels(*lead[:12], None, len(PAIR), arrs["levels_uniform"], *tail,
                                            L.stream_of(dev)), "shpl_build_index_levels")

    fns = {"per_level": per_level, "levels_ragged": ragged("levels_ragged", own),
           "levels_ragged_eq": ragged("levels_ragged_eq", equal), "levels_uniform": uniform}
    graphs = {}
    for form in FORMS:
        fn = fns[form]
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
    us = {form: [] for form in FORMS}
    for _ in range(repeats):  # alternated: every form sees the same machine state
        for form in FORMS:
            us[form].append(timed(graphs[form].replay, reps) * 1e3 / inner)
    sha = hashlib.sha256(open(L.LIB_PATH, "rb").read()).hexdigest()[:16]
    against = {"levels_ragged": "per_level", "levels_ragged_eq": "levels_uniform"}
    for form in FORMS:
        v = us[form]
        med = statistics.median(v)
        rec = {"shape": name, "form": form, "frames": B, "points_per_frame": 20000,
               "levels": [[list(s), list(b)] for s, b in PAIR], "us_per_batch": round(med, 3), "min": round(min(v), 3),
               "max": round(max(v), 3), "rounds": [round(x, 3) for x in v], "reps": reps, "inner": inner,
               "nnz": [int(o.nnz.sum().item()) for o in outs[form]], "lib_sha256": sha}
        if form in against:
            other = against[form]
            lo, hi = min(us[other]), max(us[other])
            rec["against"] = other
            rec["faster_than_its_spread"] = bool(med < lo)
            rec["inside_its_spread"] = bool(lo <= med <= hi)
            rec["median_over_its_median"] = round(med / statistics.median(us[other]), 4)
            rec["equals_it_bitwise"] = bool(same(outs[form], outs[other]))
        print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--shape", choices=("avod", "config2", "both"), default="both")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_index_levels_ragged.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    for name in ("avod", "config2") if args.shape == "both" else (args.shape,):
        run_shape(name, dev, args.repeats, args.reps, args.inner)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
