"""Kept zeros at config 2's shape (64 frames, BEV 704x800, 32 + 32 channels, f32): what a step costs when bv_fused's
pooled half is kept zero between steps instead of being streamed as zeros (FusedPipeline.KEEP_ZEROS).

(i) Half-row copy calibration: scripts/calib_halfrow.py's forms at 128-byte halves (C = 32 f32, R = 64*704*800
    rows), shpl_pull_dense each, HIP events around --reps launches, every form twice:
      half   the pass-through copy into the first half of 256-byte output rows (the kept-zeros step's copy)
      cont   the same bytes into contiguous 128-byte rows
      full   the concat's whole rows (pass-through + pooled zeros: today's k_dense)
      zhalf  the pooled zeros alone into the second halves
(ii) The bench's graph-replayed step_overlapped in three forms over one pipeline in one process, each captured
    after --warmup eager steps and timed with HIP events around --reps replays, the forms alternated --rounds times:
      full    KEEP_ZEROS False: k_dense over every row, then k_sparse
      beside  kept zeros, the sparse pass beside the side stream's copy
      serial  kept zeros, the sparse pass after the copy (KEEP_ZEROS_SERIAL)
    One JSON line per form (every round's ms_per_step, their median) and torch.equal of each kept-zeros form's
    bv_fused with the full form's. SHPL_LIB selects a variant build.

    python scripts/time_keep_zeros.py [--frames 64] [--reps 20] [--rounds 3] [--part calib|step|both]
"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparse_pooling_amd import _lib as L, dist as sd, pipeline, synth  # noqa: E402


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


def calib(dev, frames, reps):
    spec = synth.CONFIG2
    Hb, Wb = spec.bev_feat_hw
    R, C = frames * Hb * Wb, spec.c_bev
    bev = torch.randn(R, C, device=dev)
    out = torch.empty(R, 2 * C, device=dev)
    cont = torch.empty(R, C, device=dev)
    lib = L.lib()

    def dense(c_pool, pass_, out_ptr, out_stride, c_pass):
        c = L.ShplCsr()
        c.n_keys = R
        L.check(lib.shpl_pull_dense(L.BY_CELL, L.F32, ctypes.byref(c), L.ptr(bev), C, 0, c_pool,
                                    L.ptr(pass_) if pass_ is not None else None, C, 0, c_pass,
                                    L.OUT_CONCAT if c_pass else L.OUT_POOL, ctypes.c_void_p(out_ptr), out_stride,
                                    L.stream_of(dev)), "shpl_pull_dense")

    forms = {
        "half": (lambda: dense(0, bev, out.data_ptr(), 2 * C, C), 2 * R * C * 4),
        "cont": (lambda: dense(0, bev, cont.data_ptr(), C, C), 2 * R * C * 4),
        "full": (lambda: dense(C, bev, out.data_ptr(), 2 * C, C), 3 * R * C * 4),
        "zhalf": (lambda: dense(C, None, out.data_ptr() + C * 4, 2 * C, 0), R * C * 4),
    }
    for name, (fn, nbytes) in list(forms.items()) * 2:
        ms = timed(fn, reps)
        print(json.dumps({"calib": name, "rows": R, "half_bytes": C * 4, "ms": round(ms, 4),
                          "GB": round(nbytes / 1e9, 3), "GBps": round(nbytes / ms / 1e6, 1)}), flush=True)


def steps(dev, frames, reps, rounds, warmup):
    spec = synth.CONFIG2
    fids = list(range(frames))
    frs = [synth.make_frame(spec, seed=s, n_outside=200) for s in fids]
    pts, vox, off, P, maxp, N = pipeline.stack_frames(frs, dev)
    pl = pipeline.FusedPipeline(frames, maxp, N, spec.im_size, spec.bv_size, spec.stride, spec.c_bev, spec.c_img,
                                dtype=torch.float32, device=dev)
    Hb, Wb = spec.bev_feat_hw
    Hi, Wi = spec.img_feat_hw
    bev = sd.fill_features(torch.empty((frames, Hb, Wb, spec.c_bev), device=dev), fids, 1)
    img = sd.fill_features(torch.empty((frames, Hi, Wi, spec.c_img), device=dev), fids, 2)
    side = torch.cuda.Stream(device=dev)
    forms = {"full": (False, False), "beside": (True, False), "serial": (True, True)}
    graphs = {}
    for name, (keep, serial) in forms.items():
        pipeline.FusedPipeline.KEEP_ZEROS, pipeline.FusedPipeline.KEEP_ZEROS_SERIAL = keep, serial
        pl.invalidate()
        for _ in range(warmup):
            pl.step_overlapped(pts, vox, off, P, bev, img, side)
        torch.cuda.synchronize()
        assert pl._pooled_clean == keep
        gs = torch.cuda.Stream(device=dev)
        gs.wait_stream(torch.cuda.current_stream(dev))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=gs):
            pl.step_overlapped(pts, vox, off, P, bev, img, side)
        g.replay()
        torch.cuda.synchronize()
        graphs[name] = g
    pl.check()
    ms = {name: [] for name in forms}
    for _ in range(rounds):  # alternated: every form sees the same machine state
        for name, g in graphs.items():
            ms[name].append(timed(g.replay, reps))
    graphs["full"].replay()
    torch.cuda.synchronize()
    want = pl.bv_fused.clone()
    sha = hashlib.sha256(open(L.LIB_PATH, "rb").read()).hexdigest()[:16]
    for name, g in graphs.items():
        g.replay()
        g.replay()
        torch.cuda.synchronize()
        print(json.dumps({"step": "config2_step_overlapped_graph", "form": name, "frames": frames,
                          "ms_per_step": round(statistics.median(ms[name]), 4),
                          "rounds": [round(v, 4) for v in ms[name]], "reps": reps,
                          "equals_full": bool(torch.equal(pl.bv_fused, want)), "lib_sha256": sha}), flush=True)
    pl.check()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--part", choices=("calib", "step", "both"), default="both")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_keep_zeros.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.part in ("calib", "both"):
        calib(dev, args.frames, args.reps)
        torch.cuda.empty_cache()
    if args.part in ("step", "both"):
        steps(dev, args.frames, args.reps, args.rounds, args.warmup)


if __name__ == "__main__":
    main()
