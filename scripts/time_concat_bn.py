"""Times the SHPL concat with BatchNorm on both halves (fusion_bn.FusionConcatBN) at config 2's shape -- 64
frames, BEV 704x800x32, image 360x1200x32, 20 k points per frame, f32 and bf16 -- and at config 3's -- 4 frames,
stride 8, 256 + 256 channels, bf16. Forms, alternated in one process after a warm-up, each call between two HIP
events on the current stream:

  fused   FusionConcatBN.fused / fused_img: statistics over the occupied rows, apply and concat in one row-keyed
          launch, no pooled map;
  chain   what the library could run before: shpl_map.layer (the plain concat), then
          torch.nn.functional.batch_norm over the concatenated map, and its autograd backward;
  concat  (inference forward only) shpl_map.layer alone: what the normalisation costs beside the plain concat.

Steps: the inference forward, the training forward, the training step (forward + backward to bev, img and beta).
One JSON line per (config, dtype, side, step, form): every repeat's time, their median and spread, the byte model
in passes of R c e bytes (R rows, c the channels of one half, e the element size: training forward 4 fused / 9
chain, inference forward 3 fused and concat / 7 chain) with its time at 8 TB/s and the measured share of that
floor, and the library's hash.

    python scripts/time_concat_bn.py [--configs 2,3] [--reps 10] [--dtypes f32,bf16] [--sides bv,img]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparse_pooling_amd import _lib as L, fusion_bn as fb, pipeline, shpl_map as sm, synth  # noqa: E402

CONFIGS = {2: (synth.CONFIG2, 64, ("f32", "bf16")), 3: (synth.CONFIG3, 4, ("bf16",))}
EPS, DECAY = 1e-3, 0.999
PASSES = {("inference_forward", "fused"): 3, ("inference_forward", "chain"): 7, ("inference_forward", "concat"): 3,
          ("training_forward", "fused"): 4, ("training_forward", "chain"): 9}


def lib_sha256():
    with open(L.LIB_PATH, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="2,3")
    ap.add_argument("--frames", type=int, default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dtypes", default="f32,bf16")
    ap.add_argument("--sides", default="bv,img")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_concat_bn.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    sha = lib_sha256()
    for cfg in (int(c) for c in args.configs.split(",")):
        spec, F, dtypes = CONFIGS[cfg]
        F = args.frames or F
        frames = [synth.make_frame(spec, seed=s) for s in range(F)]
        pts, vox, off, P, maxp, _ = pipeline.stack_frames(frames, dev)
        smap = sm.build_index_batch(pts, vox, off, P, spec.im_size, spec.bv_size, spec.stride, maxp).map
        Hb, Wb = spec.bev_feat_hw
        Hi, Wi = spec.img_feat_hw
        cb, ci = spec.c_bev, spec.c_img
        for name in (d for d in args.dtypes.split(",") if d in dtypes):
            dtype = {"bf16": torch.bfloat16, "f32": torch.float32}[name]
            esz = 2 if dtype == torch.bfloat16 else 4
            gen = torch.Generator(device=dev).manual_seed(0)
            bev = torch.randn((F, Hb, Wb, cb), device=dev, generator=gen).to(dtype).requires_grad_(True)
            img = torch.randn((F, Hi, Wi, ci), device=dev, generator=gen).to(dtype).requires_grad_(True)
            for side in args.sides.split(","):
                mod = fb.FusionConcatBN(cb, ci, eps=EPS, decay=DECAY, dtype=dtype, device=dev)
                beta = mod.params[side]["beta"]
                c = cb + ci
                rows = F * (Hb * Wb if side == "bv" else Hi * Wi)
                rm, rv = torch.zeros(c, device=dev), torch.ones(c, device=dev)
                beta_c = torch.zeros(c, device=dev, requires_grad=True)
                ones_c = torch.ones(c, device=dev)
                gy = torch.randn((F, Hb, Wb, c) if side == "bv" else (F, Hi, Wi, c), device=dev, generator=gen).to(dtype)

                def fused(training):
                    return mod.fused(bev, img, smap, training) if side == "bv" else mod.fused_img(img, bev, smap, training)

                def concat():
                    return sm.layer(bev, img, smap, dual=True)[0 if side == "bv" else 1]

                def chain(training):
                    x = concat().permute(0, 3, 1, 2)  # NHWC memory, channels as dim 1
                    # scale=False as a constant weight of ones (the backward of a batch_norm without a weight fails)
                    y = torch.nn.functional.batch_norm(x, rm, rv, ones_c, beta_c, training, 1.0 - DECAY, EPS)
                    return y.permute(0, 2, 3, 1)

                def no_grad(fn, *a):
                    def step():
                        with torch.no_grad():
                            return fn(*a)
                    return step

                def train(fn, b):
                    def step():
                        for t in (bev, img, b):
                            t.grad = None
                        fn(True).backward(gy)
                    return step

                steps = {"inference_forward": {"fused": no_grad(fused, False), "chain": no_grad(chain, False),
                                               "concat": no_grad(concat)},
                         "training_forward": {"fused": no_grad(fused, True), "chain": no_grad(chain, True)},
                         "training_step": {"fused": train(fused, beta), "chain": train(chain, beta_c)}}
                with torch.no_grad():
                    diff = float((fused(True).float() - chain(True).float()).abs().max().item())
                for step, forms in steps.items():
                    for _ in range(args.warmup):
                        for fn in forms.values():
                            fn()
                    torch.cuda.synchronize()
                    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                              for _ in range(args.reps)] for k in forms}
                    for r in range(args.reps):  # alternated: every form sees the same machine state
                        for k, fn in forms.items():
                            ev[k][r][0].record()
                            fn()
                            ev[k][r][1].record()
                    torch.cuda.synchronize()
                    for k in forms:
                        ms = [a.elapsed_time(b) for a, b in ev[k]]
                        med = statistics.median(ms)
                        rec = {"step": "concat_bn_" + step, "form": k, "config": cfg, "dtype": name, "side": side,
                               "frames": F, "rows": rows, "channels": f"{cb}+{ci}", "nnz_cap": smap.nnz_cap,
                               "ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                               "ms_spread": round(max(ms) - min(ms), 4), "ms": [round(v, 4) for v in ms],
                               "max_abs_diff_fused_vs_chain_training": diff, "lib_sha256": sha,
                               "lib": os.environ.get("SHPL_LIB", "default")}
                        if (step, k) in PASSES:
                            model = PASSES[(step, k)] * rows * (c // 2) * esz  # passes in units of R * 32 * e per half
                            rec["model_passes_RCe_per_half"] = PASSES[(step, k)]
                            rec["model_bytes"] = model
                            rec["model_ms_at_8TBps"] = round(model / 8e12 * 1e3, 4)
                            rec["fraction_of_8TBps_floor"] = round(model / 8e12 * 1e3 / med, 4)
                        print(json.dumps(rec), flush=True)
                del mod, gy
                torch.cuda.empty_cache()
            del bev, img
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
