"""Times the after-VGG upconv3 (fusion_vgg_pyramid.py:53-60, :198-206) at the reference's shapes: BEV 88x100 and
image 45x150 (stride 8 of 704x800 and 1200x360), 256 + 256 -> 128 channels, 20 k points per frame, 8 frames, in
bf16 and in f32, both sides. The forms, alternated in one process after a warm-up, each call between two HIP
events on the current stream:

  fused    FusionUpconv.fused / .fused_img: shpl_upconv3x3 with the pooling in its staging (no pooled map, no
           concat); its training step runs backward="direct" (shpl_upconv3x3_dgrad / shpl_upconv3x3_wgrad);
  fused_phases  (training step only) the same module with backward="phases": the gradients through
           shpl_conv3x3_dgrad / shpl_conv3x3_wgrad with phase_weights -- the comparator of the direct backward;
  phases   (forward only) FusionUpconv.forward_phases: shpl_conv3x3 with phase_weights (4 c_out channels, 27 of 36
           taps zero), then depth_to_space;
  unfused  the pull with the concat fused in (shpl_map.pool_*), torch.nn.functional.conv_transpose2d on the
           materialised map, cropped to 2h x 2w, then the same BatchNorm call (shpl_batch_norm; inference: the same
           affine map and ReLU in torch).

for the forward (inference) and for the training step (forward + backward to both maps, the weights and beta).
One JSON line per (dtype, side, step, form): every repeat's time, their median and spread, the byte model
((rows_a c_a + rows_b c_b) e in, 4 rows_a c_out e out; the unfused route adds 2 rows_a (c_a + c_b) e for the
concat written and read) and the FLOP model (2 rows_a 9 (c_a + c_b) c_out) with their shares of 8 TB/s and of
the dense MFMA peak (bf16 2.5 PFLOP/s, f32 157 TFLOP/s), the largest difference from the fused form's output,
and the library's hash. SHPL_LIB selects a variant build.

    python scripts/time_upconv.py [--frames 8] [--reps 10] [--dtypes bf16,f32]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparse_pooling_amd import _lib as L, fusion_conv as fc, fusion_upconv as fu, pipeline, shpl_map as sm  # noqa: E402
from sparse_pooling_amd import synth  # noqa: E402

SPEC = synth.FrameSpec(20000, (1200, 360), (704, 800), (8, 8), 256, 256)
C_OUT = 128
PEAK_FLOPS = {"bf16": 2.5e15, "f32": 157.3e12}


def lib_sha256():
    with open(L.LIB_PATH, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtypes", default="bf16,f32")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_upconv.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    spec, F = SPEC, args.frames
    frames = [synth.make_frame(spec, seed=s) for s in range(F)]
    pts, vox, off, P, maxp, _ = pipeline.stack_frames(frames, dev)
    ib = sm.build_index_batch(pts, vox, off, P, spec.im_size, spec.bv_size, spec.stride, maxp)
    smap = ib.map
    for side in (fc.SIDE_BEV, fc.SIDE_IMG):  # every CSR built once, outside the timing
        smap.csr(*side.fwd)
        smap.csr(*side.grad)
    hw = {"bev": spec.bev_feat_hw, "img": spec.img_feat_hw}
    nnz = int(ib.frame_nnz.sum().item())
    sha = lib_sha256()
    for name in args.dtypes.split(","):
        dtype = {"bf16": torch.bfloat16, "f32": torch.float32}[name]
        esz = 2 if dtype == torch.bfloat16 else 4
        g = torch.Generator(device=dev).manual_seed(0)
        maps = {"bev": torch.randn((F,) + hw["bev"] + (spec.c_bev,), device=dev, generator=g).to(dtype),
                "img": torch.randn((F,) + hw["img"] + (spec.c_img,), device=dev, generator=g).to(dtype)}
        for side_name, side, other in (("bev", fc.SIDE_BEV, "img"), ("img", fc.SIDE_IMG, "bev")):
            a = maps[side_name].detach().clone().requires_grad_(True)
            b = maps[other].detach().clone().requires_grad_(True)
            ca, cb = int(a.shape[-1]), int(b.shape[-1])
            h, w = hw[side_name]
            up = fu.FusionUpconv(ca + cb, C_OUT, dtype=dtype, device=dev, seed=0, backward="direct")
            up.weights.requires_grad_(True)
            up.beta.requires_grad_(True)
            up_ph = fu.FusionUpconv(ca + cb, C_OUT, dtype=dtype, device=dev, seed=0, backward="phases")
            up_ph.weights, up_ph.beta = up.weights, up.beta  # one set of variables, two backward routes
            gy = torch.randn((F, 2 * h, 2 * w, C_OUT), device=dev, generator=g).to(dtype)
            pool, fo = smap.csr(*side.fwd), smap.frame_off

            def fused(training, m=None):
                m = up if m is None else m
                return (m.fused if side_name == "bev" else m.fused_img)(a, b, smap, is_training=training)

            def phases(training):
                return up.forward_phases(a, b, pool, fo, is_training=training)

            def unfused(training):
                x = (sm.pool_img_to_bev(smap, b, a.shape, bev=a) if side_name == "bev"
                     else sm.pool_bev_to_img(smap, b, a.shape, img=a))
                if torch.is_grad_enabled():  # the concat as a leaf of its own graph; its gradient is split below
                    x = x.detach().requires_grad_(True)
                wt = up.weights.permute(3, 2, 0, 1)
                y = torch.nn.functional.conv_transpose2d(x.permute(0, 3, 1, 2), wt, stride=2)
                raw = y[..., :2 * h, :2 * w].permute(0, 2, 3, 1).contiguous()
                if not training:
                    center, scale, shift = up._inference_epilogue()
                    return torch.relu((raw.float() - center) * scale + shift).to(dtype), x
                rf = raw.detach().float().reshape(-1, C_OUT).double()
                stats = torch.stack([rf.sum(0), (rf * rf).sum(0)])
                out = fc.batch_norm_train(raw.detach(), stats, raw.numel() // C_OUT, eps=up.eps, beta=up.beta,
                                          relu=up.relu, moving_mean=up.moving_mean.clone(),
                                          moving_var=up.moving_var.clone(), decay=up.decay,
                                          out=torch.empty_like(raw))
                return out, x, raw

            def fwd(fn):
                def step():
                    with torch.no_grad():
                        r = fn(False)
                        return r[0] if isinstance(r, tuple) else r
                return step

            def train_fused(m=None):
                for t in (a, b, up.weights, up.beta):
                    t.grad = None
                fused(True, m).backward(gy)

            def train_fused_phases():
                train_fused(up_ph)

            def train_unfused():
                # forward as above; backward: the library's BatchNorm backward, torch's autograd through the
                # transposed conv, the pooled half of the concat's gradient pulled back
                for t in (a, b, up.weights, up.beta):
                    t.grad = None
                out, x, raw = unfused(True)
                g_raw, dbeta, _ = fc.batch_norm_backward(gy, raw=raw.detach(), mean=raw.detach().float().mean((0, 1, 2)),
                                                         scale=up._scale, relu=up.relu, training=True, beta=up.beta)
                raw.backward(g_raw)
                dx_b = x.grad[..., ca:].contiguous()
                d_b = torch.empty_like(b)
                sm.pull(smap, *side.grad, dx_b, cb, 0, cb, d_b, cb)
                return d_b

            with torch.no_grad():
                ref = fused(False).float()
                diff = {"fused": 0.0, "fused_phases": 0.0,
                        "phases": float((phases(False).float() - ref).abs().max().item()),
                        "unfused": float((unfused(False)[0].float() - ref).abs().max().item())}
            rows_a, rows_b = F * h * w, b.numel() // cb
            model_bytes = (rows_a * ca + rows_b * cb) * esz + 4 * rows_a * C_OUT * esz
            model_flops = 2 * rows_a * 9 * (ca + cb) * C_OUT
            steps = (("forward", {"fused": fwd(fused), "phases": fwd(phases), "unfused": fwd(unfused)}),
                     ("train", {"fused": train_fused, "fused_phases": train_fused_phases, "unfused": train_unfused}))
            for step, forms in steps:
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
                    ms = [x0.elapsed_time(x1) for x0, x1 in ev[k]]
                    med = statistics.median(ms)
                    rec = {"step": "upconv_" + step, "side": side_name, "form": k, "dtype": name, "frames": F,
                           "input_hw": [h, w], "channels": f"{ca}+{cb}->{C_OUT}", "nnz": nnz,
                           "ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                           "ms": [round(v, 4) for v in ms], "max_abs_diff_from_fused": diff[k], "lib_sha256": sha,
                           "lib": os.environ.get("SHPL_LIB", "default")}
                    if step == "forward":
                        extra = 2 * rows_a * (ca + cb) * esz if k == "unfused" else 0
                        rec["model_bytes"] = model_bytes + extra
                        rec["model_flops"] = model_flops
                        rec["fraction_of_8TBps"] = round((model_bytes + extra) / 8e12 * 1e3 / med, 4)
                        rec["fraction_of_mfma_peak"] = round(model_flops / PEAK_FLOPS[name] * 1e3 / med, 4)
                    print(json.dumps(rec), flush=True)
            del a, b, up, up_ph, gy
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
