"""Times the image-side post-fusion step (pyramid_fusion_pooled_img over a dual SHPL) at config-2 geometry: 64
frames, image 360x1200, 32 + 32 -> 32 channels, BatchNorm inference + ReLU, in bf16 and in f32. Two forms,
alternated in one process after a warm-up, each call between two HIP events on the current stream:

  fused    FusionConv.fused_img_csr over the pixel-keyed CSR (img_fused never written);
  unfused  shpl_map.pool_bev_to_img(..., img=img), then the conv of the map.

One JSON line per (dtype, form): every repeat's time, their median and spread, whether the two forms' outputs
are bitwise equal, and the library's hash. SHPL_LIB selects a variant build.

    python scripts/time_conv_img.py [--frames 64] [--reps 10] [--dtypes bf16,f32]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparse_pooling_amd import _lib as L, fusion_conv as fc, pipeline, shpl_map as sm, synth  # noqa: E402


def lib_sha256():
    with open(L.LIB_PATH, "rb") as fh:
        return hashlib.sha256(fh.read()).hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtypes", default="bf16,f32")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_conv_img.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    spec = synth.CONFIGS[2]
    F = args.frames
    frames = [synth.make_frame(spec, seed=s, n_outside=200) for s in range(F)]
    pts, vox, off, P, maxp, N = pipeline.stack_frames(frames, dev)
    ib = sm.build_index_batch(pts, vox, off, P, spec.im_size, spec.bv_size, spec.stride, maxp)
    smap = ib.map
    csr = smap.csr(L.BY_PIXEL, L.ORDER_COL_ROW)
    Hb, Wb = spec.bev_feat_hw
    Hi, Wi = spec.img_feat_hw
    cb, ci = spec.c_bev, spec.c_img
    sha = lib_sha256()
    for name in args.dtypes.split(","):
        dtype = {"bf16": torch.bfloat16, "f32": torch.float32}[name]
        g = torch.Generator(device=dev).manual_seed(0)
        bev = torch.randn((F, Hb, Wb, cb), device=dev, generator=g).to(dtype)
        img = torch.randn((F, Hi, Wi, ci), device=dev, generator=g).to(dtype)
        conv = fc.FusionConv(ci + cb, cb, dtype=dtype, device=dev, seed=0)
        out = {k: torch.empty((F, Hi, Wi, cb), dtype=dtype, device=dev) for k in ("fused", "unfused")}

        def fused():
            conv.fused_img_csr(img, bev, csr, smap.frame_off, out=out["fused"])

        def unfused():
            conv(sm.pool_bev_to_img(smap, bev, img.shape, img=img), out=out["unfused"])

        forms = {"fused": fused, "unfused": unfused}
        for _ in range(args.warmup):
            for fn in forms.values():
                fn()
        torch.cuda.synchronize()
        ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                  for _ in range(args.reps)] for k in forms}
        for r in range(args.reps):  # alternated: both forms see the same machine state
            for k, fn in forms.items():
                ev[k][r][0].record()
                fn()
                ev[k][r][1].record()
        torch.cuda.synchronize()
        same = bool(torch.equal(out["fused"], out["unfused"]))
        esz = 2 if dtype == torch.bfloat16 else 4
        for k in forms:
            ms = [a.elapsed_time(b) for a, b in ev[k]]
            print(json.dumps({
                "step": "conv_img", "form": k, "dtype": name, "frames": F, "image": [Hi, Wi], "bev": [Hb, Wb],
                "channels": f"{ci}+{cb}->{cb}", "nnz": int(ib.frame_nnz.sum().item()),
                "ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4),
                "ms_max": round(max(ms), 4), "ms": [round(v, 4) for v in ms],
                "img_fused_bytes_written_and_read": 0 if k == "fused" else 2 * F * Hi * Wi * (ci + cb) * esz,
                "bitwise_equal": same, "lib_sha256": sha, "lib": os.environ.get("SHPL_LIB", "default")}), flush=True)
        del bev, img, out, conv
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
