"""Times MV3D's fused RPN heads (MV3D_voxel_train.py:144-178) at the network's shape: BEV 100x120, image 48x160,
768 + 768 -> 4 + 14 channels, 20 k points per frame at stride [8, 2], 8 frames, in bf16 and in f32. Three forms,
alternated in one process after a warm-up, each call between two HIP events on the current stream:

  fused          FusionHead.fused: the heads applied before the pooling (no pooled map, no concat);
  unfused        the op behind mv3d.sparse_pool over the same prebuilt map (shpl_map.pool_op: mv3d.sparse_pool itself
                 is batch-1 and packs M on every call), torch.cat, then FusionHead.__call__;
  unfused_torch  the same pooling and concat, then the 1x1 convs as one torch matmul + bias: no kernel of
                 FusionHead at all.

and the same three for the training step (forward + backward to lidar, img, every weight and bias). One JSON
line per (dtype, step, form): every repeat's time, their median and spread, the fused byte model
((R c_lidar + P c_img) e + R c_out e + P c_out 4 + nnz 12) with its share of an 8 TB/s floor, the largest
difference from the fused form's output, and the library's hash. SHPL_LIB selects a variant build.

With --keep-prob P (absent: the three forms above and nothing else) the heads under dropout over the concat, as
MV3D trains them, are timed instead, again alternated in one process:

  fused_dropout          FusionHead.fused_dropout: pooling, mask and heads in one GEMM (no pooled map, concat or mask);
  unfused_dropout        shpl_map.pool_op, torch.cat, then FusionHead.dropout over the materialised map;
  unfused_torch_dropout  the same pooling and concat, torch.nn.functional.dropout, one matmul + bias: nothing of
                         the dropout kernels at all (the form the code before them could run);
  fused                  FusionHead.fused at keep 1: what the staging and the generator cost beside it.

The byte model of fused_dropout's forward is (R c_lidar + nnz c_img) e + R c_out e + nnz 12: the image rows are
gathered per entry, not streamed once per pixel. The largest difference is taken from fused_dropout's output
for the two forms that share its mask.

    python scripts/time_mv3d_head.py [--frames 8] [--reps 10] [--dtypes bf16,f32] [--keep-prob 0.5]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparse_pooling_amd import _lib as L, fusion_head as fh, pipeline, shpl_map as sm, synth  # noqa: E402

SPEC = synth.FrameSpec(20000, (1280, 384), (200, 240), (8, 2), 768, 768)  # MV3D: image 1280x384, BEV 200x240
HEADS = (4, 14)


def lib_sha256():
    with open(L.LIB_PATH, "rb") as fh_:
        return hashlib.sha256(fh_.read()).hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtypes", default="bf16,f32")
    ap.add_argument("--keep-prob", type=float, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_mv3d_head.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    spec, F = SPEC, args.frames
    frames = [synth.make_frame(spec, seed=s) for s in range(F)]
    pts, vox, off, P, maxp, _ = pipeline.stack_frames(frames, dev)
    ib = sm.build_index_batch(pts, vox, off, P, spec.im_size, spec.bv_size, spec.stride, maxp)
    smap = ib.map
    for key in ((L.BY_CELL, L.ORDER_ENTRY), (L.BY_PIXEL, L.ORDER_COL_ENTRY)):  # built once, outside the timing
        smap.csr(*key)
    Hb, Wb = spec.bev_feat_hw
    Hi, Wi = spec.img_feat_hw
    cl, ci, co = spec.c_bev, spec.c_img, sum(HEADS)
    R, Pn, nnz = F * Hb * Wb, F * Hi * Wi, int(ib.frame_nnz.sum().item())
    sha = lib_sha256()
    for name in args.dtypes.split(","):
        dtype = {"bf16": torch.bfloat16, "f32": torch.float32}[name]
        esz = 2 if dtype == torch.bfloat16 else 4
        g = torch.Generator(device=dev).manual_seed(0)
        lidar = torch.randn((F, Hb, Wb, cl), device=dev, generator=g).to(dtype).requires_grad_(True)
        img = torch.randn((F, Hi, Wi, ci), device=dev, generator=g).to(dtype).requires_grad_(True)
        head = fh.FusionHead(cl, ci, heads=HEADS, dtype=dtype, device=dev, seed=0)
        params = [*head.weights, *head.biases]
        for p in params:
            p.requires_grad_(True)
        gy = [torch.randn((F, Hb, Wb, n), device=dev, generator=g).to(dtype) for n in HEADS]

        def fused():
            return head.fused(lidar, img, smap)

        def concat():
            return torch.cat([lidar, sm.pool_op(img, smap, (F, Hb, Wb))], dim=-1)

        def unfused():
            return head(concat())

        def unfused_torch():
            x = concat()
            return tuple(torch.matmul(x, w.reshape(cl + ci, n)) + b.to(dtype)
                         for w, b, n in zip(head.weights, head.biases, HEADS))

        def train(fn):
            def step():
                for t in (lidar, img, *params):
                    t.grad = None
                torch.autograd.backward(fn(), gy)
            return step

        def inference(fn):
            def step():
                with torch.no_grad():
                    return fn()
            return step

        kp, seed = args.keep_prob, 20261

        def fused_dropout():
            return head.fused_dropout(lidar, img, smap, kp, seed=seed)

        def unfused_dropout():
            return head.dropout(concat(), kp, seed=seed)

        def unfused_torch_dropout():
            x = torch.nn.functional.dropout(concat(), p=1.0 - kp, training=True)
            return tuple(torch.matmul(x, w.reshape(cl + ci, n)) + b.to(dtype)
                         for w, b, n in zip(head.weights, head.biases, HEADS))

        if kp is None:
            base = {"fused": fused, "unfused": unfused, "unfused_torch": unfused_torch}
            first, same_mask = "fused", set(base)
            model = (R * cl + Pn * ci) * esz + R * co * esz + Pn * co * 4 + nnz * 12
        else:
            base = {"fused_dropout": fused_dropout, "unfused_dropout": unfused_dropout,
                    "unfused_torch_dropout": unfused_torch_dropout, "fused": fused}
            first, same_mask = "fused_dropout", {"fused_dropout", "unfused_dropout"}
            model = (R * cl + nnz * ci) * esz + R * co * esz + nnz * 12
        with torch.no_grad():
            ref = torch.cat(base[first](), -1).float()
            diff = {k: float((torch.cat(fn(), -1).float() - ref).abs().max().item()) if k in same_mask else None
                    for k, fn in base.items()}
        for step, wrap in (("forward", inference), ("train", train)):
            forms = {k: wrap(fn) for k, fn in base.items()}
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
                rec = {"step": "mv3d_head_" + step, "form": k, "dtype": name, "frames": F, "bev": [Hb, Wb],
                       "image": [Hi, Wi], "channels": f"{cl}+{ci}->{'+'.join(str(n) for n in HEADS)}", "nnz": nnz,
                       "ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                       "ms": [round(v, 4) for v in ms], "max_abs_diff_from_" + first: diff[k], "lib_sha256": sha,
                       "lib": os.environ.get("SHPL_LIB", "default")}
                if kp is not None:
                    rec["keep_prob"] = kp
                if step == "forward":
                    rec[first + "_model_bytes"] = model
                    rec[first + "_model_ms_at_8TBps"] = round(model / 8e12 * 1e3, 4)
                    if k == first:
                        rec["fraction_of_8TBps_floor"] = round(model / 8e12 * 1e3 / med, 4)
                print(json.dumps(rec), flush=True)
        del lidar, img, head, params, gy
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
