"""Host cost of issuing 200 eager step_overlapped calls at config 3 (bf16, dual, 4 frames, bucketed):
time.perf_counter around the loop, one synchronise after it. bench.py's timed loops replay captured graphs, which
hold the launches and not the Python that issued them; this is what a change of pipeline.py's Python costs a caller
who issues the step eagerly. One JSON line. SHPL_LIB selects a variant build.

    python scripts/time_step_issue.py [TREE]     TREE: the checkout whose package is imported (default: this one)
"""
import json
import os
import sys
import time

root = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, root)
import torch  # noqa: E402
from sparse_pooling_amd import pipeline, synth, _lib as L  # noqa: E402

assert os.path.dirname(os.path.dirname(os.path.abspath(pipeline.__file__))) == root
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
spec = synth.CONFIGS[3]
F = 4
frames = [synth.make_frame(spec, seed=s, n_outside=200) for s in range(F)]
pts, vox, off, P, maxp, N = pipeline.stack_frames(frames, dev)
pl = pipeline.FusedPipeline(F, maxp, N, spec.im_size, spec.bv_size, spec.stride, spec.c_bev, spec.c_img,
                            dtype=torch.bfloat16, dual=True, device=dev)
Hb, Wb = spec.bev_feat_hw
Hi, Wi = spec.img_feat_hw
bev = torch.randn((F, Hb, Wb, spec.c_bev), device=dev).to(torch.bfloat16)
img = torch.randn((F, Hi, Wi, spec.c_img), device=dev).to(torch.bfloat16)
side, side2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
for _ in range(20):
    pl.step_overlapped(pts, vox, off, P, bev, img, side, side2=side2)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(200):
    pl.step_overlapped(pts, vox, off, P, bev, img, side, side2=side2)
t1 = time.perf_counter()
torch.cuda.synchronize()
t2 = time.perf_counter()
pl.check()
print(json.dumps({"host_cost": "200 eager step_overlapped, config 3", "tree": sys.argv[1] if len(sys.argv) > 1 else ".",
                  "buckets": pl.buckets, "issue_us_per_step": round(1e6 * (t1 - t0) / 200, 2),
                  "with_sync_us_per_step": round(1e6 * (t2 - t0) / 200, 2), "lib": os.path.basename(L.LIB_PATH)}),
      flush=True)
