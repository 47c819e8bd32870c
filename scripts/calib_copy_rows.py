"""Calibration of a pass-only row copy at config 2's shape (not part of the library): 64 x 704 x 800 rows of
128 B (32 f32), copied
  half  -- into the first half of 256-byte output rows (the kept-zeros step's copy)
  cont  -- into contiguous 128-byte rows (the same bytes, no gaps)
by shpl_pull_dense (the library's form), by scripts/calib.hip's k_copy (cont only) and by every k_copy_rows form
of calib.hip: U = 1, 2, 4, 8 chunks per thread over adjacent blocks, 256 or 512 threads, non-temporal or plain
loads and stores; then the U = 1 non-temporal form under other launch shapes (k_copy_rows_shape: 64 to 1024
threads, 2 to 6 waves per SIMD at most, workgroups ordered so that each XCD walks contiguous rows). All forms run in one process, every form twice (the whole list, then the whole list again),
HIP events around --reps launches; each form's first output is compared bit for bit with the source. One JSON
line per run.

    python scripts/calib_copy_rows.py --build     # hipcc: libcalib.so (+ libcalib_preload.so, kernarg preloading)
    python scripts/calib_copy_rows.py [--frames 64 | --rows R] [--reps 20] [--chunks 8] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VDIR = os.path.join(ROOT, "sparse_pooling_amd", "variants")
LIBS = {"": [], "_preload": ["-mllvm", "-amdgpu-kernarg-preload-count=8"]}


def build():
    from sparse_pooling_amd import build as b
    os.makedirs(VDIR, exist_ok=True)
    for tag, extra in LIBS.items():
        out = os.path.join(VDIR, f"libcalib{tag}.so")
        subprocess.run([b.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", *extra,
                        os.path.join(ROOT, "scripts", "calib.hip"), "-o", out], check=True)
        print("built", out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", action="store_true")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--chunks", type=int, default=8, help="16-byte chunks per source row (a power of two)")
    ap.add_argument("--rows", type=int, default=0, help="rows instead of config 2's frames x 704 x 800")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    if args.build:
        return build()
    import torch
    from sparse_pooling_amd import _lib as L, synth
    if not torch.cuda.is_available():
        sys.exit("calib_copy_rows.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    Hb, Wb = synth.CONFIG2.bev_feat_hw
    R, cpr = args.rows or args.frames * Hb * Wb, args.chunks
    C, shift = 4 * cpr, cpr.bit_length() - 1
    assert 1 << shift == cpr and R * cpr < 1 << 31
    bev = torch.randn(R, C, device=dev)
    outs = {"half": torch.empty(R, 2 * C, device=dev), "cont": torch.empty(R, C, device=dev)}
    ocpr = {"half": 2 * cpr, "cont": cpr}
    st = L.stream_of(dev)
    lib = L.lib()
    cals = {tag: ctypes.CDLL(os.path.join(VDIR, f"libcalib{tag}.so")) for tag in LIBS
            if os.path.exists(os.path.join(VDIR, f"libcalib{tag}.so"))}

    def dense(layout):
        c = L.ShplCsr()
        c.n_keys = R
        L.check(lib.shpl_pull_dense(L.BY_CELL, L.F32, ctypes.byref(c), L.ptr(bev), C, 0, 0, L.ptr(bev), C, 0, C,
                                    L.OUT_CONCAT, L.ptr(outs[layout]), ocpr[layout] * 4, st), "shpl_pull_dense")

    def rows(cal, layout, U, B, policy):
        rc = cal.calib_copy_rows(L.ptr(bev), L.ptr(outs[layout]), ctypes.c_uint32(R * cpr), ctypes.c_uint32(shift),
                                 ctypes.c_uint32(ocpr[layout]), U, B, policy, st)
        assert rc == 0, rc

    def shape(cal, layout, B, W, xcd):
        rc = cal.calib_copy_rows_shape(L.ptr(bev), L.ptr(outs[layout]), ctypes.c_uint32(R * cpr),
                                       ctypes.c_uint32(shift), ctypes.c_uint32(ocpr[layout]), B, W, xcd, st)
        assert rc == 0, rc

    def plain(cal):
        rc = cal.calib_copy(L.ptr(bev), L.ptr(outs["cont"]), ctypes.c_uint64(R * cpr), 1, 1, 0, st)
        assert rc == 0, rc

    forms = []  # (record, layout, fn)
    for layout in ("half", "cont"):
        forms.append(({"form": "shpl_pull_dense"}, layout, lambda layout=layout: dense(layout)))
    forms.append(({"form": "k_copy", "U": 1, "block": 256, "nt_load": True, "nt_store": True}, "cont",
                  lambda: plain(cals[""])))
    for tag, cal in cals.items():
        for layout in ("half", "cont"):
            for B in (256, 512):
                for policy in (3, 0, 1, 2):
                    for U in (1, 2, 4, 8):
                        rec = {"form": "k_copy_rows" + tag, "U": U, "block": B, "nt_load": bool(policy & 1),
                               "nt_store": bool(policy & 2)}
                        forms.append((rec, layout, lambda c=cal, l=layout, U=U, B=B, p=policy: rows(c, l, U, B, p)))
    # launch shapes of the U = 1 non-temporal form: (threads, waves per SIMD at most, XCD-contiguous block order)
    shapes = [(64, 8, 0), (128, 8, 0), (256, 8, 0), (1024, 8, 0), (256, 2, 0), (256, 3, 0), (256, 4, 0), (256, 5, 0),
              (256, 6, 0), (256, 7, 0), (256, 8, 1), (256, 4, 1), (128, 8, 1), (256, 5, 1), (256, 6, 1), (256, 7, 1),
              (128, 6, 1), (512, 8, 1), (64, 8, 1)]
    for layout in ("half", "cont"):
        for B, W, xcd in shapes:
            rec = {"form": "k_copy_rows_shape", "U": 1, "block": B, "nt_load": True, "nt_store": True,
                   "waves_per_simd": W, "xcd_contiguous": bool(xcd)}
            forms.append((rec, layout, lambda l=layout, B=B, W=W, x=xcd: shape(cals[""], l, B, W, x)))
    nbytes = 2 * R * C * 4
    sink = open(args.out, "a") if args.out else None
    for rnd in range(2):
        for rec, layout, fn in forms:
            if rnd == 0:
                outs[layout].fill_(float("nan"))
            fn()
            torch.cuda.synchronize()
            ok = None
            if rnd == 0:
                ok = bool(torch.equal(outs[layout][:, :C].view(torch.int32), bev.view(torch.int32)))
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            ms = a.elapsed_time(b) / args.reps
            line = json.dumps({"calib": "copy_rows", **rec, "layout": layout, "rows": R, "row_bytes": C * 4,
                               "run": rnd, "ms": round(ms, 4), "GBps": round(nbytes / ms / 1e6, 1), "equal": ok})
            print(line, flush=True)
            if sink:
                sink.write(line + "\n")
                sink.flush()


if __name__ == "__main__":
    main()
