"""Record tests/golden/conv_host_plan.json: what the conv / BatchNorm host code of libshpl.so answers
without a GPU -- workspace sizes, the row-streaming and the wide kernel's predicate, and the status of calls it rejects before
its first HIP call. tests/test_conv_host_plan.py replays every row against the built library.

Each row is {"fn", "args", "status", "out"}. args are the C arguments in order, with
  "P" / "Q"       a fake non-null device pointer, 16-byte aligned (256) / not (264); never dereferenced
  null            NULL
  {"csr": [...]}  a shpl_csr by reference: ent_dst, ent_src, ent_val ("P" / null), n_keys, nnz_cap
  "OUT"           the size_t / int the call writes; "out" holds its value (null unless status is 0)

Run (after building the library):  python tests/golden/make_conv_host_plan.py
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
TABLE = os.path.join(HERE, "conv_host_plan.json")

F32, BF16 = 0, 1
INT_OUT = {"shpl_conv3x3_rows_form", "shpl_conv3x3_wide_form"}  # write an int; the other "OUT" calls a size_t


def replay(lib, L, fn, args):
    """(status, out) of one recorded call."""
    out = ctypes.c_int(-1) if fn in INT_OUT else ctypes.c_size_t(0)
    keep, c = [], []
    for a in args:
        if a == "P" or a == "Q":
            c.append(ctypes.c_void_p(256 if a == "P" else 264))
        elif a == "OUT":
            c.append(ctypes.byref(out))
        elif isinstance(a, dict):
            dst, src, val, n_keys, cap = a["csr"]
            p = lambda t: 256 if t == "P" else None  # noqa: E731
            keep.append(L.ShplCsr(p(dst), p(src), p(val), None, n_keys, cap))
            c.append(ctypes.byref(keep[-1]))
        else:
            c.append(a)
    rc = getattr(lib, fn)(*c)
    return rc, (out.value if "OUT" in args and rc == 0 else None)


def csr(n_keys, cap=1000, ent="P"):
    return {"csr": [ent, ent, ent, n_keys, cap]}


SHAPES = [  # h, w, c_a, c_b, c_out (2 frames)
    (176, 200, 32, 32, 32),
    (9, 33, 8, 8, 32),
    (61, 40, 32, 16, 64),
    (121, 40, 32, 32, 32),     # three bands
    (16, 32, 64, 64, 256),     # wide, compact pooled runs
    (700, 900, 64, 64, 256),   # wide, past OCC_MAX_WORDS: the map materialised
    (18433, 3, 64, 64, 256),   # the same at the smallest map that gets there
    (18433, 3, 32, 32, 32),    # the row form declined at that limit
    (61, 40, 32, 0, 64),       # c_b = 0
    (9, 33, 0, 16, 32),        # c_a = 0
]
NF = 2


def workspace_calls():
    for h, w, ca, cb, co in SHAPES:
        for dt in (F32, BF16):
            for cap in (-1, 0, 1000):
                for stats in (0, 1):
                    yield "shpl_conv3x3_workspace_bytes", [dt, NF, h, w, ca, cb, co, cap, stats, "OUT"]
                if cap != 0:
                    yield "shpl_conv3x3_wgrad_workspace_bytes", [dt, NF, h, w, ca, cb, co, cap, "OUT"]
        yield "shpl_batch_norm_backward_workspace_bytes", [NF * h * w, co, "OUT"]
    # the plans' own rejections
    yield "shpl_conv3x3_workspace_bytes", [7, NF, 16, 32, 32, 32, 32, -1, 0, "OUT"]
    yield "shpl_conv3x3_workspace_bytes", [BF16, NF, 16, 32, 0, 0, 32, -1, 0, "OUT"]
    yield "shpl_conv3x3_workspace_bytes", [BF16, NF, (1 << 20) + 1, 32, 32, 32, 32, -1, 0, "OUT"]
    yield "shpl_conv3x3_workspace_bytes", [BF16, NF, 16, 32, 32, 32, 32, 1 << 31, 0, "OUT"]
    yield "shpl_conv3x3_workspace_bytes", [BF16, NF, 16, 32, 32, 32, 32, -1, 0, None]
    yield "shpl_conv3x3_wgrad_workspace_bytes", [7, NF, 16, 32, 32, 32, 32, -1, "OUT"]
    yield "shpl_conv3x3_wgrad_workspace_bytes", [BF16, NF, 16, 32, 32, 32, 0, -1, "OUT"]
    yield "shpl_batch_norm_backward_workspace_bytes", [-1, 32, "OUT"]
    yield "shpl_batch_norm_backward_workspace_bytes", [100, 0, "OUT"]


def rows_form(dt, nf, h, w, ca, cb, co, pool=None, stats=0, act=0, a="P", a_stride=None, a_off=0, b="P",
              b_stride=None, b_off=0, out="P", out_stride=None, frame_off="P", weights="P"):
    return "shpl_conv3x3_rows_form", [
        dt, nf, h, w, a, ca + a_off if a_stride is None else a_stride, a_off, ca,
        b if cb else None, cb + b_off if b_stride is None else b_stride, b_off, cb, pool, frame_off if pool else None,
        weights, co, act, out, co if out_stride is None else out_stride, stats, "OUT"]


def rows_form_calls():
    for h, w, ca, cb, co in SHAPES:
        for stats in (0, 1):
            yield rows_form(BF16, NF, h, w, ca, cb, co, stats=stats)
            if cb:
                yield rows_form(BF16, NF, h, w, ca, cb, co, pool=csr(NF * h * w), stats=stats)
    # the variants of tests/test_abi.py
    one = csr(176 * 200)
    for dt, cb, stats in ((F32, 32, 0), (BF16, 32, 0), (BF16, 16, 1), (BF16, 32, 1)):
        yield rows_form(dt, 1, 176, 200, 32, cb, 32, pool=one, stats=stats)
    yield rows_form(BF16, 1, 176, 200, 32, 32, 16, pool=one)
    # alignment: rows, offsets and pointers off the 16-byte grid; a ReLU with statistics; no frames
    g = (BF16, 1, 176, 200, 32, 32, 32)
    yield rows_form(*g, out_stride=36)
    yield rows_form(*g, out_stride=40)
    yield rows_form(*g, a_off=4)
    yield rows_form(*g, a_off=8)
    yield rows_form(*g, a_stride=36)
    yield rows_form(*g, b_off=4, pool=one)
    yield rows_form(*g, b_stride=36)
    yield rows_form(*g, a="Q")
    yield rows_form(*g, b="Q", pool=one)
    yield rows_form(*g, out="Q")
    yield rows_form(*g, act=1, stats=1)
    yield rows_form(*g, act=1)
    yield rows_form(BF16, 0, 176, 200, 32, 32, 32)
    # rejected: the checks it shares with shpl_conv3x3
    yield rows_form(*g, act=2)
    yield rows_form(*g, weights=None)
    yield rows_form(*g, out_stride=16)
    yield rows_form(*g, pool=csr(176 * 200 - 1))
    yield rows_form(*g, pool=one, frame_off=None)
    yield rows_form(*g, out=None)


def wide_form(*args, **kw):
    """shpl_conv3x3_wide_form: rows_form's arguments."""
    return "shpl_conv3x3_wide_form", rows_form(*args, **kw)[1]


def wide_form_calls():
    """Each form (out 1, 2, 3), then one row per rule of wide::supported and of the shared predicate (out 0)."""
    g, px = (BF16, NF, 17, 33), NF * 17 * 33
    yield wide_form(*g, 128, 0, 256)                                     # 1: A only
    yield wide_form(*g, 64, 64, 256)                                     # 1: the smallest, Q = 2
    yield wide_form(*g, 128, 64, 256)
    yield wide_form(*g, 256, 256, 512)                                   # 1: two output blocks
    yield wide_form(*g, 64, 64, 256, act=1)
    yield wide_form(*g, 64, 64, 256, pool=csr(px))                       # 2: the compact pooled runs
    yield wide_form(*g, 64, 64, 256, pool=csr(px, cap=0))                # 2: an empty pool
    yield wide_form(BF16, NF, 18432, 3, 64, 64, 256, pool=csr(NF * 18432 * 3))  # 2: the occupancy table's last map
    yield wide_form(BF16, NF, 18433, 3, 64, 64, 256, pool=csr(NF * 18433 * 3))  # 3: past OCC_MAX_WORDS
    yield wide_form(*g, 64, 64, 256, pool=csr(px, cap=(1 << 24) - 1))    # 2: pool_cap * c_b * 2 = 2^31 - 128
    yield wide_form(*g, 64, 64, 256, pool=csr(px, cap=1 << 24))          # 3: pool_cap * c_b * 2 = 2^31
    # wide::supported
    yield wide_form(*g, 0, 128, 256)                                     # c_a = 0
    yield wide_form(*g, 32, 96, 256)                                     # c_a = 32
    yield wide_form(*g, 64, 96, 256)                                     # c_b no multiple of 64
    yield wide_form(*g, 64, 0, 256)                                      # c_a + c_b = 64: the row form's
    yield wide_form(*g, 32, 32, 256)
    yield wide_form(*g, 64, 64, 128)                                     # c_out no multiple of 256
    yield wide_form(*g, 64, 64, 257)
    yield wide_form(F32, NF, 17, 33, 64, 64, 256)
    yield wide_form(*g, 64, 64, 256, stats=1)
    yield wide_form(BF16, 0, 17, 33, 64, 64, 256)                        # no frame
    # alignment: offsets, rows and pointers off the 16-byte grid (a whole piece off it is fine)
    yield wide_form(*g, 64, 64, 256, a_off=8, b_off=8, out_stride=264)   # 1
    yield wide_form(*g, 64, 64, 256, a_off=3)
    yield wide_form(*g, 64, 64, 256, b_off=3)
    yield wide_form(*g, 64, 64, 256, b_off=3, pool=csr(px))
    yield wide_form(*g, 64, 64, 256, a_stride=68)
    yield wide_form(*g, 64, 64, 256, out_stride=260)
    yield wide_form(*g, 64, 64, 256, a="Q")
    yield wide_form(*g, 64, 64, 256, b="Q")
    yield wide_form(*g, 64, 64, 256, out="Q")
    # a frame's rows end 2^31 bytes or more past its start (k_conv_wide's 32-bit halo offsets): A, a dense B, the
    # materialised map in rows of c_b; the compact runs are bounded by pool_cap
    big = (BF16, 1, 1025, 1024, 64, 64, 256)
    yield wide_form(BF16, 1, 1024, 1024, 64, 64, 256, a_stride=1016, b_stride=1016)  # 1: 2^31 - 2^24 bytes
    yield wide_form(BF16, 1, 1024, 1024, 64, 64, 256, a_stride=1024)
    yield wide_form(*big, a_stride=1024)
    yield wide_form(*big, b_stride=1024)
    yield wide_form(*big, a_stride=1024, b_stride=1024)
    yield wide_form(*big, a_stride=1024, pool=csr(1025 * 1024))
    yield wide_form(*big, b_stride=1024, pool=csr(1025 * 1024))          # 3: the pooled image's rows do not count
    yield wide_form(*big)                                                # 1: contiguous, 2^27 + 2^17 bytes
    yield wide_form(BF16, 1, 1 << 20, 15, 64, 64, 256, pool=csr(15 << 20))  # 3: a map of 15 * 2^27 bytes
    yield wide_form(BF16, 1, 1 << 20, 16, 64, 64, 256, pool=csr(16 << 20))  # a map of 2^31 bytes
    # rejected: the checks it shares with shpl_conv3x3
    yield wide_form(*g, 64, 64, 256, act=2)
    yield wide_form(*g, 64, 64, 256, weights=None)
    yield wide_form(*g, 64, 64, 256, pool=csr(px - 1))
    yield wide_form(*g, 64, 64, 256, out=None)


def conv(dt=BF16, nf=1, h=176, w=200, a="P", a_stride=32, a_off=0, ca=32, b="P", b_stride=32, b_off=0, cb=32,
         pool=None, frame_off="P", weights="P", co=32, act=0, out="P", out_stride=32, stats=None, ws="P",
         ws_bytes=1 << 30):
    return "shpl_conv3x3", [dt, nf, h, w, a, a_stride, a_off, ca, b, b_stride, b_off, cb, pool, frame_off, weights,
                            co, None, None, None, act, out, out_stride, stats, ws, ws_bytes, None]


def dgrad(dt=BF16, nf=1, h=176, w=200, gy="P", gy_stride=32, c_gy=32, weights="P", c_dx=64, dx="P", dx_stride=32,
          split=32, dx_b="P", dx_b_stride=32, ws="P", ws_bytes=1 << 30, reuse=None):
    args = [dt, nf, h, w, gy, gy_stride, c_gy, weights, c_dx, dx, dx_stride, split, dx_b, dx_b_stride, ws, ws_bytes]
    if reuse is None:
        return "shpl_conv3x3_dgrad", args + [None]
    return "shpl_conv3x3_dgrad_reuse", args + list(reuse) + [None]  # reuse: pool, fwd_ws, fwd_ws_bytes, fwd_stats


def wgrad(dt=BF16, nf=1, h=176, w=200, a="P", a_stride=32, a_off=0, ca=32, b="P", b_stride=32, b_off=0, cb=32,
          pool=None, frame_off="P", gy="P", gy_stride=32, co=32, dw="P", ws="P", ws_bytes=1 << 30, reuse=None):
    args = [dt, nf, h, w, a, a_stride, a_off, ca, b, b_stride, b_off, cb, pool, frame_off, gy, gy_stride, co, dw, ws,
            ws_bytes]
    if reuse is None:
        return "shpl_conv3x3_wgrad", args + [None]
    return "shpl_conv3x3_wgrad_reuse", args + list(reuse) + [None]  # reuse: fwd_ws, fwd_ws_bytes, fwd_stats


def batch_norm(dt=BF16, rows=100, x="P", y="P", stride=32, c=32, stats="P", count=100.0, act=1, ws="P"):
    return "shpl_batch_norm", [dt, rows, x, y, stride, c, stats, count, 1e-3, "P", "P", act, None, None, 0.999, None,
                               None, ws, None]


def batch_norm_backward(dt=BF16, rows=100, y="P", raw="P", gy="P", stride=32, c=32, act=1, training=1, graw="P",
                        ws="P", ws_bytes=1 << 20):
    return "shpl_batch_norm_backward", [dt, rows, y, raw, gy, stride, c, "P", "P", "P", "P", act, training, graw, "P",
                                        "P", ws, ws_bytes, None]


def rejected_calls():
    """Calls with one fault each, then calls with two: the status says which check came first."""
    one = csr(176 * 200)
    FWS = 1 << 30
    # shpl_conv3x3
    yield conv(dt=7)
    yield conv(act=2)
    yield conv(weights=None)
    yield conv(ws_bytes=16)
    yield conv(ws=None)
    yield conv(a_stride=16)
    yield conv(out_stride=16)
    yield conv(b_stride=16)
    yield conv(a_off=-8, a_stride=64)
    yield conv(b=None)
    yield conv(out=None)
    yield conv(a=None)
    yield conv(co=0)
    yield conv(pool=csr(176 * 200 - 1))
    yield conv(pool=one, frame_off=None)
    yield conv(pool=one, cb=0)
    yield conv(pool=csr(176 * 200, ent=None))
    yield conv(co=0, dt=7)                                   # dtype before shape
    yield conv(co=0, act=2)                                  # the plan before act
    yield conv(act=2, ws_bytes=16)                           # act before the workspace
    yield conv(ws_bytes=16, a_stride=16)                     # the workspace before strides
    yield conv(a_stride=16, pool=one, frame_off=None)        # strides before the pool
    yield conv(pool=csr(176 * 200 - 1), frame_off=None)      # frame_off before the pool's keys
    yield conv(pool=csr(176 * 200 - 1), out=None)            # the pool's keys before the output
    yield conv(b=None, out=None)
    # shpl_conv3x3_dgrad
    yield dgrad(dt=7)
    yield dgrad(weights=None)
    yield dgrad(ws_bytes=16)
    yield dgrad(split=65)
    yield dgrad(split=-1)
    yield dgrad(gy_stride=16)
    yield dgrad(dx_stride=16)
    yield dgrad(dx_b_stride=16)
    yield dgrad(gy=None)
    yield dgrad(dx=None)
    yield dgrad(ws_bytes=16, split=65)                       # the workspace before the split
    yield dgrad(weights=None, ws_bytes=16)                   # weights before the workspace
    yield dgrad(split=65, gy=None)
    # shpl_conv3x3_dgrad_reuse
    yield dgrad(reuse=(None, "P", FWS, 0))
    yield dgrad(reuse=(one, None, FWS, 0))
    yield dgrad(dx_b=None, reuse=(one, "P", FWS, 0))
    yield dgrad(reuse=(csr(176 * 200 - 1), "P", FWS, 0))
    yield dgrad(split=0, reuse=(one, "P", FWS, 0))
    yield dgrad(split=64, reuse=(one, "P", FWS, 0))
    yield dgrad(reuse=(one, "P", 16, 1))                     # a forward workspace smaller than its plan
    yield dgrad(reuse=(one, "P", 16, 0))
    yield dgrad(c_dx=128, split=64, dx_stride=64, dx_b_stride=64, reuse=(one, "P", FWS, 0))  # a dense-only plan
    yield dgrad(c_gy=16, reuse=(one, "P", FWS, 0))           # the forward's outputs not whole blocks
    yield dgrad(c_dx=48, dx_b_stride=16, reuse=(one, "P", FWS, 1))  # statistics the row form does not have
    yield dgrad(dt=F32, reuse=(one, "P", FWS, 0))
    yield dgrad(dt=7, reuse=(one, "P", FWS, 0))
    yield dgrad(weights=None, reuse=(one, "P", FWS, 0))      # past the lookup: shpl_conv3x3_dgrad's own checks
    yield dgrad(ws_bytes=16, reuse=(one, "P", FWS, 0))
    yield dgrad(split=0, reuse=(None, "P", FWS, 0))          # the pool before the split
    yield dgrad(reuse=(csr(176 * 200 - 1), "P", 16, 0))      # the pool's keys before the forward workspace
    yield dgrad(weights=None, reuse=(one, "P", 16, 0))       # the forward workspace before the weights
    # shpl_conv3x3_wgrad
    yield wgrad(dt=7)
    yield wgrad(dw=None)
    yield wgrad(ws_bytes=16)
    yield wgrad(ws=None)
    yield wgrad(a_stride=16)
    yield wgrad(gy_stride=16)
    yield wgrad(b_stride=16)
    yield wgrad(b=None)
    yield wgrad(a=None)
    yield wgrad(gy=None)
    yield wgrad(pool=csr(176 * 200 - 1))
    yield wgrad(pool=one, frame_off=None)
    yield wgrad(pool=csr(176 * 200, ent=None))
    yield wgrad(ws_bytes=16, dw=None)                        # dW before the workspace
    yield wgrad(ws_bytes=16, a_stride=16)                    # the workspace before strides
    yield wgrad(pool=csr(176 * 200 - 1), gy=None)            # the pool's keys before the gradient
    yield wgrad(a_stride=16, pool=one, frame_off=None)
    # shpl_conv3x3_wgrad_reuse
    yield wgrad(reuse=("P", FWS, 0))                         # no pool
    yield wgrad(pool=one, reuse=(None, FWS, 0))
    yield wgrad(dt=F32, pool=one, reuse=("P", FWS, 0))
    yield wgrad(pool=one, reuse=("P", 16, 0))                # a forward workspace smaller than its plan
    yield wgrad(pool=one, reuse=("P", 16, 1))
    yield wgrad(pool=one, ca=64, a_stride=64, cb=64, b_stride=64, reuse=("P", FWS, 0))  # a dense-only plan
    yield wgrad(pool=one, co=16, gy_stride=16, reuse=("P", FWS, 0))
    yield wgrad(pool=one, cb=16, b_stride=16, reuse=("P", FWS, 1))
    yield wgrad(pool=one, ws_bytes=16, reuse=("P", 16, 0))   # this call's workspace before the forward's
    yield wgrad(pool=one, gy=None, reuse=("P", 16, 0))       # the gradient before the forward's workspace
    # shpl_batch_norm
    yield batch_norm(dt=7)
    yield batch_norm(act=2)
    yield batch_norm(stride=16)
    yield batch_norm(c=0)
    yield batch_norm(rows=-1)
    yield batch_norm(stats=None)
    yield batch_norm(ws=None)
    yield batch_norm(x=None)
    yield batch_norm(count=0.0)
    yield batch_norm(dt=7, c=0)
    yield batch_norm(c=0, act=2)
    yield batch_norm(act=2, stats=None)
    # shpl_batch_norm_backward
    yield batch_norm_backward(dt=7)
    yield batch_norm_backward(act=2)
    yield batch_norm_backward(stride=16)
    yield batch_norm_backward(c=(1 << 16) + 1, stride=1 << 17)
    yield batch_norm_backward(ws_bytes=16)
    yield batch_norm_backward(ws=None)
    yield batch_norm_backward(gy=None)
    yield batch_norm_backward(graw=None)
    yield batch_norm_backward(y=None, raw=None)
    yield batch_norm_backward(raw=None)                      # training needs raw
    yield batch_norm_backward(stride=16, act=2)              # shape before act
    yield batch_norm_backward(act=2, ws_bytes=16)            # act before the workspace
    yield batch_norm_backward(ws_bytes=16, gy=None)          # the workspace before the pointers


def record():
    sys.path.insert(0, REPO)
    from sparse_pooling_amd import _lib as L
    lib = L.lib()
    table = {}
    for kind, calls in (("workspace", workspace_calls), ("rows_form", rows_form_calls), ("wide_form", wide_form_calls),
                        ("rejected", rejected_calls)):
        table[kind] = []
        for fn, args in calls():
            rc, out = replay(lib, L, fn, args)
            if kind == "rejected":
                assert rc not in (L.OK, L.ERR_HIP), (fn, args)  # a call that gets through reaches the GPU
            table[kind].append({"fn": fn, "args": args, "status": rc, "out": out})
    return table


if __name__ == "__main__":
    t = record()
    with open(TABLE, "w") as fh:
        fh.write("{\n" + ",\n".join(
            '"%s": [\n%s\n]' % (k, ",\n".join(json.dumps(r) for r in rows)) for k, rows in t.items()) + "\n}\n")
    print({k: len(v) for k, v in t.items()}, "->", TABLE)
