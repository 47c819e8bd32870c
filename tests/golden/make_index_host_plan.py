"""Record tests/golden/index_host_plan.json: what the index and CSR builders' host code of libshpl.so answers
without a GPU -- the three workspace sizes, and the status of calls it rejects before its first HIP call
(so the order of the argument checks). tests/test_index_host_plan.py replays every row against the built
library. The committed table was recorded from the library of the commit before the builders' clean-up
(docs/HISTORY.md §8), so that clean-up is held to the answers of the code it replaced.

Each row is {"fn", "args", "status", "out"}. args are the C arguments in order, with
  "P" / "Q"        a fake non-null device pointer, 16-byte aligned (256) / not (264); never dereferenced
  null             NULL
  {"csr": [...]}   a shpl_csr by reference: ent_dst = ent_src = ent_val, ent_col, n_keys, nnz_cap, key_range,
                   flags, heads, head_k (pointers "P" / null)
  {"copy": [...]}  a shpl_pass_copy by reference: dtype, src, src_stride, out, out_stride, channels
  {"bk": [...]}    a shpl_buckets by reference, its fields in order
  "OUT"            the size_t the call writes; "out" holds its value (null unless status is 0)

No row gets through to a launch: a workspace of 0 bytes stops the calls whose arguments are otherwise fine
(SHPL_ERR_WORKSPACE comes after every argument check and after the dtype / itype rungs of shpl_build_index
and shpl_build_index_buckets; in shpl_gen_index and shpl_produce_index it comes before the rungs, which
therefore cannot be told apart here), and the nnz_cap == 0 calls with key_range, which memset it, are left out.

Run (after building the library):  python tests/golden/make_index_host_plan.py
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
TABLE = os.path.join(HERE, "index_host_plan.json")

F32, BF16, F64 = 0, 1, 2
I32, I64 = 0, 1
BY_CELL, BY_PIXEL = 0, 1
AUTO, FRAME, SEGMENT, RANGE = 0, 1, 2, 3
BIG = 1 << 40  # bytes of a fake workspace that is never too small


def _ptr(t):
    return {"P": 256, "Q": 264, None: None}[t]


def replay(lib, L, fn, args):
    """(status, out) of one recorded call."""
    out = ctypes.c_size_t(0)
    keep, c = [], []
    for a in args:
        if a == "P" or a == "Q":
            c.append(ctypes.c_void_p(_ptr(a)))
        elif a == "OUT":
            c.append(ctypes.byref(out))
        elif isinstance(a, dict):
            if "csr" in a:
                ent, col, n_keys, cap, key_range, flags, heads, head_k = a["csr"]
                s = L.ShplCsr(_ptr(ent), _ptr(ent), _ptr(ent), _ptr(col), n_keys, cap, _ptr(key_range))
                s.flags, s.heads, s.head_k = flags, _ptr(heads), head_k
            elif "copy" in a:
                dt, src, src_stride, dst, dst_stride, channels = a["copy"]
                s = L.ShplPassCopy(dt, _ptr(src), src_stride, _ptr(dst), dst_stride, channels)
            else:
                v = a["bk"]
                s = L.ShplBuckets(*v[:5], *[_ptr(t) for t in v[5:11]], v[11], _ptr(v[12]))
            keep.append(s)
            c.append(ctypes.byref(s))
        else:
            c.append(a)
    rc = getattr(lib, fn)(*c)
    return rc, (out.value if "OUT" in args and rc == 0 else None)


def csr(n_keys, cap=1000, ent="P", col="P", key_range=None, flags=0, heads=None, head_k=0):
    return {"csr": [ent, col, n_keys, cap, key_range, flags, heads, head_k]}


def copy(dt=BF16, src="P", src_stride=64, out="P", out_stride=96, channels=32):
    return {"copy": [dt, src, src_stride, out, out_stride, channels]}


def workspace_calls():
    points = (0, 1, 1023, 1024, 1025, 4096, 20000, 131072)  # around the chunk size and well past it
    for nf in (1, 4, 64):
        for mp in points:
            yield "shpl_build_index_workspace_bytes", [nf, mp, "OUT"]
    yield "shpl_build_index_workspace_bytes", [0, 1000, "OUT"]
    yield "shpl_build_index_workspace_bytes", [1, -1, "OUT"]
    yield "shpl_build_index_workspace_bytes", [1, 1000, None]
    for nf in (1, 4):
        for mp in points:
            for cap, cells, pix in ((nf * mp, 8700, 6750), (0, 0, 0), (nf * mp, 65536, 128), (nf * mp, 129, 65535)):
                yield "shpl_bucket_workspace_bytes", [nf, mp, cap, cells, pix, "OUT"]
    # bucket_shape_ok's limits, each from both sides
    yield "shpl_bucket_workspace_bytes", [1, 1 << 24, 1000, 8700, 6750, "OUT"]
    yield "shpl_bucket_workspace_bytes", [1, (1 << 24) + 1, 1000, 8700, 6750, "OUT"]
    yield "shpl_bucket_workspace_bytes", [1, 1000, (1 << 31) - 1, 8700, 6750, "OUT"]
    yield "shpl_bucket_workspace_bytes", [1, 1000, 1 << 31, 8700, 6750, "OUT"]
    yield "shpl_bucket_workspace_bytes", [1, 1000, -1, 8700, 6750, "OUT"]
    yield "shpl_bucket_workspace_bytes", [1, 1000, 1000, 65537, 6750, "OUT"]
    yield "shpl_bucket_workspace_bytes", [1, 1000, 1000, 8700, 65537, "OUT"]
    yield "shpl_bucket_workspace_bytes", [0, 1000, 1000, 8700, 6750, "OUT"]
    yield "shpl_bucket_workspace_bytes", [1, -1, 1000, 8700, 6750, "OUT"]
    yield "shpl_bucket_workspace_bytes", [1, 1000, 1000, -1, 6750, "OUT"]
    yield "shpl_bucket_workspace_bytes", [1, 1000, 1000, 8700, -1, "OUT"]
    yield "shpl_bucket_workspace_bytes", [1, 1000, 1000, 8700, 6750, None]
    yield "shpl_bucket_workspace_bytes", [0, 1000, 1 << 31, 8700, 6750, "OUT"]  # arguments before the shape
    for n_keys in (0, 1, 8700, 4 * 35200, (1 << 31) - 2):
        for cap in (0, 1, 1000, 18432, 1 << 20, (1 << 31) - 2):
            yield "shpl_csr_workspace_bytes", [n_keys, cap, "OUT"]
    yield "shpl_csr_workspace_bytes", [-1, 1000, "OUT"]
    yield "shpl_csr_workspace_bytes", [1000, -1, "OUT"]
    yield "shpl_csr_workspace_bytes", [1000, 1000, None]


def build_index(nf=2, off="P", counts=None, max_pts=5000, pts="P", pdt=F64, vox="P", vit=I64, vstride=3, P="P",
                im_w=1200.0, im_h=360.0, bv_h=700.0, bv_w=800.0, s_img=8.0, s_bv=8.0, mval=None, cell="P", pix="P",
                val="P", mij=None, flip=None, nnz="P", out_off="P", err="P", ws="P", ws_bytes=0, buckets=None):
    """shpl_build_index, or with buckets = (nnz_cap, bkt, bkt_bytes, cell_copy, pixel_copy) shpl_build_index_buckets."""
    head = [nf, off, counts, max_pts, pts, pdt, vox, vit, vstride, P, im_w, im_h, bv_h, bv_w, s_img, s_bv, mval,
            cell, pix, val]
    tail = [nnz, out_off, err, ws, ws_bytes]
    if buckets is None:
        return "shpl_build_index", head + [mij, flip] + tail + [None]
    return "shpl_build_index_buckets", head + tail + list(buckets) + [None]


def with_buckets(cap=10000, bkt="P", bkt_bytes=BIG, cell_copy=None, pixel_copy=None, **kw):
    return build_index(buckets=(cap, bkt, bkt_bytes, cell_copy, pixel_copy), **kw)


def gen_index(n=1000, pts="P", pdt=F64, vox="P", vit=I64, vstride=3, P="P", bv="P", img="P", ld=1000, nv="P",
              ws="P", ws_bytes=8):
    return "shpl_gen_index", [n, pts, pdt, vox, vit, vstride, P, 1200.0, 360.0, bv, img, ld, nv, ws, ws_bytes, None]


def produce_index(nv=1000, bv="P", bit=I64, bstride=2, img="P", ld=1000, s_img=8.0, s_bv=8.0, mij="P", flip="P",
                  cell="P", pix="P", nk="P", err="P", ws="P", ws_bytes=8):
    return "shpl_produce_index", [nv, bv, bit, bstride, img, ld, 1200.0, 360.0, 700.0, 800.0, s_img, s_bv, mij, flip,
                                  cell, pix, nk, err, ws, ws_bytes, None]


def csr_path(path=AUTO, direction=BY_CELL, order=0, nf=2, off="P", nnz="P", kpf=8700, cell="P", col=None, val="P",
             pix="P", c="default", ws="P", ws_bytes=0):
    if c == "default":
        c = csr(nf * kpf if nf > 0 and kpf > 0 else 1)
    return "shpl_build_csr_path", [path, direction, order, nf, off, nnz, kpf, cell, col, val, pix, c, ws, ws_bytes,
                                   None]


def csr_buckets(nf=2, max_pts=5000, cap=10000, cells=8700, n_pix=6750, off="P", nnz="P", cell="P", pix="P", val="P",
                ws="P", ws_bytes=BIG, err=None, by_cell="default", by_pixel="default"):
    if by_cell == "default":
        by_cell = csr(nf * cells, cap, key_range="P")
    if by_pixel == "default":
        by_pixel = csr(nf * n_pix, cap, key_range="P")
    return "shpl_build_csr_buckets", [{"bk": [nf, max_pts, cap, cells, n_pix, off, nnz, cell, pix, val, ws, ws_bytes,
                                              err]}, by_cell, by_pixel, None]


def rejected_calls():
    """Calls with one fault each (a 0-byte workspace where there is no other), then calls with two: the status
    says which check came first."""
    for make in (build_index, with_buckets):
        # each dtype / itype rung reaches the workspace check; no other value does
        for pdt in (F64, F32):
            for vit in (I64, I32):
                yield make(pdt=pdt, vit=vit)
        yield make(pdt=BF16)
        yield make(pdt=7)
        yield make(vit=2)
        yield make(vit=-1)
        yield make(nf=0)
        yield make(off=None)
        yield make(P=None)
        yield make(ws=None)
        yield make(pts=None)
        yield make(vox=None)
        yield make(cell=None)
        yield make(pix=None)
        yield make(val=None)
        yield make(max_pts=0, pts=None, vox=None, cell=None, pix=None, val=None)  # an empty batch needs none
        yield make(vstride=1)
        yield make(s_img=0.0)
        yield make(s_bv=-1.0)
        yield make(nf=4000, s_bv=1.0)                        # n_frames * cells past 2^31
        yield make(nf=8000, s_img=1.0)                       # n_frames * pixels past 2^31
        yield make(nf=0, vstride=1)                          # arguments before shapes
        yield make(pts=None, s_img=0.0)
        yield make(vstride=1, pdt=7)                         # shapes before the rungs
        yield make(nf=4000, s_bv=1.0, vit=2)
        yield make(max_pts=1 << 20, counts="P", mval="P")
    yield build_index(mij="P", flip="P")
    # shpl_build_index_buckets' own checks
    yield with_buckets(bkt=None)
    yield with_buckets(nnz=None)
    yield with_buckets(max_pts=(1 << 24) + 1)                # bucket_shape_ok: 24-bit entry offsets
    yield with_buckets(max_pts=1 << 24)
    yield with_buckets(cap=-1)
    yield with_buckets(cap=1 << 31)
    yield with_buckets(s_bv=2.0)                             # 140,000 cells: over 512 ranges of 128
    yield with_buckets(s_img=2.0)                            # 108,000 pixels
    yield with_buckets(bkt_bytes=1024)
    yield with_buckets(bkt_bytes=0, max_pts=0, cap=0)
    yield with_buckets(bkt=None, cap=-1)                     # the pointers before the bucket shape
    yield with_buckets(cap=-1, bkt_bytes=0)                  # the bucket shape before its workspace
    yield with_buckets(bkt_bytes=0, cell_copy=copy(dt=7))    # the bucket workspace before the copies
    yield with_buckets(cell_copy=copy(dt=7), pdt=7)          # the copies before the rungs
    yield with_buckets(pdt=7, bkt_bytes=0)
    # make_pass_copy, as the cell copy and as the pixel copy
    for side in ("cell_copy", "pixel_copy"):
        yield with_buckets(**{side: copy()})                 # a good copy: on to the workspace
        yield with_buckets(**{side: copy(dt=F32, channels=32, src_stride=32, out_stride=64)})
        yield with_buckets(**{side: copy(channels=0, src=None, out=None)})  # no channels: no copy
        yield with_buckets(**{side: copy(dt=F64)})
        yield with_buckets(**{side: copy(dt=-1)})
        yield with_buckets(**{side: copy(src=None)})
        yield with_buckets(**{side: copy(out=None)})
        yield with_buckets(**{side: copy(channels=-8)})
        yield with_buckets(**{side: copy(channels=12)})      # a row that is no whole number of 16-byte pieces
        yield with_buckets(**{side: copy(src_stride=68)})
        yield with_buckets(**{side: copy(out_stride=100)})
        yield with_buckets(**{side: copy(src="Q")})
        yield with_buckets(**{side: copy(out="Q")})
        yield with_buckets(**{side: copy(src_stride=24, channels=32)})
        yield with_buckets(**{side: copy(out_stride=24, channels=32)})
        yield with_buckets(**{side: copy(dt=F32, channels=1 << 20, src_stride=1 << 20, out_stride=1 << 20)})  # 2^31 pieces
        yield with_buckets(**{side: copy(dt=7, channels=12)})  # the dtype before the shape
        yield with_buckets(**{side: copy(src=None, channels=12)})
    yield with_buckets(cell_copy=copy(channels=12), pixel_copy=copy(dt=7))  # the cell copy first
    yield with_buckets(cell_copy=copy(), pixel_copy=copy(dt=7))
    # shpl_gen_index: the workspace of the [0, n] pair comes before its rungs
    for pdt in (F64, F32, 7):
        for vit in (I64, I32, 2):
            yield gen_index(pdt=pdt, vit=vit)
    yield gen_index(n=-1)
    yield gen_index(P=None)
    yield gen_index(bv=None)
    yield gen_index(img=None)
    yield gen_index(nv=None)
    yield gen_index(ws=None)
    yield gen_index(pts=None)
    yield gen_index(vox=None)
    yield gen_index(n=0, ld=0, pts=None, vox=None)
    yield gen_index(vstride=1)
    yield gen_index(ld=999)
    yield gen_index(n=-1, vstride=1)
    yield gen_index(vox=None, ld=999)
    yield gen_index(ld=999, ws_bytes=0)
    # shpl_produce_index
    for bit in (I64, I32, 2):
        yield produce_index(bit=bit)
    yield produce_index(nv=-1)
    yield produce_index(mij=None)
    yield produce_index(flip=None)
    yield produce_index(nk=None)
    yield produce_index(ws=None)
    yield produce_index(bv=None)
    yield produce_index(img=None)
    yield produce_index(nv=0, ld=0, bv=None, img=None)
    yield produce_index(cell=None, pix=None, err=None)
    yield produce_index(bstride=1)
    yield produce_index(ld=999)
    yield produce_index(s_img=0.0)
    yield produce_index(s_bv=-2.0)
    yield produce_index(mij=None, bstride=1)
    yield produce_index(img=None, s_img=0.0)
    yield produce_index(ld=999, ws_bytes=0)
    # shpl_build_csr_path
    for path in (AUTO, FRAME, SEGMENT, RANGE):
        for direction in (BY_CELL, BY_PIXEL):
            for col in (None, "P"):
                yield csr_path(path=path, direction=direction, col=col, order=2 if col else 0)
        yield csr_path(path=path, nf=64)
        yield csr_path(path=path, nf=2, kpf=1 << 20, c=csr(2 << 20, 1 << 20))
        yield csr_path(path=path, c=csr(2 * 8700, 1 << 24))                  # a capacity of 2^24: no range builder
        if path != FRAME:                                                     # (FRAME zeroes key_range first)
            yield csr_path(path=path, c=csr(2 * 8700, key_range="P"))
            yield csr_path(path=path, c=csr(2 * 8700, 1 << 24, key_range="P"))  # key_range with capacity >= 2^24
            yield csr_path(path=path, c=csr(2 * 8700, (1 << 24) - 1, key_range="P"))
            yield csr_path(path=path, nf=1, kpf=65535 * 128 + 1, c=csr(65535 * 128 + 1, key_range="P"),
                           ws_bytes=BIG)                                      # more than 65535 ranges
            yield csr_path(path=path, nf=1, kpf=65535 * 128 + 1, c=csr(65535 * 128 + 1, key_range="P"))
    yield csr_path(path=FRAME, c=csr(2 * 8700, 1 << 24, key_range="P"))
    yield csr_path(path=RANGE, nf=1, kpf=65535 * 128 + 1, c=csr(65535 * 128 + 1), ws_bytes=BIG)
    yield csr_path(path=-1)
    yield csr_path(path=4)
    yield csr_path(c=None)
    yield csr_path(off=None)
    yield csr_path(nf=0)
    yield csr_path(c=csr(2 * 8700, key_range="P", heads="P", head_k=4))      # heads: shpl_build_csr_buckets only
    yield csr_path(direction=2)
    yield csr_path(order=-1)
    yield csr_path(order=3)
    yield csr_path(kpf=0)
    yield csr_path(c=csr(2 * 8700, -1))
    yield csr_path(c=csr(2 * 8700 - 1))
    yield csr_path(c=csr((1 << 31) - 1))                                     # the 2^31 key limit
    yield csr_path(c=csr((1 << 31) - 2))
    yield csr_path(c=csr(2 * 8700, (1 << 31) - 1))
    yield csr_path(c=csr(2 * 8700, (1 << 31) - 2))
    yield csr_path(cell=None)
    yield csr_path(val=None)
    yield csr_path(pix=None)
    yield csr_path(ws=None)
    yield csr_path(c=csr(2 * 8700, ent=None))
    yield csr_path(direction=BY_PIXEL, c=csr(2 * 8700, col=None))            # a pixel-keyed CSR without ent_col
    yield csr_path(direction=BY_CELL, c=csr(2 * 8700, col=None))
    yield csr_path(nnz=None)
    yield csr_path(path=4, c=None)                                           # the path before the pointers
    yield csr_path(nf=0, direction=2)
    yield csr_path(c=csr(2 * 8700, heads="P", head_k=4), direction=2)        # heads before the direction
    yield csr_path(direction=2, order=3)
    yield csr_path(order=3, kpf=0)
    yield csr_path(kpf=0, cell=None)                                         # shapes before the entry pointers
    yield csr_path(cell=None, direction=BY_PIXEL, c=csr(2 * 8700, col=None))
    yield csr_path(direction=BY_PIXEL, c=csr(2 * 8700, 1 << 24, col=None, key_range="P"))  # ent_col before key_range
    yield csr_path(ws=None, c=csr(2 * 8700, 1 << 24, key_range="P"))
    # shpl_build_csr_buckets
    yield csr_buckets(ws_bytes=0)
    yield "shpl_build_csr_buckets", [None, csr(1000), csr(1000), None]
    yield csr_buckets(nf=0)
    yield csr_buckets(off=None)
    yield csr_buckets(nnz=None)
    yield csr_buckets(ws=None)
    yield csr_buckets(max_pts=-1)
    yield csr_buckets(cells=-1)
    yield csr_buckets(max_pts=(1 << 24) + 1)
    yield csr_buckets(cap=1 << 31)
    yield csr_buckets(cells=65537)
    yield csr_buckets(n_pix=65537)
    yield csr_buckets(ws_bytes=1024)
    for mp in (1023, 1024, 1025, 4096, 5000):  # the bucket workspace at every chunk count: one byte short
        yield csr_buckets(max_pts=mp, ws_bytes=_bucket_bytes(2, mp, 10000, 8700, 6750) - 1)
    yield csr_buckets(cell=None)
    yield csr_buckets(pix=None)
    yield csr_buckets(val=None)
    for side in ("by_cell", "by_pixel"):
        kpf = 8700 if side == "by_cell" else 6750
        yield csr_buckets(**{side: csr(2 * kpf - 1, 10000, key_range="P")})
        yield csr_buckets(**{side: csr((1 << 31) - 1, 10000, key_range="P")})
        yield csr_buckets(**{side: csr(2 * kpf, 9999, key_range="P")})
        yield csr_buckets(**{side: csr(2 * kpf, 10000, ent=None, key_range="P")})
        yield csr_buckets(**{side: csr(2 * kpf, 10000, key_range="P", heads="P", head_k=0)})
        yield csr_buckets(**{side: csr(2 * kpf, 10000, key_range="P", heads="P", head_k=33)})
        yield csr_buckets(**{side: csr(2 * kpf, 10000, heads="P", head_k=4)})  # heads need key_range
        yield csr_buckets(**{side: csr(2 * kpf - 1, 10000, ent=None)})          # shape before pointers
    yield csr_buckets(by_pixel=csr(2 * 6750, 10000, col=None, key_range="P"))  # a pixel-keyed CSR without ent_col
    yield csr_buckets(by_pixel=csr(2 * 6750, 10000, col=None, ent=None, flags=1))
    yield csr_buckets(by_cell=csr(2 * 8700 - 1, 10000), by_pixel=csr(2 * 6750, 10000, col=None))  # the cell side first
    yield csr_buckets(nf=0, ws_bytes=0)
    yield csr_buckets(cap=1 << 31, ws_bytes=0)               # the bucket shape before the workspace
    yield csr_buckets(ws_bytes=0, cell=None)                 # the workspace before the index arrays
    yield csr_buckets(cell=None, by_cell=csr(2 * 8700 - 1, 10000))
    # shpl_bucket_workspace_reset
    yield "shpl_bucket_workspace_reset", [0, "P", BIG, None]
    yield "shpl_bucket_workspace_reset", [-1, "P", BIG, None]
    yield "shpl_bucket_workspace_reset", [4, None, BIG, None]
    yield "shpl_bucket_workspace_reset", [4, "P", 0, None]
    yield "shpl_bucket_workspace_reset", [4, "P", 31, None]  # 8 bytes per frame
    yield "shpl_bucket_workspace_reset", [1000, "P", 7999, None]
    yield "shpl_bucket_workspace_reset", [0, None, 0, None]


def _bucket_bytes(nf, mp, cap, cells, n_pix):
    """shpl_bucket_workspace_bytes by BkLayout's rule (shpl_common.h) with chunks of 1024 points; the workspace
    rows above pin that the library agrees."""
    up = lambda x: (x + 255) // 256 * 256  # noqa: E731
    nrmax = max((cells + 127) // 128, (n_pix + 127) // 128, 1)
    chunks = max((mp + 1023) // 1024, 1)
    return up(8 * nf) + up(8 * nf * chunks * nrmax) + up(16 * nf * nrmax) + up(8 * max(cap, 1))


def record():
    sys.path.insert(0, REPO)
    from sparse_pooling_amd import _lib as L
    lib = L.lib()
    table = {}
    for kind, calls in (("workspace", workspace_calls), ("rejected", rejected_calls)):
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
