"""Record tests/golden/frames_host_plan.json: what the frame producers' host code of libshpl.so answers without
a GPU -- the BEV voxelizer's, the MV3D producer's and the velodyne loader's workspace sizes, and the status of
calls they reject before their first HIP call (so the order of the argument checks).
tests/test_frames_host_plan.py replays every row against the built library. The committed table was recorded
from the library of the commit before the frame producers' clean-up (docs/HISTORY.md §22), so that clean-up is
held to the answers of the code it replaced.

Each row is {"fn", "args", "status", "out"}, with make_index_host_plan.py's conventions for args:
  "P" / "Q"   a fake non-null device pointer, 16-byte aligned (256) / not (264); never dereferenced
  null        NULL
  [..]        a small host array of doubles (extents, slice bounds, density table, ranges), passed by pointer
  "OUT"       the size_t the call writes; "out" holds its value (null unless status is 0)

No row gets through to a launch or a fill. A workspace of 0 bytes stops the calls whose arguments are otherwise
fine; shpl_mv3d_augment_points has no workspace, so each of its rows carries a fault. Left out, because the
code would reach HIP with them: a fully valid call; a shpl_bev_slices row with map pointers and a geometry that
passes (the fills come before the dtype check -- its dtype rows have null maps); a shpl_bev_maps row with
zero = 1 and maps whose other arguments pass. Left out as well: a negative total_points in shpl_bev_slices and
shpl_mv3d_voxels, which neither checks before it sizes the workspace.

Run (after building the library):  python tests/golden/make_frames_host_plan.py
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
TABLE = os.path.join(HERE, "frames_host_plan.json")

F32, BF16, F64 = 0, 1, 2
BIG = 1 << 40  # bytes of a fake workspace that is never too small

# a BEV geometry that passes (800 x 700 cells, 81 discrete heights, 6 * 560,000 keys) and the MV3D default ranges
EXT = [-40.0, 40.0, -5.0, 3.0, 0.0, 70.0]
LO = [-0.2, 0.3, 0.8, 1.3, 1.8]
HI = [0.3, 0.8, 1.3, 1.8, 2.3]
TABLE16 = [0.0, 0.25, 0.396, 0.5, 0.58, 0.646, 0.702, 0.75, 0.792, 0.83, 0.865, 0.896, 0.925, 0.952, 0.977, 1.0]
RANGES = [0.0, 47.99, -20.0, 19.99, -1.0, 2.99]


def replay(lib, L, fn, args):
    """(status, out) of one recorded call."""
    out = ctypes.c_size_t(0)
    keep, c = [], []
    for a in args:
        if a == "P" or a == "Q":
            c.append(ctypes.c_void_p({"P": 256, "Q": 264}[a]))
        elif a == "OUT":
            c.append(ctypes.byref(out))
        elif isinstance(a, list):
            keep.append((ctypes.c_double * len(a))(*a))
            c.append(ctypes.cast(keep[-1], ctypes.c_void_p))
        else:
            c.append(a)
    rc = getattr(lib, fn)(*c)
    return rc, (out.value if "OUT" in args and rc == 0 else None)


def workspace_calls():
    points = (0, 1, 1023, 1024, 1025, 10239, 10240, 10241, 131072, 2000000)  # around a block and a window, and past
    for s in range(1, 9):
        for n in points:
            yield "shpl_bev_workspace_bytes", [n, s, "OUT"]
    yield "shpl_bev_workspace_bytes", [1000, 5, None]
    yield "shpl_bev_workspace_bytes", [-1, 5, "OUT"]
    yield "shpl_bev_workspace_bytes", [1000, 0, "OUT"]
    yield "shpl_bev_workspace_bytes", [1000, 9, "OUT"]
    for n in points:
        yield "shpl_mv3d_workspace_bytes", [n, "OUT"]
    yield "shpl_mv3d_workspace_bytes", [1000, None]
    yield "shpl_mv3d_workspace_bytes", [-1, "OUT"]
    for nf in (1, 4, 64):
        for n in points:
            yield "shpl_velo_workspace_bytes", [nf, n, "OUT"]
    yield "shpl_velo_workspace_bytes", [1, 1000, None]
    yield "shpl_velo_workspace_bytes", [0, 1000, "OUT"]
    yield "shpl_velo_workspace_bytes", [1, -1, "OUT"]


def bev_slices(nf=2, off="P", counts=None, n=5000, pts="P", pdt=F64, planes="P", ext=EXT, vs=0.1, s=5, lo=LO, hi=HI,
               table=TABLE16, vox="P", upts="P", nvox="P", hm="P", dm="P", err="P", ws="P", ws_bytes=0):
    return "shpl_bev_slices", [nf, off, counts, n, pts, pdt, planes, ext, vs, s, lo, hi, -0.2, 2.3, 0.5, table, vox,
                               upts, nvox, hm, dm, err, ws, ws_bytes, None]


def bev_maps(nf=2, off="P", n=5000, pts="P", pdt=F64, planes="P", ext=EXT, vs=0.1, s=5, lo=LO, hi=HI, table=TABLE16,
             hm="P", dm="P", zero=0, ws="P", ws_bytes=0):
    return "shpl_bev_maps", [nf, off, n, pts, pdt, planes, ext, vs, s, lo, hi, -0.2, 2.3, 0.5, table, hm, dm, zero, ws,
                             ws_bytes, None]


def bev_input(nf=2, off="P", n=5000, pts="P", pdt=F64, planes="P", ext=EXT, vs=0.1, s=5, lo=LO, hi=HI, table=TABLE16,
              out="P", ws="P", ws_bytes=0):
    return "shpl_bev_input", [nf, off, n, pts, pdt, planes, ext, vs, s, lo, hi, -0.2, 2.3, 0.5, table, out, ws,
                              ws_bytes, None]


def mv3d_voxels(nf=2, off="P", n=5000, pts="P", stride=4, img2="P", P=None, fv=None, ranges=RANGES, res=0.2, zres=0.4,
                cap=45, img="P", ld=5000, bv="P", mval="P", fn="P", nb=None, nvox=None, ws="P", ws_bytes=0):
    return "shpl_mv3d_voxels", [nf, off, n, pts, stride, img2, P, fv, ranges, res, zres, cap, img, ld, bv, mval, fn,
                                nb, nvox, ws, ws_bytes, None]


def mv3d_voxels_aug(nf=2, off="P", n=5000, pts="P", pdt=F64, stride=4, img2=None, P="P", fv=None, vox_aug="P",
                    remain=None, roff=None, n_out=5000, ranges=RANGES, res=0.2, zres=0.4, cap=45, img="P", ld=5000,
                    bv="P", mval="P", fn="P", nb=None, nvox=None, err="P", ws="P", ws_bytes=0):
    return "shpl_mv3d_voxels_aug", [nf, off, n, pts, pdt, stride, img2, P, fv, vox_aug, remain, roff, n_out, ranges,
                                    res, zres, cap, img, ld, bv, mval, fn, nb, nvox, err, ws, ws_bytes, None]


def augment_points(nf=2, off="P", n=5000, pts="P", pdt=F64, stride=4, P="P", vox_aug="P", remain=None, roff=None,
                   n_out=5000, cloud="P", img2="P", ld=5000, err="P"):
    return "shpl_mv3d_augment_points", [nf, off, n, pts, pdt, stride, P, vox_aug, remain, roff, n_out, cloud, img2, ld,
                                        err, None]


def velo_to_cam(nf=2, off="P", max_pts=5000, xyzi="P", rect="P", P="P", im_size="P", flip=None, pts="P", counts="P",
                err="P", ws="P", ws_bytes=0):
    return "shpl_velo_to_cam", [nf, off, max_pts, xyzi, rect, P, im_size, 0.0, flip, pts, counts, err, ws, ws_bytes,
                                None]


# geometries bev_geom refuses after its pointer and slice checks: no column, no row, no height, 1024 discrete
# heights and more, 2^22 keys and more
BAD_GEOMS = (dict(ext=[40.0, -40.0, -5.0, 3.0, 0.0, 70.0]), dict(ext=[-40.0, 40.0, -5.0, 3.0, 70.0, 0.0]),
             dict(ext=[-40.0, 40.0, 3.0, -5.0, 0.0, 70.0]), dict(ext=[-40.0, 40.0, -60.0, 60.0, 0.0, 70.0]),
             dict(s=8, lo=LO + LO[:3], hi=HI + HI[:3]))


def rejected_calls():
    """Calls with one fault each (a 0-byte workspace where there is no other), then calls with two: the status
    says which check came first."""
    # ---- shpl_bev_slices
    yield bev_slices()
    yield bev_slices(counts="P", err=None)
    yield bev_slices(n=0, pts=None, vox=None, upts=None)   # an empty batch needs none of the three
    yield bev_slices(nf=5000)                              # more frames than word counts are kept for: still served
    yield bev_slices(hm=None, dm=None)
    yield bev_slices(nf=0)
    for name in ("off", "planes", "ext", "lo", "hi", "table", "nvox", "ws", "pts", "vox", "upts"):
        yield bev_slices(**{name: None})
    yield bev_slices(s=0)
    yield bev_slices(s=9)
    yield bev_slices(vs=0.0)
    yield bev_slices(vs=-0.1)
    yield bev_slices(n=1 << 31)
    yield bev_slices(n=(1 << 31) - 1, ws_bytes=1 << 30)
    yield bev_slices(ws_bytes=1024)
    for s in range(1, 9):                                  # one byte short at every slice count
        g = dict(ext=[-20.0, 20.0, -5.0, 3.0, 0.0, 40.0], s=s, lo=(LO + LO)[:s], hi=(HI + HI)[:s])
        yield bev_slices(ws_bytes=_bev_bytes(5000, s) - 1, **g)
    for g in BAD_GEOMS:                                    # the geometry, behind the workspace
        yield bev_slices(ws_bytes=BIG, **g)
    for pdt in (F32, BF16, 7, -1):                         # the dtype, behind everything else: null maps, no fill
        yield bev_slices(pdt=pdt, hm=None, dm=None, ws_bytes=BIG)
    yield bev_slices(pdt=F32, hm=None, dm=None)
    yield bev_slices(nf=0, s=0)                            # pointers before the slice count
    yield bev_slices(table=None, vs=0.0)
    yield bev_slices(s=0, pts=None)                        # the slice count before the point arrays
    yield bev_slices(vs=0.0, vox=None)
    yield bev_slices(pts=None, n=1 << 31)                  # the point arrays before the point count
    yield bev_slices(n=1 << 31, ws_bytes=0)                # the point count before the workspace
    for g in BAD_GEOMS:                                    # the workspace before the geometry
        yield bev_slices(ws_bytes=0, **g)
    for g in BAD_GEOMS:                                    # the geometry before the dtype
        yield bev_slices(pdt=F32, hm=None, dm=None, ws_bytes=BIG, **g)
    yield bev_slices(pdt=F32, s=9, hm=None, dm=None, ws_bytes=BIG)
    # ---- shpl_bev_maps and shpl_bev_input: the same checks, the geometry before the workspace
    for make, out in ((bev_maps, "hm"), (bev_input, "out")):
        yield make()
        yield make(n=0, pts=None)
        yield make(nf=4096)
        yield make(nf=0)
        for name in ("off", "planes", "ws", "pts", "ext", "lo", "hi", "table"):
            yield make(**{name: None})
        for pdt in (F32, BF16, 7, -1):
            yield make(pdt=pdt)
        yield make(n=-1)
        yield make(n=1 << 31)
        yield make(nf=4097)
        yield make(s=0)
        yield make(s=9)
        yield make(vs=0.0)
        for g in BAD_GEOMS:
            yield make(ws_bytes=BIG, **g)
        yield make(ws_bytes=1024)
        yield make(ws_bytes=_bev_bytes(5000, 5) - 1)
        yield make(nf=0, n=-1)                             # pointers before the point count
        yield make(pdt=F32, n=-1)                          # the dtype before the point count
        yield make(pdt=F32, nf=4097)
        yield make(pts=None, n=1 << 31)
        yield make(n=-1, ext=None)                         # the point count before the geometry's pointers
        yield make(nf=4097, table=None)
        yield make(ext=None, s=0)                          # the geometry's pointers before its shapes
        yield make(lo=None, vs=0.0)
        for g in BAD_GEOMS:                                # the geometry before the workspace
            yield make(ws_bytes=0, **g)
        yield make(s=9, ws_bytes=0)
        yield make(vs=0.0, ws_bytes=0)
        yield make(**{out: None})                          # bev_input needs its tensor; the maps are optional
    yield bev_maps(dm=None)
    yield bev_maps(hm=None, dm=None)                       # no map asked for: still checked, stopped by the workspace
    yield bev_maps(zero=1)
    yield bev_maps(zero=1, ws_bytes=0, **BAD_GEOMS[0])
    yield bev_input(out=None, pdt=F32)
    yield bev_input(out=None, n=-1)
    # ---- shpl_mv3d_voxels
    yield mv3d_voxels()
    yield mv3d_voxels(img2=None, P="P")
    yield mv3d_voxels(img2="P", P="P", fv="P", nb="P", nvox="P")
    yield mv3d_voxels(nvox="P")
    yield mv3d_voxels(n=0, ld=0, pts=None, img=None, bv=None, mval=None)
    yield mv3d_voxels(nf=0)
    for name in ("off", "ranges", "fn", "ws", "pts", "img", "bv", "mval"):
        yield mv3d_voxels(**{name: None})
    yield mv3d_voxels(img2=None)
    yield mv3d_voxels(nb="P")
    yield mv3d_voxels(stride=2)
    yield mv3d_voxels(ld=4999)
    yield mv3d_voxels(res=0.0)
    yield mv3d_voxels(zres=-0.4)
    yield mv3d_voxels(cap=0)
    yield mv3d_voxels(n=1 << 31, ld=1 << 31)
    yield mv3d_voxels(ws_bytes=1024)
    for n in (0, 1, 31, 32, 33, 5000):                     # one byte short
        yield mv3d_voxels(n=n, ld=n, ws_bytes=_mv3d_bytes(n) - 1)
    yield mv3d_voxels(res=0.01, zres=0.01, ws_bytes=BIG)   # 2^31 voxels and more, behind the workspace
    yield mv3d_voxels(nf=0, stride=2)                      # pointers before shapes
    yield mv3d_voxels(img=None, ld=4999)
    yield mv3d_voxels(img2=None, res=0.0)
    yield mv3d_voxels(nb="P", cap=0)
    yield mv3d_voxels(stride=2, ws_bytes=0)                # shapes before the workspace
    yield mv3d_voxels(res=0.01, zres=0.01, ws_bytes=0)     # the workspace before the voxel count
    # ---- shpl_mv3d_voxels_aug
    yield mv3d_voxels_aug()
    yield mv3d_voxels_aug(pdt=F32)
    yield mv3d_voxels_aug(img2="P", P=None, fv="P", nb="P", nvox="P", err=None)
    yield mv3d_voxels_aug(remain="P", roff="P", n_out=4000, ld=4000)
    yield mv3d_voxels_aug(n=0, n_out=0, ld=0, pts=None, img=None, bv=None, mval=None)
    yield mv3d_voxels_aug(nf=0)
    for name in ("ranges", "fn", "ws", "off", "vox_aug", "pts", "img", "bv", "mval"):
        yield mv3d_voxels_aug(**{name: None})
    yield mv3d_voxels_aug(remain="P")
    yield mv3d_voxels_aug(roff="P")
    yield mv3d_voxels_aug(pdt=BF16)
    yield mv3d_voxels_aug(pdt=7)
    yield mv3d_voxels_aug(n=-1)
    yield mv3d_voxels_aug(n_out=-1, remain="P", roff="P")
    yield mv3d_voxels_aug(n=1 << 31, n_out=1 << 31, ld=1 << 31)
    yield mv3d_voxels_aug(remain="P", roff="P", n_out=1 << 31, ld=1 << 31)
    yield mv3d_voxels_aug(n_out=4999)                      # no redraw: as many out points as points
    yield mv3d_voxels_aug(P=None)
    yield mv3d_voxels_aug(nb="P")
    yield mv3d_voxels_aug(stride=2)
    yield mv3d_voxels_aug(ld=4999)
    yield mv3d_voxels_aug(remain="P", roff="P", n_out=6000)  # ld counts out points
    yield mv3d_voxels_aug(res=0.0)
    yield mv3d_voxels_aug(zres=-0.4)
    yield mv3d_voxels_aug(cap=0)
    yield mv3d_voxels_aug(ws_bytes=1024)
    yield mv3d_voxels_aug(ws_bytes=_mv3d_bytes(5000) - 1)
    yield mv3d_voxels_aug(remain="P", roff="P", n_out=4000, ld=4000, ws_bytes=_mv3d_bytes(4000) - 1)  # by out points
    yield mv3d_voxels_aug(res=0.01, zres=0.01, ws_bytes=BIG)
    yield mv3d_voxels_aug(nf=0, pdt=7)                     # the call's own pointers before the augmentation's checks
    yield mv3d_voxels_aug(fn=None, n=-1)
    yield mv3d_voxels_aug(vox_aug=None, pdt=7)             # the augmentation's pointers before its dtype
    yield mv3d_voxels_aug(roff="P", n=-1)
    yield mv3d_voxels_aug(pdt=7, img=None)                 # the augmentation before the outputs
    yield mv3d_voxels_aug(n_out=4999, P=None)
    yield mv3d_voxels_aug(img=None, stride=2)              # the outputs before the shapes
    yield mv3d_voxels_aug(P=None, ld=4999)
    yield mv3d_voxels_aug(nb="P", res=0.0)
    yield mv3d_voxels_aug(cap=0, ws_bytes=0)               # the shapes before the workspace
    yield mv3d_voxels_aug(res=0.01, zres=0.01, ws_bytes=0)  # the workspace before the voxel count
    # ---- shpl_mv3d_augment_points: no workspace, a fault in every row
    yield augment_points(nf=0)
    for name in ("P", "off", "vox_aug", "pts", "cloud", "img2"):
        yield augment_points(**{name: None})
    yield augment_points(remain="P")
    yield augment_points(roff="P")
    yield augment_points(pdt=BF16)
    yield augment_points(pdt=-1)
    yield augment_points(n=-1)
    yield augment_points(n_out=-1, remain="P", roff="P")
    yield augment_points(n=1 << 31, n_out=1 << 31, ld=1 << 31)
    yield augment_points(remain="P", roff="P", n_out=1 << 31, ld=1 << 31)
    yield augment_points(n_out=4999)
    yield augment_points(stride=3)
    yield augment_points(ld=4999)
    yield augment_points(remain="P", roff="P", n_out=6000)
    yield augment_points(cloud="Q")
    yield augment_points(pdt=F32, cloud="Q")
    yield augment_points(nf=0, pdt=BF16)                   # the call's own pointers before the augmentation's checks
    yield augment_points(P=None, n=-1)
    yield augment_points(off=None, pdt=BF16)
    yield augment_points(remain="P", n_out=-1)
    yield augment_points(pdt=BF16, cloud=None)             # the augmentation before the outputs
    yield augment_points(n_out=4999, img2=None)
    yield augment_points(cloud=None, stride=3)             # the outputs before the shapes
    yield augment_points(img2=None, ld=4999)
    # ---- shpl_velo_to_cam
    yield velo_to_cam()
    yield velo_to_cam(P=None, im_size=None, flip="P", err=None)
    yield velo_to_cam(max_pts=0, xyzi=None, pts=None)
    yield velo_to_cam(nf=0)
    for name in ("off", "rect", "counts", "ws", "xyzi", "pts", "P", "im_size"):
        yield velo_to_cam(**{name: None})
    yield velo_to_cam(max_pts=-1)
    yield velo_to_cam(xyzi="Q")
    yield velo_to_cam(ws_bytes=255)
    for nf, mp in ((1, 1024), (2, 5000), (64, 131072)):    # one byte short
        yield velo_to_cam(nf=nf, max_pts=mp, ws_bytes=_velo_bytes(nf, mp) - 1)
    yield velo_to_cam(nf=0, max_pts=-1)                    # pointers before shapes
    yield velo_to_cam(P=None, xyzi="Q")
    yield velo_to_cam(max_pts=-1, ws_bytes=0)
    yield velo_to_cam(xyzi="Q", ws_bytes=0)                # shapes before the workspace


def _up(x):
    return (x + 255) // 256 * 256


def _bev_bytes(n, s):
    """shpl_bev_workspace_bytes by its rule: two arrays of a word per (point, slice or density range) and 4096
    frame counts; the workspace rows pin that the library agrees."""
    return 2 * _up(8 * max(n, 1) * (s + 1)) + _up(4 * 4096)


def _mv3d_bytes(n):
    """shpl_mv3d_workspace_bytes: two words and a count per point slot."""
    return 2 * _up(8 * max(n, 1)) + _up(4 * max(n, 1))


def _velo_bytes(nf, mp):
    """shpl_velo_workspace_bytes: the index builder's, three counts per chunk of 1024 points behind a 256-byte head."""
    return 256 + _up(12 * nf * max((mp + 1023) // 1024, 1))


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
