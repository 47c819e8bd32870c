"""Planted batches for the KITTI velodyne loader (shpl_velo_to_cam, csrc/shpl_kitti.hip: VeloStage over the
chunked stable compaction of csrc/shpl_compact.h), shared by tests/test_kitti_cases.py (no GPU: the oracle
against the reference's goldens, and the preconditions that make each case discriminating) and
tests/test_gpu_kitti_edges.py (the device against both).

Every builder returns a ``Batch``

    (scans [F] of (n, 4) f32, rects [F] of (3, 4) f64, Ps [F] of (3, 4) f64 or None, im_sizes [F] of (w, h) or None,
     flips [F], min_intensity, max_points_per_frame (None: the batch's own maximum))

Frames named after a record of tests/golden/kitti_edges.npz (tests/golden/make_golden.py, _kitti_edges_case) carry
the reference's own outputs; every other expectation is the C oracle's (oracle.shpl_oracle.velo_to_cam), which
tests/test_kitti_cases.py ties to the reference on every record.
"""
import collections
import functools
import os

import numpy as np

from oracle import shpl_oracle as orc
from sparse_pooling_amd import synth

IDX_CHUNK = 1024  # points per chunk, one workgroup each: sparse_pooling_amd/csrc/shpl_common.h

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kitti_edges.npz")

Batch = collections.namedtuple("Batch", "scans rects Ps im_sizes flips min_intensity max_points_per_frame")
Frame = collections.namedtuple("Frame", "scan rect P im_size")


@functools.lru_cache(maxsize=None)
def gold():
    with np.load(GOLD) as g:
        return {k: g[k] for k in g.files}


def bits(a):
    """The bytes of an f64 array as u64 words: unlike assert_array_equal on floats this tells -0.0 from 0.0, and
    a NaN from every number. NaNs are first made one quiet NaN. The sign and payload of a NaN that an operation
    makes (0 * inf) or passes on from one of two NaN operands are left to the processor by IEEE 754: x86 and the
    GPU choose differently (measured on the kat scan: 49 of its 996 NaN words), and so may two BLAS kernels of
    the reference's numpy on two CPUs, so those bits of a golden belong to the machine that wrote it. No consumer
    reads them: a NaN row fails every later range test whatever its bits."""
    a = np.array(a, dtype=np.float64, copy=True)
    a[np.isnan(a)] = np.nan
    return np.ascontiguousarray(a).view(np.uint64)


def frame(name):
    """A golden record's inputs as a Frame."""
    g = gold()
    if name == "two_front":
        scan = g["one_front_late_velo"].copy()
        scan[10] = g["two_front_row10"]
    elif name.startswith("calibs"):
        scan = g["calibs0_velo"]
    else:
        scan = g[f"{name}_velo"]
    return Frame(scan, orc.rect_matrix(g[f"{name}_r0_rect"], g[f"{name}_tr"]), g[f"{name}_p2"], g[f"{name}_im_size"])


def _batch(frames, flips, min_intensity=None, max_points_per_frame=None, fov=True):
    return Batch([f.scan for f in frames], [f.rect for f in frames], [f.P for f in frames] if fov else None,
                 [f.im_size for f in frames] if fov else None, list(flips), min_intensity, max_points_per_frame)


# the edges batch's frames and the npz key of the cloud each must give
EDGES = [("kat", 1, "kat_flip_point_cloud"), ("calibs0", 0, "calibs0_point_cloud"),
         ("calibs1", 1, "calibs1_flip_point_cloud"), ("calibs2", 0, "calibs2_point_cloud"),
         ("one_front_late", 1, "one_front_late_flip_point_cloud"), ("two_front", 0, "two_front_point_cloud"),
         ("one_point", 0, "one_point_point_cloud")]
EDGE_AT = 2300  # the lone z > 0 point of one_front_late (chunk 2 of 3)


def edges():
    return _batch([frame(n) for n, _, _ in EDGES], [fl for _, fl, _ in EDGES])


def _lidar_point_at(fr, u, v, z=20.0):
    """A lidar point that fr's calibration projects to about (u, v) at camera depth z."""
    P = fr.P
    cx = (u * (P[2, 2] * z + P[2, 3]) - P[0, 2] * z - P[0, 3]) / P[0, 0]
    cy = (v * (P[2, 2] * z + P[2, 3]) - P[1, 2] * z - P[1, 3]) / P[1, 1]
    return np.linalg.solve(np.vstack([fr.rect, [0, 0, 0, 1]]), [cx, cy, z, 1.0])[:3]


CHUNK_SIZES = [0, 1, IDX_CHUNK - 1, IDX_CHUNK, IDX_CHUNK + 1, 2 * IDX_CHUNK - 1, 2 * IDX_CHUNK, 2 * IDX_CHUNK + 1,
               3 * IDX_CHUNK + 1]


def chunks(max_points_per_frame=None):
    """Scans whose sizes sit on the chunk edges, under the three calibrations in turn, flips alternating. Every
    scan of a chunk or more has two planted points, half a pixel inside its own image's right and lower edges:
    the sizes include 1241 x 376 and 1242 x 375, which few points of a small scan tell apart."""
    rng = np.random.default_rng(71)
    cal = [frame(f"calibs{k}") for k in range(3)]
    frames = []
    for f, n in enumerate(CHUNK_SIZES):
        c = cal[f % 3]
        scan = synth.synthetic_scan(rng, n) if n else np.zeros((0, 4), np.float32)
        if n >= IDX_CHUNK - 1:
            scan[n // 2, :3] = _lidar_point_at(c, c.im_size[0] - 0.5, 100.0)
            scan[n // 3, :3] = _lidar_point_at(c, 600.0, c.im_size[1] - 0.5)
        frames.append(Frame(scan, c.rect, c.P, c.im_size))
    return _batch(frames, [f % 2 for f in range(len(frames))], max_points_per_frame=max_points_per_frame)


N_PATTERN = 3 * IDX_CHUNK + 1  # 4 chunks, the last of one point
PATTERNS = collections.OrderedDict([
    ("none", (lambda i: np.zeros_like(i, bool), [0, 0, 0, 0])),
    ("all", (lambda i: np.ones_like(i, bool), [IDX_CHUNK, IDX_CHUNK, IDX_CHUNK, 1])),
    ("first", (lambda i: i == 0, [1, 0, 0, 0])),
    ("last", (lambda i: i == N_PATTERN - 1, [0, 0, 0, 1])),
    ("chunk1_dropped", (lambda i: i // IDX_CHUNK != 1, [IDX_CHUNK, 0, IDX_CHUNK, 1])),
    ("alternate", (lambda i: i % 2 == 0, [IDX_CHUNK // 2, IDX_CHUNK // 2, IDX_CHUNK // 2, 1])),
    ("chunks_0_3", (lambda i: (i // IDX_CHUNK) % 3 == 0, [IDX_CHUNK, 0, 0, 1])),
])


def patterns():
    """3073-point scans of points well inside every image when in front of the camera; a pattern keeps a point
    by the sign of its lidar x, the camera's z. The calibrations and flips cycle as in `chunks`."""
    rng = np.random.default_rng(72)
    cal = [frame(f"calibs{k}") for k in range(3)]
    frames = []
    i = np.arange(N_PATTERN)
    for f, (mask, _) in enumerate(PATTERNS.values()):
        x = rng.uniform(15, 40, N_PATTERN)
        scan = np.stack([x, x * rng.uniform(-0.4, 0.4, N_PATTERN), x * rng.uniform(-0.08, 0.05, N_PATTERN),
                         rng.uniform(0, 1, N_PATTERN)], 1).astype(np.float32)
        scan[~mask(i), 0] *= -1
        c = cal[f % 3]
        frames.append(Frame(scan, c.rect, c.P, c.im_size))
    return _batch(frames, [f % 2 for f in range(len(frames))])


AUX_AT = 10  # aux_intensity's second z > 0 point (chunk 0), which fails the intensity test


def aux_intensity():
    """Frame 0: one_front_late's scan with a second point in front of the camera, inside the image, whose
    intensity fails min_intensity: it is dropped and still counts as a column of the projection, so the edge
    point (index EDGE_AT) is decided in the two-column order. Frame 1: the scan without it (one column)."""
    one = frame("one_front_late")
    two = one.scan.copy()
    two[AUX_AT] = [20.0, 1.0, -0.5, 0.1]
    return _batch([one._replace(scan=two), one], [0, 0], min_intensity=0.35)


def nofilter():
    """No image filter (P = None): every point passes, NaN and infinite coordinates included."""
    kat = frame("kat")
    c = frame("calibs1")
    return _batch([kat, c._replace(scan=synth.synthetic_scan(np.random.default_rng(73), IDX_CHUNK + 1))], [1, 1],
                  fov=False)


BATCHES = collections.OrderedDict([("edges", edges), ("chunks", chunks), ("patterns", patterns),
                                   ("aux_intensity", aux_intensity), ("nofilter", nofilter)])


def oracle_clouds(b, frames=None):
    """The oracle's (3, n') cloud of every frame of a batch."""
    out = []
    for f in (range(len(b.scans)) if frames is None else frames):
        out.append(orc.velo_to_cam(b.scans[f], b.rects[f], b.Ps[f] if b.Ps is not None else None,
                                   b.im_sizes[f] if b.im_sizes is not None else None,
                                   min_intensity=b.min_intensity, flip=b.flips[f]))
    return out


def front_count(scan, rect):
    """Points of a scan with camera z > 0: the columns of the reference's project_to_image."""
    return int((orc.velo_to_cam(scan, rect)[2] > 0).sum())


def concat(b):
    """The batch as velo_to_cam_batch takes it: xyzi [N,4] f32 and point_offsets [F+1]."""
    off = np.concatenate([[0], np.cumsum([len(s) for s in b.scans])]).astype(np.int64)
    return np.concatenate(b.scans).astype(np.float32), off
