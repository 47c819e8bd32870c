"""The KITTI velodyne loader on the device (shpl_velo_to_cam, csrc/shpl_kitti.hip: VeloStage over k_count /
k_compact of csrc/shpl_compact.h) on the planted batches of tests/kitti_cases.py: every frame with its own
calibration and image size, points on every bound, scans on every chunk edge, the dgemm / dgemv boundary of the
projection across chunks, capacity, buffer reuse and the single-frame wrappers. Expectations are the reference's
goldens (tests/golden/kitti_edges.npz) and the C oracle, which tests/test_kitti_cases.py ties to them and which
proves there that each case reaches what it was planted for. Every comparison is bitwise.
"""
import numpy as np
import pytest
import torch

import kitti_cases as kc

pytestmark = pytest.mark.gpu

DEV = "cuda"
GARBAGE = 12345.678
G = kc.gold()


def _np(t):
    return t.detach().cpu().numpy()


def _same(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    np.testing.assert_array_equal(kc.bits(got), kc.bits(want), err_msg=str(what))


def _run(b, max_points_per_frame=None, ws=None, out=None):
    """One velo_to_cam_batch call over a Batch: (points [N,3], counts [F], err, offsets [F+1]) as numpy. The
    output starts as finite garbage: an uninitialised buffer is often an earlier call's, with its NaN holes
    still in place, and would hide a hole that is never written."""
    from sparse_pooling_amd import kitti
    xyzi, off = kc.concat(b)
    if out is None:
        out = torch.full((max(len(xyzi), 1), 3), GARBAGE, dtype=torch.float64, device=DEV)
    fov = b.Ps is not None
    if max_points_per_frame is None:
        max_points_per_frame = b.max_points_per_frame
    vb = kitti.velo_to_cam_batch(torch.from_numpy(xyzi).to(DEV), torch.from_numpy(off).to(DEV), np.stack(b.rects),
                                 np.stack(b.Ps) if fov else None, np.stack(b.im_sizes) if fov else None,
                                 min_intensity=b.min_intensity, flip=b.flips,
                                 max_points_per_frame=max_points_per_frame, ws=ws, out=out)
    torch.cuda.synchronize()
    return _np(vb.points)[:off[-1]], _np(vb.counts), int(vb.err.item()), off


def _check_frame(pts, counts, off, f, want, what):
    n = int(counts[f])
    assert n == want.shape[1], (what, f, n, want.shape)
    _same(pts[off[f]:off[f] + n].T, want, (what, f))
    assert np.isnan(pts[off[f] + n:off[f + 1]]).all(), (what, f)  # the holes, all three columns


@pytest.fixture(scope="module")
def fresh():
    """Every batch's default call, run once and left unchanged: (points, counts, err, offsets)."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _run(kc.BATCHES[name]())
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(kc.BATCHES))
def test_batch_vs_oracle(fresh, name):
    b = kc.BATCHES[name]()
    pts, counts, err, off = fresh(name)
    assert err == 0
    for f, want in enumerate(kc.oracle_clouds(b)):
        _check_frame(pts, counts, off, f, want, name)
    if name == "nofilter":
        assert counts.tolist() == [len(s) for s in b.scans]


def test_edges_vs_reference_golden(fresh):
    pts, counts, err, off = fresh("edges")
    assert err == 0
    for f, (name, _, key) in enumerate(kc.EDGES):
        _check_frame(pts, counts, off, f, G[key], name)
    # the unfiltered kat cloud, flipped, in the nofilter batch: the -0.0 of every flipped zero
    pts, counts, err, off = fresh("nofilter")
    _check_frame(pts, counts, off, 0, G["kat_flip_point_cloud_all"], "kat, no filter")


def test_max_points_above_the_batch(fresh):
    """max_points_per_frame = 5000: five chunks per frame, the trailing ones empty, in a workspace sized for it."""
    from sparse_pooling_amd import _lib as L
    b = kc.chunks()
    ws = L.workspace(L.ws_bytes("shpl_velo", len(b.scans), 5000), DEV)
    assert ws.numel() > L.ws_bytes("shpl_velo", len(b.scans), max(kc.CHUNK_SIZES))
    pts, counts, err, off = _run(b, max_points_per_frame=5000, ws=ws)
    want = fresh("chunks")
    assert err == 0
    np.testing.assert_array_equal(counts, want[1])
    np.testing.assert_array_equal(kc.bits(pts), kc.bits(want[0]))


def test_reused_buffers_leave_no_stale_row(fresh):
    """One workspace and one output, as FramePipeline.velo_step reuses them: filled with finite garbage, then
    `patterns`, then `chunks` (the smaller batch: the buffers keep the larger one's size). The second result is
    a fresh call's, byte for byte -- holes included --, and the rows past it are still the first call's."""
    from sparse_pooling_amd import _lib as L
    pa, ch = kc.patterns(), kc.chunks()
    n_pa, n_ch = sum(map(len, pa.scans)), sum(map(len, ch.scans))
    assert n_pa > n_ch
    nb = max(L.ws_bytes("shpl_velo", len(pa.scans), kc.N_PATTERN), L.ws_bytes("shpl_velo", len(ch.scans), kc.N_PATTERN))
    ws = torch.full((nb,), 0x5A, dtype=torch.uint8, device=DEV)
    out = torch.full((n_pa, 3), GARBAGE, dtype=torch.float64, device=DEV)
    first = _run(pa, ws=ws, out=out)
    np.testing.assert_array_equal(kc.bits(first[0]), kc.bits(fresh("patterns")[0]))
    np.testing.assert_array_equal(first[1], fresh("patterns")[1])
    pts, counts, err, off = _run(ch, ws=ws, out=out)
    assert err == 0 and first[2] == 0
    np.testing.assert_array_equal(counts, fresh("chunks")[1])
    np.testing.assert_array_equal(kc.bits(pts), kc.bits(fresh("chunks")[0]))
    np.testing.assert_array_equal(kc.bits(_np(out)[n_ch:]), kc.bits(first[0][n_ch:]))


def test_capacity_bit(fresh):
    """max_points_per_frame = 2048 under scans of 2049 and 3073 points: the capacity bit and no other; every
    frame that fits is exact; an oversized frame's rows past its two processed chunks are holes and its count
    is at most its capacity. (count_phase raises the bit in the frame's last chunk; compact_phase bounds the
    last chunk's holes by cap_end.)"""
    from sparse_pooling_amd import _lib as L
    b = kc.chunks()
    cap = 2 * kc.IDX_CHUNK
    pts, counts, err, off = _run(b, max_points_per_frame=cap)
    assert err == L.EBIT_CAPACITY
    want = fresh("chunks")
    over = [f for f, n in enumerate(kc.CHUNK_SIZES) if n > cap]
    assert len(over) == 2
    for f, n in enumerate(kc.CHUNK_SIZES):
        if f in over:
            assert 0 <= counts[f] <= cap
            assert np.isnan(pts[off[f] + cap:off[f + 1]]).all()
        else:
            assert counts[f] == want[1][f]
            np.testing.assert_array_equal(kc.bits(pts[off[f]:off[f + 1]]), kc.bits(want[0][off[f]:off[f + 1]]))


@pytest.fixture(scope="module")
def edge_files(tmp_path_factory):
    """The kat, one_point and all_front_intensity records as KITTI files (calib/, velodyne/)."""
    d = tmp_path_factory.mktemp("kitti_edges")
    (d / "calib").mkdir()
    (d / "velodyne").mkdir()
    names = ("kat", "one_point", "all_front_intensity")
    for idx, name in enumerate(names):
        (d / "calib" / ("%06d.txt" % idx)).write_text(str(G[f"{name}_calib_text"]))
        G[f"{name}_velo"].astype(np.float32).tofile(str(d / "velodyne" / ("%06d.bin" % idx)))
    return str(d / "calib"), str(d / "velodyne"), names


@pytest.mark.parametrize("min_intensity", [None, 0, 0.35, 0.1])
@pytest.mark.parametrize("im", ["none", "empty", "wh"])
def test_get_lidar_point_cloud_wrapper(edge_files, min_intensity, im):
    """kitti.get_lidar_point_cloud as the reference's: im_size None / [] mean no filter at all, min_intensity
    None / 0 no intensity filter, and a threshold compares as f32 (0.1 rounds up to f32, 0.35 down)."""
    from sparse_pooling_amd import kitti
    calib_dir, velo_dir, names = edge_files
    for idx, name in enumerate(names):
        if min_intensity and name != "all_front_intensity":
            continue  # the reference raises there (its mask lengths); the per-point filter is the oracle's alone
        im_size = {"none": None, "empty": [], "wh": list(G[f"{name}_im_size"])}[im]
        got = _np(kitti.get_lidar_point_cloud(idx, calib_dir, velo_dir, im_size=im_size, min_intensity=min_intensity))
        if im != "wh":
            want = G[f"{name}_point_cloud_all"]
        elif min_intensity:
            want = G[f"{name}_min" + {0.35: "035", 0.1: "01"}[min_intensity]]
        else:
            want = G[f"{name}_point_cloud"]
        _same(got, want, (name, im, min_intensity))


@pytest.mark.parametrize("k", [1, 2, 5])
def test_lidar_to_cam_frame_wrapper(k):
    from sparse_pooling_amd import kitti
    fc = kitti.FrameCalibrationData()
    fc.r0_rect, fc.tr_velodyne_to_cam = G["all_front_intensity_r0_rect"], G["all_front_intensity_tr"]
    _same(_np(kitti.lidar_to_cam_frame(G[f"lidar_to_cam{k}_xyz"], fc)), G[f"lidar_to_cam{k}_out"], k)
