"""The KITTI loader's cases without a GPU (tests/kitti_cases.py): the C oracle equals the reference's recorded
outputs byte for byte on every record of tests/golden/kitti_edges.npz, and every planted case reaches the branch
it was planted for -- a case that could not tell the right kernel from a wrong one proves nothing on the device.

What tests/golden/make_golden.py cannot record, so that the oracle stands alone there:
  * min_intensity on a scan with a point behind the camera (``aux_intensity``): the reference compares the
    intensities of all points with a mask over the z > 0 ones and raises (obj_utils.py:266-267); the filter is
    restated per point and pinned by the reference only on the all-front scan;
  * the capacity layout (NaN holes, counts, the error word, max_points_per_frame): the reference has no batches;
  * the ``chunks`` and ``patterns`` scans: the reference would run on them, their worth is their sizes, which
    mean nothing to it; the oracle it is tied to here has no chunks either.
"""
import os
import re

import numpy as np
import pytest

import kitti_cases as kc
from oracle import shpl_oracle as orc

G = kc.gold()


def _same(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    np.testing.assert_array_equal(kc.bits(got), kc.bits(want))


def test_idx_chunk_is_the_kernels():
    src = open(os.path.join(os.path.dirname(kc.GOLD), "..", "..", "sparse_pooling_amd", "csrc", "shpl_common.h")).read()
    assert int(re.search(r"constexpr int IDX_CHUNK = (\d+);", src).group(1)) == kc.IDX_CHUNK
    assert kc.CHUNK_SIZES == [0, 1, 1023, 1024, 1025, 2047, 2048, 2049, 3073] and kc.N_PATTERN == 3073


@pytest.mark.parametrize("name", [n for n, _, _ in kc.EDGES] + ["all_front_intensity"])
def test_oracle_equals_reference_record(name):
    fr = kc.frame(name)
    for flip, fov, key in ((0, True, "point_cloud"), (1, True, "flip_point_cloud"), (0, False, "point_cloud_all"),
                           (1, False, "flip_point_cloud_all")):
        if f"{name}_{key}" not in G:
            continue
        got = orc.velo_to_cam(fr.scan, fr.rect, fr.P if fov else None, fr.im_size if fov else None, flip=flip)
        _same(got, G[f"{name}_{key}"])
    assert f"{name}_point_cloud" in G


def test_oracle_equals_reference_intensity():
    """The strict threshold on the all-front scan. The reference compares f32 intensities with the threshold as
    f32 (an f32 array against a Python float): f32(0.35) < 0.35 and f32(0.1) > 0.1, and the scan holds both
    and their f32 neighbours. min_intensity = 0 is no filter there (``if not min_intensity``)."""
    fr = kc.frame("all_front_intensity")
    inten = fr.scan[:, 3]
    for key, t in (("035", 0.35), ("01", 0.1)):
        t32 = np.float32(t)
        assert (inten == t32).any() and (inten == np.nextafter(t32, np.float32(1))).any()
        _same(orc.velo_to_cam(fr.scan, fr.rect, fr.P, fr.im_size, min_intensity=float(t32)),
              G[f"all_front_intensity_min{key}"])
    # in f64 the 0.1 threshold keeps the points at f32(0.1): the wrapper's f32 rule is visible on this scan
    assert orc.velo_to_cam(fr.scan, fr.rect, fr.P, fr.im_size, min_intensity=0.1).shape[1] > \
        G["all_front_intensity_min01"].shape[1]
    _same(G["all_front_intensity_min0"], G["all_front_intensity_point_cloud"])
    assert (inten == 0).sum() > 50  # i > 0 would drop them
    assert orc.velo_to_cam(fr.scan, fr.rect, fr.P, fr.im_size, min_intensity=0.0).shape[1] < \
        G["all_front_intensity_min0"].shape[1]


@pytest.mark.parametrize("k", [1, 2, 5])
def test_oracle_equals_reference_lidar_to_cam(k):
    fr = kc.frame("all_front_intensity")
    xyz = G[f"lidar_to_cam{k}_xyz"]
    assert np.array_equal(xyz, xyz.astype(np.float32))  # f32-exact: the device takes f32 scans
    xyzi = np.concatenate([xyz, np.zeros((k, 1))], 1).astype(np.float32)
    _same(orc.velo_to_cam(xyzi, fr.rect).T, G[f"lidar_to_cam{k}_out"])


def test_summation_order_cases_sit_on_the_edge():
    """one_front_late / two_front / aux_intensity: the edge point is kept in exactly one scan of each pair, the
    projection has 1 and 2 columns, and the point lies in another chunk than the column that decides."""
    assert kc.EDGE_AT // kc.IDX_CHUNK == 2 and kc.AUX_AT // kc.IDX_CHUNK == 0
    one, two = kc.frame("one_front_late"), kc.frame("two_front")
    assert (kc.front_count(one.scan, one.rect), kc.front_count(two.scan, two.rect)) == (1, 2)
    edge = orc.velo_to_cam(one.scan[kc.EDGE_AT:kc.EDGE_AT + 1], one.rect)  # (n = 1: dgemv's rect product)
    c1 = orc.velo_to_cam(one.scan, one.rect, one.P, one.im_size)
    c2 = orc.velo_to_cam(two.scan, two.rect, two.P, two.im_size)
    assert c1.shape[1] + c2.shape[1] == 1
    kept = c1 if c1.shape[1] else c2
    assert abs(kept[2, 0] - edge[2, 0]) < 1e-9  # it is the edge point
    # wide of the edge both orders keep it: only the width decides
    wide = [one.im_size[0] + 1, one.im_size[1]]
    assert orc.velo_to_cam(one.scan, one.rect, one.P, wide).shape[1] == 1
    assert orc.velo_to_cam(two.scan, two.rect, two.P, wide).shape[1] == 1
    # aux_intensity: the second column fails the intensity test alone
    b = kc.aux_intensity()
    assert [kc.front_count(s, r) for s, r in zip(b.scans, b.rects)] == [2, 1]
    assert not b.scans[0][kc.AUX_AT, 3] > b.min_intensity < b.scans[0][kc.EDGE_AT, 3]
    no_int = orc.velo_to_cam(b.scans[0], b.rects[0], b.Ps[0], wide)
    assert no_int.shape[1] == 2  # inside the image: only its intensity drops it
    counts = [c.shape[1] for c in kc.oracle_clouds(b)]
    assert sorted(counts) == [0, 1] and counts[0] == c2.shape[1] and counts[1] == c1.shape[1]


def test_one_point_sits_on_the_edge():
    """one_point: both products have one column. The image's width is the smallest u of the other three pairs
    of orders, so a wrong order in either product drops the point; the cloud's bytes pin the rect product's."""
    fr = kc.frame("one_point")
    assert fr.scan.shape[0] == 1 and G["one_point_point_cloud"].shape[1] == 1
    # in a two-point scan (dgemm's order) the same point has other coordinates
    pair = orc.velo_to_cam(np.concatenate([fr.scan, fr.scan]), fr.rect)
    assert not np.array_equal(kc.bits(pair[:, :1]), kc.bits(G["one_point_point_cloud_all"]))
    assert orc.velo_to_cam(np.concatenate([fr.scan, fr.scan]), fr.rect, fr.P, fr.im_size).shape[1] == 0


def _swaps_show(frames, others):
    for fr in frames:
        own = orc.velo_to_cam(fr.scan, fr.rect, fr.P, fr.im_size)
        for o in others:
            if o.P is fr.P:
                continue
            for swapped in (fr._replace(rect=o.rect), fr._replace(P=o.P), fr._replace(im_size=o.im_size)):
                got = orc.velo_to_cam(*swapped)
                assert got.shape != own.shape or not np.array_equal(kc.bits(got), kc.bits(own))


def test_another_frames_calibration_shows():
    """calibs and chunks: another frame's rect, P or im_size, each alone, changes the frame's cloud. (Frames of
    0 and 1 points have nothing to tell them apart; the chunk-sized ones each carry a planted point.)"""
    cal = [kc.frame(f"calibs{k}") for k in range(3)]
    _swaps_show(cal, cal)
    b = kc.chunks()
    frames = [kc.Frame(s, r, p, i) for s, r, p, i in zip(b.scans, b.rects, b.Ps, b.im_sizes)]
    big = [fr for fr in frames if len(fr.scan) >= kc.IDX_CHUNK - 1]
    assert len(big) == 7
    for fr in big:
        _swaps_show([fr], [c for c in cal if c.P is not fr.P])
    assert [len(s) for s in b.scans] == kc.CHUNK_SIZES and len(set(b.flips)) == 2
    e = kc.edges()
    assert len({tuple(np.ravel(r)) for r in e.rects}) >= 5 and len({tuple(i) for i in e.im_sizes}) >= 5


def test_kat_bounds_are_strict():
    """kat: u = x, v = y, w = 1 exactly, so the kept set is known in plain numpy; moving any strict bound to a
    non-strict one changes it. The image filter keeps x > 0 only, so a -0.0 can appear only where there is no
    filter: the flipped unfiltered cloud holds one for every x = +-0.0."""
    fr = kc.frame("kat")
    W, H = fr.im_size
    x, y, z = (fr.scan[:, k].astype(np.float64) for k in range(3))
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)  # 0 * inf in any row poisons all three

        def kept(z0=z > 0, x0=x > 0, x1=x < W, y0=y > 0, y1=y < H):
            return fin & z0 & x0 & x1 & y0 & y1
        strict = kept()
        _same(np.stack([x, y, z])[:, strict], G["kat_point_cloud"])
        for relaxed in (kept(z0=z >= 0), kept(x0=x >= 0), kept(x1=x <= W), kept(y0=y >= 0), kept(y1=y <= H)):
            assert relaxed.sum() > strict.sum()
    den = np.nextafter(np.float32(0), np.float32(1))
    for col in (x, y, z):
        assert (col[strict] == den).any()  # denormals are kept, as numbers above zero
    assert 0 < strict.sum() < len(x) and not fin.all()
    flipped = G["kat_flip_point_cloud_all"]
    plain = G["kat_point_cloud_all"]
    # (a lidar x of -0.0 is +0.0 in the camera frame already: the product's later terms add +0.0 to it)
    assert (plain[0] == 0).sum() == ((x == 0) & fin).sum() > 0 and not np.signbit(plain[0][plain[0] == 0]).any()
    assert np.signbit(flipped[0][flipped[0] == 0]).all() and (flipped[0] == 0).sum() == (plain[0] == 0).sum()
    assert not np.signbit(G["kat_flip_point_cloud"][1:]).any() and (G["kat_flip_point_cloud"][0] < 0).all()


def test_patterns_keep_what_their_names_say():
    b = kc.patterns()
    assert len(b.scans) == len(kc.PATTERNS) == 7 and len({tuple(i) for i in b.im_sizes}) == 3
    i = np.arange(kc.N_PATTERN)
    for f, (name, (mask, per_chunk)) in enumerate(kc.PATTERNS.items()):
        every = orc.velo_to_cam(b.scans[f], b.rects[f], flip=b.flips[f])
        got = orc.velo_to_cam(b.scans[f], b.rects[f], b.Ps[f], b.im_sizes[f], flip=b.flips[f])
        m = mask(i)
        _same(got, every[:, m])  # the kept set is the mask
        assert np.bincount(i[m] // kc.IDX_CHUNK, minlength=4).tolist() == per_chunk, name


def test_nofilter_passes_everything():
    b = kc.nofilter()
    assert b.Ps is None and b.im_sizes is None and all(b.flips)
    assert [c.shape[1] for c in kc.oracle_clouds(b)] == [len(s) for s in b.scans] == [700, 1025]
    assert np.isnan(b.scans[0][:, :3]).any() and np.isinf(b.scans[0][:, :3]).any()
