"""The ragged index build on MI355X: batches of mixed image sizes (shpl_build_index_ragged,
shpl_build_index_buckets_ragged and everything above them) against the oracle called per frame with the
frame's OWN image size (tests/ragged_cases.py; pinned to a reference run by tests/test_oracle_ragged_golden.py).

Integer outputs (mij, flip, nnz, pix) must be bit-exact; the layer's outputs and gradients are bitwise equal to the
oracle's under the window rule of ragged_cases (f32, TF-CPU's operation order on both sides).
"""
import os

import numpy as np
import pytest
import torch

import ragged_cases as rc
from oracle import shpl_numpy as onp
from sparse_pooling_amd import synth

pytestmark = pytest.mark.gpu

DEV = "cuda"
GOLD = os.path.join(os.path.dirname(__file__), "golden")
SIZES5 = [rc.KITTI_SIZES[1], rc.KITTI_SIZES[0], rc.KITTI_SIZES[2], rc.KITTI_SIZES[3], rc.HALF]


def _np(t):
    return t.detach().cpu().numpy()


def _same(got, exp):
    got, exp = _np(got), np.asarray(exp, np.float32)
    assert got.shape == exp.shape, (got.shape, exp.shape)
    np.testing.assert_array_equal(got, exp)


def _sizes(sizes):
    return torch.tensor([[float(w), float(h)] for w, h in sizes], dtype=torch.float64, device=DEV)


def _stack(frames, dtype=torch.float64):
    from sparse_pooling_amd import pipeline
    pts, vox, off, P, maxp, N = pipeline.stack_frames(frames, DEV)
    return pts.to(dtype), vox, off, P, maxp, N


# ------------------------------------------------------------------ 1. the two-launch form

@pytest.mark.parametrize("pdt", ["f64", "f32"])
@pytest.mark.parametrize("s", [1, 4, 8])
def test_two_launch_form_matches_oracle_per_frame(s, pdt):
    """Frames across the 1024-point chunk (1025, 1, 0, 3000, 1024 points inside the padded image), each with its
    own image size: mij, flip and nnz per frame are the oracle's at the frame's own size, pix takes the padded
    pitch."""
    from sparse_pooling_amd import shpl_map as sm
    stride = (s, s)
    frames = rc.make_frames([1025, 1, 0, 3000, 1024], stride, 100)
    npdt = np.float64 if pdt == "f64" else np.float32
    refs = rc.frame_refs(frames, SIZES5, stride, npdt)
    pts, vox, off, P, maxp, N = _stack(frames, torch.float64 if pdt == "f64" else torch.float32)
    hp, wp = rc.strided(rc.PADDED, s)
    ib = sm.build_index_batch(pts, vox, off, P, rc.PADDED, rc.BV_SIZE, stride, maxp, ref_outputs=True,
                              im_sizes=_sizes(SIZES5))
    assert ib.img_hw == (hp, wp)
    np.testing.assert_array_equal(_np(ib.img_hw_frames), [rc.strided(sz, s) for sz in SIZES5])
    fo, fn = _np(ib.frame_off), _np(ib.frame_nnz)
    np.testing.assert_array_equal(fo, _np(off))
    differs = 0
    for f, (fr, ref) in enumerate(zip(frames, refs)):
        a, b = fo[f], fo[f] + fn[f]
        assert fn[f] == ref["M_size"][1] == ref["Mij_pool"].shape[0], f
        np.testing.assert_array_equal(_np(ib.mij[a:b]), ref["Mij_pool"])
        np.testing.assert_array_equal(_np(ib.flip[a:b]), ref["img_index_flip_pool"])
        np.testing.assert_array_equal(_np(ib.map.pix[a:b]), rc.pix_ids(ref["img_index_flip_pool"], f, hp, wp))
        np.testing.assert_array_equal(_np(ib.map.cell[a:b]), ref["Mij_pool"][:, 0] + f * int(ref["M_size"][0]))
        assert (_np(ib.map.cell[b:fo[f + 1]]) == -1).all() and (_np(ib.map.pix[b:fo[f + 1]]) == -1).all()
        # the batch can tell a frame's own size from the shared one: the oracle at the padded size differs
        pad = rc.oracle_index(fr.points.astype(npdt).astype(np.float64), fr.voxel_indices, fr.P, rc.PADDED,
                              rc.BV_SIZE, stride)
        differs += pad["Mij_pool"].shape != ref["Mij_pool"].shape or not np.array_equal(
            pad["img_index_flip_pool"], ref["img_index_flip_pool"])
    assert differs >= 3
    assert ib.map.error_bits() == 0


# ------------------------------------------------------------------ 2. the survivor-count edge

def test_one_survivor_at_own_size_projects_like_numpy():
    """A frame whose own width leaves exactly ONE clip survivor while the padded width leaves several: numpy then
    projects the survivor with one column (dgemv's order), and the survivor sits where the two orders round u
    differently (the single_tie golden's point) -- the order must follow the frame's own count."""
    from sparse_pooling_amd import shpl_map as sm
    tie = np.load(os.path.join(GOLD, "index_single_tie.npz"))["points"].reshape(-1, 3)[:1]
    base = rc.make_frames([40], (1, 1), 900)[0]

    def u_of(p):
        uvw = synth.KITTI_P2 @ np.vstack((p.T, np.ones(p.shape[0])))
        return uvw[0] / uvw[2]
    u_tie = float(u_of(tie)[0])
    inside = rc.oracle_index(base.points, base.voxel_indices, base.P, rc.PADDED, rc.BV_SIZE, (1, 1))
    assert inside["Mij_pool"].shape[0] >= 30
    keep = u_of(base.points) > u_tie + 5  # every other point projects right of the survivor (the 7 outside ones too)
    pts = np.concatenate([base.points[keep][:9], tie, base.points[keep][9:]])
    vox = np.concatenate([base.voxel_indices[keep][:9], [[300, 400]], base.voxel_indices[keep][9:]])
    us = u_of(pts)  # (u_tie came from a one-column product: its last bits may differ from this one's)
    assert np.argmin(us) == 9 and abs(us[9] - u_tie) < 1e-9
    us = np.sort(us)
    assert us[1] > u_tie + 5
    own = ((us[0] + us[1]) / 2 + 1.0, 376.0)  # u < W - 1 holds for the smallest u alone
    edge = synth.Frame(pts, vox.astype(np.int64), synth.KITTI_P2, base.spec)
    other = rc.make_frames([50], (1, 1), 901)[0]
    frames, sizes = [other, edge], [rc.KITTI_SIZES[2], own]
    refs = rc.frame_refs(frames, sizes, (1, 1))
    assert refs[1]["Mij_pool"].shape[0] == 1
    at_padded = rc.oracle_index(pts, vox, synth.KITTI_P2, rc.PADDED, rc.BV_SIZE, (1, 1))
    assert at_padded["Mij_pool"].shape[0] > 5
    # the same point among the padded clip's several survivors (found by its BEV row) rounds u the other way
    row = np.flatnonzero(at_padded["Mij_pool"][:, 0] == refs[1]["Mij_pool"][0, 0])
    assert row.size == 1
    assert at_padded["img_index_flip_pool"][row[0], 2] != refs[1]["img_index_flip_pool"][0, 2]
    # numpy's own np.dot (dgemv for one column) says the same as the C oracle
    gen = onp.gen_sparse_pooling_input_avod(pts, vox, synth.KITTI_P2, list(own), rc.BV_SIZE)
    npref = onp.produce_sparse_pooling_input(gen, stride=(1, 1))
    np.testing.assert_array_equal(npref["img_index_flip_pool"], refs[1]["img_index_flip_pool"])
    np.testing.assert_array_equal(npref["Mij_pool"], refs[1]["Mij_pool"])
    dpts, dvox, off, P, maxp, N = _stack(frames)
    ib = sm.build_index_batch(dpts, dvox, off, P, rc.PADDED, rc.BV_SIZE, (1, 1), maxp, ref_outputs=True,
                              im_sizes=_sizes(sizes))
    fo, fn = _np(ib.frame_off), _np(ib.frame_nnz)
    for f, ref in enumerate(refs):
        a, b = fo[f], fo[f] + fn[f]
        assert fn[f] == ref["Mij_pool"].shape[0]
        np.testing.assert_array_equal(_np(ib.mij[a:b]), ref["Mij_pool"])
        np.testing.assert_array_equal(_np(ib.flip[a:b]), ref["img_index_flip_pool"])
    assert ib.map.error_bits() == 0


# ------------------------------------------------------------------ 3. the bucketed forms

def _bucket_case(s, one_launch, seed=300):
    """4 frames (one per KITTI size, one of them with few points) through a bucketed dual ragged pipeline; more
    than 32 chunks of declared capacity per frame force the two-launch form."""
    from sparse_pooling_amd import pipeline
    stride = (s, s)
    sizes = [rc.KITTI_SIZES[1], rc.KITTI_SIZES[3], rc.KITTI_SIZES[0], rc.KITTI_SIZES[2]]
    frames = rc.make_frames([1500, 1025, 3, 700], stride, seed)
    refs = rc.frame_refs(frames, sizes, stride)
    pts, vox, off, P, maxp, N = _stack(frames)
    if not one_launch:
        maxp = 33 * 1024 + 5
    Cb, Ci = 8, 16
    pl = pipeline.FusedPipeline(4, maxp, N, rc.PADDED, rc.BV_SIZE, stride, Cb, Ci, dual=True, rows=True,
                                buckets=True, ragged=True)
    assert pl.buckets and pl.ragged and (pl.Hi, pl.Wi) == rc.strided(rc.PADDED, s)
    return pl, (pts, vox, off, P), sizes, refs, (Cb, Ci)


@pytest.mark.parametrize("one_launch", [True, False], ids=["k_index1", "two_launch"])
@pytest.mark.parametrize("s", [4, 8])
def test_bucketed_forms_layer_and_gradients(s, one_launch):
    """shpl_build_index_buckets_ragged (the one-launch k_index1 and the two-launch form) -> shpl_build_csr_buckets
    -> the pull pairs, forward (step, then step_overlapped with the pass-through halves riding the index launches)
    and backward: bitwise the oracle per frame under the window rule, the padding of the image map filled with a
    non-zero pattern."""
    pl, index, sizes, refs, (Cb, Ci) = _bucket_case(s, one_launch)
    B, (Hb, Wb), (hp, wp) = 4, (pl.Hb, pl.Wb), (pl.Hi, pl.Wi)
    bev = synth.make_features((B, Hb, Wb, Cb), 1)
    img = rc.padded_features(B, hp, wp, Ci, sizes, s, 2)
    g_bv = synth.make_features((B, Hb, Wb, Cb + Ci), 3)
    g_img = rc.padded_features(B, hp, wp, Ci + Cb, sizes, s, 4)
    want = rc.layer_oracle(refs, sizes, s, bev, img, g_bv, g_img)
    tb, ti, tgb, tgi = (torch.from_numpy(x).to(DEV) for x in (bev, img, g_bv, g_img))
    pl.set_image_sizes(_sizes(sizes))
    for form in ("step", "overlapped"):
        pl.bv_fused.fill_(float("nan"))
        pl.img_fused.fill_(float("nan"))
        if form == "step":
            pl.step(*index, tb, ti)
        else:
            assert pl.copy_riders_ok(tb, ti)
            pl.step_overlapped(*index, tb, ti, torch.cuda.Stream())
        d_bev, d_img = torch.empty_like(tb), torch.empty_like(ti)
        pl.backward(tgb, tgi, d_bev, d_img)
        torch.cuda.synchronize()
        assert int(pl.err.item()) == 0
        nnz, fo = _np(pl.frame_nnz), _np(pl.frame_off)
        for f, (eb, ei, e_bev, e_img) in enumerate(want):
            assert nnz[f] == refs[f]["M_size"][1], (form, f)
            np.testing.assert_array_equal(_np(pl.pix[fo[f]:fo[f] + nnz[f]]),
                                          rc.pix_ids(refs[f]["img_index_flip_pool"], f, hp, wp))
            _same(pl.bv_fused[f:f + 1], eb)
            _same(pl.img_fused[f:f + 1], ei)
            _same(d_bev[f:f + 1], e_bev)
            _same(d_img[f:f + 1], e_img)


def test_set_image_sizes_is_captured_with_the_step():
    """set_image_sizes + the bucketed step recorded in one graph: a replay reads the sizes the caller's tensor holds
    then (a device copy on the step's stream), and gives the eager step's bits for them."""
    pl, index, sizes, refs, (Cb, Ci) = _bucket_case(8, True, seed=320)
    bev = torch.from_numpy(synth.make_features((4, pl.Hb, pl.Wb, Cb), 1)).to(DEV)
    img = torch.from_numpy(synth.make_features((4, pl.Hi, pl.Wi, Ci), 2)).to(DEV)
    mine = _sizes([rc.PADDED] * 4)
    pl.step_overlapped(*index, bev, img, None)  # an eager step first: nothing is loaded or sized under capture
    torch.cuda.synchronize()
    graph, gs = torch.cuda.CUDAGraph(), torch.cuda.Stream(device=DEV)
    gs.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(graph, stream=gs):
        pl.set_image_sizes(mine)
        pl.step_overlapped(*index, bev, img, None)
    torch.cuda.synchronize()
    mine.copy_(_sizes(sizes))
    graph.replay()
    torch.cuda.synchronize()
    got = [_np(t).copy() for t in (pl.frame_nnz, pl.pix, pl.bv_fused, pl.img_fused)]
    np.testing.assert_array_equal(got[0], [r["M_size"][1] for r in refs])
    pl.set_image_sizes(_sizes(sizes))
    pl.step_overlapped(*index, bev, img, None)
    torch.cuda.synchronize()
    assert int(pl.err.item()) == 0
    for a, t in zip(got, (pl.frame_nnz, pl.pix, pl.bv_fused, pl.img_fused)):
        np.testing.assert_array_equal(a.view(np.uint8), _np(t).view(np.uint8))


# ------------------------------------------------------------------ 4. raw scans -> layer

def _scans(shapes, n=6000, seed=5):
    from sparse_pooling_amd import kitti
    fc = kitti.FrameCalibrationData()
    c = synth.KITTI_CALIB
    fc.p0, fc.p1, fc.p2, fc.p3 = (np.array(c[k]).reshape(3, 4) for k in ("P0", "P1", "P2", "P3"))
    fc.r0_rect = np.array(c["R0_rect"]).reshape(3, 3)
    fc.tr_velodyne_to_cam = np.array(c["Tr_velo_to_cam"]).reshape(3, 4)
    scans = [synth.synthetic_scan(np.random.default_rng([seed, f]), n) for f in range(len(shapes))]
    plane = synth.KITTI_PLANE / np.linalg.norm(synth.KITTI_PLANE[:3])
    return kitti.KittiFrames(scans, [fc] * len(shapes), [plane] * len(shapes), shapes), scans, fc, plane


@pytest.mark.parametrize("s", [4, 2], ids=["bucketed", "flat"])
def test_frame_pipeline_velo_step_mixed_image_shapes(s):
    """Synthetic velodyne scans with mixed image_shapes -> loader -> BEV slices -> index -> layer, every frame
    against its own image (FramePipeline(ragged=True)): the oracle chain per frame, and the run with a side
    stream bitwise the sequential one. Stride 4 takes the bucketed step, stride 2 the flat CSRs."""
    from oracle import shpl_oracle as orc
    from sparse_pooling_amd import pipeline
    shapes = [(375, 1242), (370, 1224), (376, 1241), (374, 1238)]
    fr, scans, fc, plane = _scans(shapes)
    assert fr.padded_im_size == rc.PADDED
    sizes = [(w, h) for h, w in shapes]
    stride, C = (s, s), 8
    rect = orc.rect_matrix(fc.r0_rect, fc.tr_velodyne_to_cam)
    refs = []
    for f, size in enumerate(sizes):
        cloud = orc.velo_to_cam(scans[f], rect, fc.p2, list(size))
        hm, dm, vox, upts = orc.bev_slices(cloud, plane, synth.AREA_EXTENTS, synth.VOXEL_SIZE, synth.HEIGHT_LO,
                                           synth.HEIGHT_HI, synth.NUM_SLICES)
        refs.append(rc.oracle_index(upts, vox, fc.p2, size, (hm.shape[1], hm.shape[2]), stride))
        if f == 1:  # this batch tells a frame's own size from the padded one
            assert rc.oracle_index(upts, vox, fc.p2, rc.PADDED, (hm.shape[1], hm.shape[2]),
                                   stride)["Mij_pool"].shape != refs[1]["Mij_pool"].shape
    outs = []
    for side in (None, torch.cuda.Stream()):
        pl = pipeline.FramePipeline(4, fr.total_points, fr.padded_im_size, synth.AREA_EXTENTS, synth.VOXEL_SIZE,
                                    synth.HEIGHT_LO, synth.HEIGHT_HI, synth.NUM_SLICES, stride, C, C, dual=True,
                                    max_points_per_frame=fr.max_points, ragged=True)
        assert pl.buckets == (s == 4)
        bev = synth.make_features((4, pl.Hb, pl.Wb, C), 3)
        img = rc.padded_features(4, pl.Hi, pl.Wi, C, sizes, s, 4)
        tb, ti = torch.from_numpy(bev).to(DEV), torch.from_numpy(img).to(DEV)
        for _ in range(2):  # the second step reuses every workspace
            pl.velo_step(fr, tb, ti, side=side)
        torch.cuda.synchronize()
        assert int(pl.err.item()) == 0 and int(pl.bev.err.item()) == 0
        np.testing.assert_array_equal(_np(pl.im_sizes), np.array(sizes, np.float64))
        outs.append([_np(t).copy() for t in (pl.bv_fused, pl.img_fused, pl.frame_nnz)])
    want = rc.layer_oracle(refs, sizes, s, bev, img)
    for f, (eb, ei, _, _) in enumerate(want):
        assert outs[0][2][f] == refs[f]["Mij_pool"].shape[0] > 0
        np.testing.assert_array_equal(outs[0][0][f:f + 1], eb)
        np.testing.assert_array_equal(outs[0][1][f:f + 1], ei)
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))


# ------------------------------------------------------------------ 5. too-small map and bad sizes

GUARD = 64


def _guarded(n, dtype, fill, width=1):
    """A buffer of n rows with GUARD rows of `fill` on either side: (whole, the view handed to the library)."""
    whole = torch.full(((n + 2 * GUARD) * width,), fill, dtype=dtype, device=DEV)
    return whole, whole[GUARD * width:(GUARD + n) * width]


@pytest.mark.parametrize("buckets", [False, True], ids=["two_launch", "buckets"])
def test_too_small_map_and_bad_sizes(buckets):
    """A frame larger than the padded map: the entries whose strided pixel lies outside it get pix = -1 and set
    SHPL_EBIT_PIXEL, exactly those; a NaN, infinite, zero or negative size keeps nothing. Every output sits in a
    sentinel-filled buffer between guard bands, which no call may touch."""
    from sparse_pooling_amd import _lib as L
    s, stride = 4, (4, 4)
    big = (1242.0, 376.0)
    sizes = [big, (float("nan"), 376.0), (1242.0, 0.0), (-5.0, 376.0), (float("inf"), 376.0), (1242.0, float("inf")),
             (1242.0, float("-inf")), rc.KITTI_SIZES[1]]
    hp, wp = rc.strided(rc.KITTI_SIZES[1], s)  # the map fits 1224 x 370: frame 0 does not
    frames = rc.make_frames([1500] + [200] * 6 + [1100], stride, 400)
    ref0 = rc.oracle_index(frames[0].points, frames[0].voxel_indices, frames[0].P, big, rc.BV_SIZE, stride)
    pts, vox, off, P, maxp, N = _stack(frames)
    B = len(frames)
    i32, i64 = torch.int32, torch.int64
    cell_w, cell = _guarded(N, i32, -7)
    pix_w, pix = _guarded(N, i32, -7)
    val_w, val = _guarded(N, torch.float32, float("nan"))
    mij_w, mij = _guarded(N, i64, -7, 2)
    flip_w, flip = _guarded(N, i64, -7, 3)
    nnz_w, nnz = _guarded(B, i64, -7)
    fo_w, fo = _guarded(B + 1, i64, -7)
    err = torch.zeros(1, dtype=i32, device=DEV)
    ws = L.workspace(L.index_ws_bytes(B, maxp), DEV)
    tsz = _sizes(sizes)
    lead = L.index_args_ragged(B, off, None, maxp, pts, vox, P, tsz, (hp, wp), rc.BV_SIZE, stride, None, cell, pix,
                               val)
    tail = (L.ptr(nnz), L.ptr(fo), L.ptr(err), L.ptr(ws), ws.numel())
    if buckets:
        n_cells = (rc.BV_SIZE[0] // s) * (rc.BV_SIZE[1] // s)
        bws = L.bucket_workspace(B, maxp, N, n_cells, hp * wp, DEV)
        L.check(L.lib().shpl_build_index_buckets_ragged(*lead, *tail, N, L.ptr(bws), bws.numel(), None, None,
                                                        L.stream_of(DEV)), "shpl_build_index_buckets_ragged")
    else:
        L.check(L.lib().shpl_build_index_ragged(*lead, L.ptr(mij), L.ptr(flip), *tail, L.stream_of(DEV)),
                "shpl_build_index_ragged")
    torch.cuda.synchronize()
    assert int(err.item()) & 0xFFFFFFFF == L.EBIT_PIXEL
    for whole, width, n in ((cell_w, 1, N), (pix_w, 1, N), (mij_w, 2, N), (flip_w, 3, N), (nnz_w, 1, B),
                            (fo_w, 1, B + 1)):
        w = _np(whole)
        assert (w[:GUARD * width] == -7).all() and (w[(GUARD + n) * width:] == -7).all()
    w = _np(val_w)
    assert np.isnan(w[:GUARD]).all() and np.isnan(w[GUARD + N:]).all()
    got_nnz, got_off = _np(nnz), _np(fo)
    np.testing.assert_array_equal(got_off, _np(off))
    np.testing.assert_array_equal(got_nnz[1:7], 0)  # the bad sizes keep nothing
    for f in range(1, 7):
        assert (_np(cell[got_off[f]:got_off[f + 1]]) == -1).all() and (_np(pix[got_off[f]:got_off[f + 1]]) == -1).all()
    a, b = got_off[0], got_off[0] + got_nnz[0]
    assert got_nnz[0] == ref0["Mij_pool"].shape[0]
    want_pix = rc.pix_ids(ref0["img_index_flip_pool"], 0, hp, wp)
    outside = (ref0["img_index_flip_pool"][:, 1] >= hp) | (ref0["img_index_flip_pool"][:, 2] >= wp)
    assert 0 < outside.sum() < outside.size and ((want_pix == -1) == outside).all()
    np.testing.assert_array_equal(_np(pix[a:b]), want_pix)
    np.testing.assert_array_equal(_np(cell[a:b]), ref0["Mij_pool"][:, 0])
    last = rc.oracle_index(frames[7].points, frames[7].voxel_indices, frames[7].P, sizes[7], rc.BV_SIZE, stride)
    a, b = got_off[7], got_off[7] + got_nnz[7]
    assert got_nnz[7] == last["Mij_pool"].shape[0]
    np.testing.assert_array_equal(_np(pix[a:b]), rc.pix_ids(last["img_index_flip_pool"], 7, hp, wp))
    assert (_np(pix[a:b]) >= 0).all()
    if not buckets:
        np.testing.assert_array_equal(_np(flip).reshape(-1, 3)[got_off[0]:got_off[0] + got_nnz[0]],
                                      ref0["img_index_flip_pool"])  # flip keeps the frame's own (v', u')


# ------------------------------------------------------------------ 6. a uniform batch

@pytest.mark.parametrize("s", [1, 8])
def test_uniform_sizes_equal_the_uniform_entry(s):
    """Ragged with every size equal is bitwise the existing entry point on the same batch: the index arrays, and
    (stride 8, bucketed pipelines) the layer."""
    from sparse_pooling_amd import pipeline, shpl_map as sm
    stride = (s, s)
    size = rc.KITTI_SIZES[1]
    spec = synth.FrameSpec(0, size, rc.BV_SIZE, stride)
    frames = [synth.make_frame(synth.FrameSpec(n, size, rc.BV_SIZE, stride), 500 + f, n_outside=11 * f)
              for f, n in enumerate([2049, 1, 1024, 300])]
    pts, vox, off, P, maxp, N = _stack(frames)
    a = sm.build_index_batch(pts, vox, off, P, size, rc.BV_SIZE, stride, maxp, ref_outputs=True)
    b = sm.build_index_batch(pts, vox, off, P, size, rc.BV_SIZE, stride, maxp, ref_outputs=True,
                             im_sizes=_sizes([size] * 4))
    assert a.img_hw == b.img_hw == spec.img_feat_hw
    fo, fn = _np(a.frame_off), _np(a.frame_nnz)
    np.testing.assert_array_equal(_np(b.frame_off), fo)
    np.testing.assert_array_equal(_np(b.frame_nnz), fn)
    for x, y in ((a.map.cell, b.map.cell), (a.map.pix, b.map.pix), (a.map.val, b.map.val)):
        np.testing.assert_array_equal(_np(x).view(np.uint8), _np(y).view(np.uint8))
    for f in range(4):  # mij / flip are written for the live entries
        for x, y in ((a.mij, b.mij), (a.flip, b.flip)):
            np.testing.assert_array_equal(_np(x[fo[f]:fo[f] + fn[f]]), _np(y[fo[f]:fo[f] + fn[f]]))
    assert a.map.error_bits() == 0 and b.map.error_bits() == 0
    if s != 8:
        return
    C = 8
    outs = []
    for ragged in (False, True):
        pl = pipeline.FusedPipeline(4, maxp, N, size, rc.BV_SIZE, stride, C, C, dual=True, rows=True, buckets=True,
                                    ragged=ragged)
        bev = torch.from_numpy(synth.make_features((4, pl.Hb, pl.Wb, C), 1)).to(DEV)
        img = torch.from_numpy(synth.make_features((4, pl.Hi, pl.Wi, C), 2)).to(DEV)
        pl.step_overlapped(pts, vox, off, P, bev, img, None)
        torch.cuda.synchronize()
        assert int(pl.err.item()) == 0
        outs.append([_np(t).copy() for t in (pl.cell, pl.pix, pl.val, pl.frame_nnz, pl.bv_fused, pl.img_fused)])
    for x, y in zip(*outs):
        np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8))
