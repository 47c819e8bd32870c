"""The index build for several fusion levels in one pass (shpl_build_index_levels and everything above it) on
MI355X, against shpl_build_index called once per level -- bitwise, over the whole capacity of every array -- and
against the oracle per frame and level (tests/levels_cases.py; pinned to a reference run by
tests/test_oracle_levels_golden.py). shpl_build_index is the comparator because this work leaves it unchanged
and the existing suite pins it to the reference goldens.

The batch (chunks are 1024 points): frame 0 2107 points (three chunks), frame 1 1030 points with a voxel of
z = 700 at points 0, 1023, 1024 and 1029 (kept at stride 8 over 704 rows, dropped at stride 1 over 700), frame 2
empty, frame 3 one clip survivor among points outside the image -- the single_tie point, whose rounded u depends
on the order of the second projection's products."""
import functools
import os

import numpy as np
import pytest
import torch

import levels_cases as lc
import ragged_cases as rc
from sparse_pooling_amd import synth

pytestmark = pytest.mark.gpu

DEV = "cuda"
GOLD = os.path.join(os.path.dirname(__file__), "golden")
CHUNK = 1024
I32_FILL, I64_FILL = -7, -7
F32_FILL = float("nan")


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ------------------------------------------------------------------ the batch and its oracle

@functools.lru_cache(maxsize=None)
def _frames():
    f0 = synth.make_frame(synth.FrameSpec(2100, lc.IM_SIZE, (704, 800), (1, 1)), 3000, n_outside=7)
    f1 = synth.make_frame(synth.FrameSpec(1030, lc.IM_SIZE, (704, 800), (1, 1)), 3001)
    for k, i in enumerate((0, 1023, 1024, 1029)):
        f1.voxel_indices[i] = (50 + k, 700)
    f2 = synth.make_frame(synth.FrameSpec(0, lc.IM_SIZE, (704, 800), (1, 1)), 3002)
    out = synth.make_frame(synth.FrameSpec(0, lc.IM_SIZE, (704, 800), (1, 1)), 3003, n_outside=9)
    tie = np.load(os.path.join(GOLD, "index_single_tie.npz"))["points"].reshape(-1, 3)[:1]
    pts = np.concatenate([out.points[:4], tie, out.points[4:]])
    vox = np.concatenate([out.voxel_indices[:4], [[300, 400]], out.voxel_indices[4:]]).astype(np.int64)
    f3 = synth.Frame(pts, vox, synth.KITTI_P2, out.spec)
    frames = [f0, f1, f2, f3]
    assert [f.points.shape[0] for f in frames] == [2107, 1030, 0, 10]
    return frames


@functools.lru_cache(maxsize=None)
def _refs(name, pdt):
    """refs[f][l]: the oracle's outputs for frame f at level l, the points as the device reads them."""
    npdt = np.float64 if pdt == "f64" else np.float32
    return [lc.oracle_levels(fr.points.astype(npdt).astype(np.float64), fr.voxel_indices, fr.P, lc.SETS[name])
            for fr in _frames()]


@functools.lru_cache(maxsize=None)
def _preconditions(pdt):
    """What makes the batch a test of per-level compaction, asserted from the oracle before any GPU result is
    compared: the pair's nnz differ in frames 0 and 1, a point only one level keeps lies in the first chunk of a
    multi-chunk frame (every later slot of that level shifts), and frame 3 has one survivor whose u the product
    order decides."""
    frames, refs = _frames(), _refs("pair", pdt)
    for f in (0, 1):
        assert refs[f][0]["M_size"][1] != refs[f][1]["M_size"][1]
    assert (refs[0][0]["M_size"][1], refs[0][1]["M_size"][1]) == (2087, 2098)
    for f in (0, 1):
        fr = frames[f]
        assert fr.points.shape[0] > CHUNK
        inside = synth._clip_mask(fr.points[:CHUNK], fr.P, lc.IM_SIZE)
        z = fr.voxel_indices[:CHUNK, 1]
        assert (inside & (z >= 700) & (z < 704)).sum() >= 1  # kept at stride 8 over 704 rows only
    assert [r["M_size"][1] for r in refs[3]] == [1, 1]
    if pdt == "f64":  # among several survivors the same point rounds u the other way (dgemm's order)
        extra = frames[0].points[:1]
        two = rc.oracle_index(np.concatenate([frames[3].points, extra]),
                              np.concatenate([frames[3].voxel_indices, [[1, 1]]]), synth.KITTI_P2, lc.IM_SIZE,
                              (700, 800), (1, 1))
        row = np.flatnonzero(two["Mij_pool"][:, 0] == refs[3][0]["Mij_pool"][0, 0])
        assert row.size == 1 and two["img_index_flip_pool"][row[0], 2] != refs[3][0]["img_index_flip_pool"][0, 2]
    return True


def _stack(frames=None, pdt="f64", vit="i64"):
    from sparse_pooling_amd import pipeline
    pts, vox, off, P, maxp, N = pipeline.stack_frames(frames or _frames(), DEV)
    return (pts.to(torch.float64 if pdt == "f64" else torch.float32),
            vox.to(torch.int64 if vit == "i64" else torch.int32), off, P, maxp, N)


# ------------------------------------------------------------------ the C ABI over sentinel-filled arrays

class Outs:
    """One level's output arrays over N slots, filled with a sentinel pattern."""

    def __init__(self, N, B, ref_outputs=True):
        self.cell = torch.full((N,), I32_FILL, dtype=torch.int32, device=DEV)
        self.pix = torch.full((N,), I32_FILL, dtype=torch.int32, device=DEV)
        self.val = torch.full((N,), F32_FILL, dtype=torch.float32, device=DEV)
        self.mij = torch.full((N, 2), I64_FILL, dtype=torch.int64, device=DEV) if ref_outputs else None
        self.flip = torch.full((N, 3), I64_FILL, dtype=torch.int64, device=DEV) if ref_outputs else None
        self.nnz = torch.full((B,), I64_FILL, dtype=torch.int64, device=DEV)

    def arrays(self):
        return [(k, getattr(self, k)) for k in ("cell", "pix", "val", "mij", "flip", "nnz")
                if getattr(self, k) is not None]

    def untouched(self):
        for k, t in self.arrays():
            a = _np(t)
            if not (np.isnan(a).all() if k == "val" else (a == I32_FILL).all()):
                return False
        return True


def _levels_call(batch, levels, outs, counts=None, mval=None, maxp=None, n_levels=None):
    """shpl_build_index_levels: (status, err bits, frame_out_off)."""
    from sparse_pooling_amd import _lib as L
    pts, vox, off, P, maxp0, N = batch
    maxp = maxp0 if maxp is None else maxp
    B = off.numel() - 1
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    fo = torch.full((B + 1,), I64_FILL, dtype=torch.int64, device=DEV)
    ws = L.workspace(L.index_levels_ws_bytes(B, maxp, min(max(len(levels), 1), L.MAX_INDEX_LEVELS)), DEV)
    arr = L.index_levels([(s, b, o.cell, o.pix, o.val, o.mij, o.flip, o.nnz) for (s, b), o in zip(levels, outs)])
    lead = L.index_args(B, off, counts, maxp, pts, vox, P, lc.IM_SIZE, (0, 0), (1, 1), mval, None, None, None)
    rc_ = L.lib().shpl_build_index_levels(*lead[:12], lead[16], len(levels) if n_levels is None else n_levels, arr,
                                          L.ptr(fo), L.ptr(err), L.ptr(ws), ws.numel(), L.stream_of(DEV))
    torch.cuda.synchronize()
    return rc_, int(err.item()) & 0xFFFFFFFF, _np(fo)


def _single_call(batch, level, out, counts=None, mval=None, maxp=None):
    """shpl_build_index at one level's arguments: (err bits, frame_out_off)."""
    from sparse_pooling_amd import _lib as L
    pts, vox, off, P, maxp0, N = batch
    maxp = maxp0 if maxp is None else maxp
    B = off.numel() - 1
    stride, bv_size = level
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    fo = torch.full((B + 1,), I64_FILL, dtype=torch.int64, device=DEV)
    ws = L.workspace(L.index_ws_bytes(B, maxp), DEV)
    lead = L.index_args(B, off, counts, maxp, pts, vox, P, lc.IM_SIZE, bv_size, stride, mval, out.cell, out.pix,
                        out.val)
    L.check(L.lib().shpl_build_index(*lead, L.ptr(out.mij), L.ptr(out.flip), L.ptr(out.nnz), L.ptr(fo), L.ptr(err),
                                     L.ptr(ws), ws.numel(), L.stream_of(DEV)), "shpl_build_index")
    torch.cuda.synchronize()
    return int(err.item()) & 0xFFFFFFFF, _np(fo)


def _assert_same(got, want, what):
    for (k, a), (k2, b) in zip(got.arrays(), want.arrays()):
        assert k == k2
        np.testing.assert_array_equal(_bits(_np(a)), _bits(_np(b)), err_msg=f"{what}: {k}")


def _against_singles(batch, levels, ref_outputs=True, **kw):
    """The levels call over sentinel-filled arrays against one shpl_build_index call per level, bit for bit over the
    whole capacity; returns the levels call's outputs and error bits."""
    from sparse_pooling_amd import _lib as L
    N, B = batch[5], batch[2].numel() - 1
    outs = [Outs(N, B, ref_outputs) for _ in levels]
    rc_, bits, fo = _levels_call(batch, levels, outs, **kw)
    assert rc_ == L.OK
    np.testing.assert_array_equal(fo, _np(batch[2]))
    want_bits = 0
    for l, level in enumerate(levels):
        one = Outs(N, B, ref_outputs)
        b1, fo1 = _single_call(batch, level, one, **kw)
        np.testing.assert_array_equal(fo1, fo)
        _assert_same(outs[l], one, f"level {l} {level}")
        want_bits |= b1
    assert bits == want_bits
    return outs, bits


# ------------------------------------------------------------------ 1. the two sets, every type pair

@pytest.mark.parametrize("vit", ["i64", "i32"])
@pytest.mark.parametrize("pdt", ["f64", "f32"])
@pytest.mark.parametrize("name", ["pair", "pyramid"])
def test_levels_equal_single_calls_and_oracle(name, pdt, vit):
    assert _preconditions(pdt)
    levels, refs = lc.SETS[name], _refs(name, pdt)
    batch = _stack(pdt=pdt, vit=vit)
    outs, bits = _against_singles(batch, levels)
    assert bits == 0
    off = _np(batch[2])
    for l, (stride, bv_size) in enumerate(levels):
        nnz = _np(outs[l].nnz)
        hq, wq = rc.strided(lc.IM_SIZE, stride[0])
        for f in range(4):
            ref = refs[f][l]
            a, b = off[f], off[f] + nnz[f]
            assert nnz[f] == ref["M_size"][1] == ref["Mij_pool"].shape[0], (l, f)
            np.testing.assert_array_equal(_np(outs[l].mij[a:b]), ref["Mij_pool"])
            np.testing.assert_array_equal(_np(outs[l].flip[a:b]), ref["img_index_flip_pool"])
            np.testing.assert_array_equal(_np(outs[l].cell[a:b]), ref["Mij_pool"][:, 0] + f * int(ref["M_size"][0]))
            np.testing.assert_array_equal(_np(outs[l].pix[a:b]), rc.pix_ids(ref["img_index_flip_pool"], f, hq, wq))
            assert (_np(outs[l].cell[b:off[f + 1]]) == -1).all() and (_np(outs[l].pix[b:off[f + 1]]) == -1).all()


@pytest.mark.parametrize("name", ["pair", "pyramid"])
def test_build_index_levels_matches_oracle(name):
    """shpl_map.build_index_levels: one IndexBatch per level with ref_outputs, the maps sharing one err tensor."""
    from sparse_pooling_amd import shpl_map as sm
    assert _preconditions("f64")
    levels, refs = lc.SETS[name], _refs(name, "f64")
    pts, vox, off, P, maxp, N = _stack()
    ibs = sm.build_index_levels(pts, vox, off, P, lc.IM_SIZE, levels, maxp, ref_outputs=True)
    assert len(ibs) == len(levels)
    for l, ((stride, bv_size), ib) in enumerate(zip(levels, ibs)):
        assert ib.map.err is ibs[0].map.err and ib.frame_off is ibs[0].frame_off
        assert ib.bev_hw == (bv_size[0] // stride[1], bv_size[1] // stride[1])
        assert ib.img_hw == rc.strided(lc.IM_SIZE, stride[0])
        assert ib.map.n_cells == 4 * ib.bev_hw[0] * ib.bev_hw[1] and ib.map.n_pix == 4 * ib.img_hw[0] * ib.img_hw[1]
        fo, fn = _np(ib.frame_off), _np(ib.frame_nnz)
        np.testing.assert_array_equal(fo, _np(off))
        for f in range(4):
            ref = refs[f][l]
            assert fn[f] == ref["M_size"][1]
            np.testing.assert_array_equal(_np(ib.mij[fo[f]:fo[f] + fn[f]]), ref["Mij_pool"])
            np.testing.assert_array_equal(_np(ib.flip[fo[f]:fo[f] + fn[f]]), ref["img_index_flip_pool"])
    assert ibs[0].map.error_bits() == 0


# ------------------------------------------------------------------ 2. one level, identical levels

def test_one_level_equals_build_index():
    for level in (lc.PAIR[0], lc.PAIR[1], ((3, 5), (704, 800))):
        _against_singles(_stack(), [level])


def test_two_identical_levels_give_identical_arrays():
    outs, bits = _against_singles(_stack(), [lc.PAIR[1], lc.PAIR[1]])
    _assert_same(outs[0], outs[1], "identical levels")
    assert bits == 0


# ------------------------------------------------------------------ 3. counts, weights, optional outputs

def test_point_counts_mval_and_one_level_without_ref_outputs():
    """The capacity layout (d_point_counts: slots past a frame's count are dead), a weight per input point, and
    mij / flip absent for one level only."""
    from sparse_pooling_amd import _lib as L
    pts, vox, off, P, maxp, N = _stack()
    counts = torch.tensor([2000, 1025, 0, 10], dtype=torch.int64, device=DEV)  # frame 0 and 1 shortened
    mval = torch.from_numpy(synth.make_features((N,), 7)).to(DEV)
    batch = (pts, vox, off, P, maxp, N)
    outs, bits = _against_singles(batch, lc.PAIR, counts=counts, mval=mval)
    assert bits == 0
    nnz = _np(outs[0].nnz)
    ref = lc.oracle_levels(_frames()[0].points[:2000], _frames()[0].voxel_indices[:2000], synth.KITTI_P2, lc.PAIR)
    assert [int(_np(o.nnz)[0]) for o in outs] == [r["M_size"][1] for r in ref] and nnz[2] == 0
    # the values follow their points through each level's own compaction
    inside = synth._clip_mask(_frames()[0].points[:2000], synth.KITTI_P2, lc.IM_SIZE)
    z = _frames()[0].voxel_indices[:2000, 1]
    for o, rows in zip(outs, (700, 704)):
        np.testing.assert_array_equal(_np(o.val[:int(_np(o.nnz)[0])]), _np(mval[:2000])[inside & (z < rows)])
    # level 1 without mij / flip: every other array as before, level 0's mij / flip too
    mixed = [Outs(N, 4), Outs(N, 4, ref_outputs=False)]
    rc_, bits, _ = _levels_call(batch, lc.PAIR, mixed, counts=counts, mval=mval)
    assert rc_ == L.OK and bits == 0
    _assert_same(mixed[0], outs[0], "level 0")
    for k in ("cell", "pix", "val", "nnz"):
        np.testing.assert_array_equal(_bits(_np(getattr(mixed[1], k))), _bits(_np(getattr(outs[1], k))))


# ------------------------------------------------------------------ 4. the error word

def test_negative_voxel_sets_the_row_bit_in_the_shared_word():
    """A negative voxel index flattens below zero at every level here: the reference keeps the entry (r < n_cells),
    so every level writes cell = -1 and the shared word gets SHPL_EBIT_ROW -- as each single call reports."""
    from sparse_pooling_amd import _lib as L
    frames = list(_frames())
    f1 = synth.Frame(frames[1].points, frames[1].voxel_indices.copy(), frames[1].P, frames[1].spec)
    f1.voxel_indices[5] = (3, -9)
    frames[1] = f1
    batch = _stack(frames)
    outs, bits = _against_singles(batch, lc.PAIR)
    assert bits == L.EBIT_ROW
    off = _np(batch[2])
    refs = lc.oracle_levels(f1.points, f1.voxel_indices, f1.P, lc.PAIR)
    for o, ref in zip(outs, refs):
        neg = np.flatnonzero(ref["Mij_pool"][:, 0] < 0)
        assert neg.size == 1
        cell = _np(o.cell[off[1]:off[1] + ref["M_size"][1]])
        assert cell[neg[0]] == -1 and (np.delete(cell, neg[0]) >= 0).all()
        np.testing.assert_array_equal(_np(o.mij[off[1]:off[1] + ref["M_size"][1]]), ref["Mij_pool"])


def test_frame_over_max_points_sets_capacity():
    from sparse_pooling_amd import _lib as L
    batch = _stack()
    outs, bits = _against_singles(batch, lc.PAIR, maxp=2048)  # frame 0 holds 2107 points: two chunks do not cover it
    assert bits == L.EBIT_CAPACITY


def test_refused_call_writes_nothing():
    from sparse_pooling_amd import _lib as L
    batch = _stack()
    N = batch[5]
    for levels, n_levels, want in (([lc.PAIR[0], ((0, 8), (704, 800))], None, L.ERR_BAD_SHAPE),
                                   ([lc.PAIR[0], ((8, 8), (-704, 800))], None, L.ERR_BAD_SHAPE),
                                   (lc.PAIR * 2 + lc.PAIR[:1], None, L.ERR_BAD_SHAPE), (lc.PAIR, 0, L.ERR_BAD_SHAPE)):
        outs = [Outs(N, 4) for _ in levels]
        rc_, bits, fo = _levels_call(batch, levels, outs, n_levels=n_levels)
        assert rc_ == want and bits == 0 and (fo == I64_FILL).all()
        assert all(o.untouched() for o in outs)
    outs = [Outs(N, 4), Outs(N, 4)]
    outs[1].pix = None
    rc_, bits, fo = _levels_call(batch, lc.PAIR, outs)
    assert rc_ == L.ERR_ARG and (fo == I64_FILL).all() and all(o.untouched() for o in outs)


# ------------------------------------------------------------------ 5. the reference fixture as a batch

@pytest.mark.parametrize("name", ["pair", "pyramid"])
def test_fixture_batch_equals_reference_arrays(name):
    from sparse_pooling_amd import shpl_map as sm
    g = lc.golden()
    spec = synth.FrameSpec(0, lc.IM_SIZE, (704, 800), (1, 1))
    frames = [synth.Frame(g[f"points_{f}"], g[f"voxels_{f}"], g["P"], spec) for f in range(3)]
    pts, vox, off, P, maxp, N = _stack(frames)
    levels = lc.golden_levels(g, name)
    ibs = sm.build_index_levels(pts, vox, off, P, tuple(g["im_size"]), levels, maxp, ref_outputs=True)
    for l, ib in enumerate(ibs):
        fo, fn = _np(ib.frame_off), _np(ib.frame_nnz)
        for f in range(3):
            assert fn[f] == g[f"{name}_msize_{l}_{f}"][1]
            assert ib.bev_hw[0] * ib.bev_hw[1] == g[f"{name}_msize_{l}_{f}"][0]
            np.testing.assert_array_equal(_np(ib.mij[fo[f]:fo[f] + fn[f]]), g[f"{name}_mij_{l}_{f}"].reshape(-1, 2))
            np.testing.assert_array_equal(_np(ib.flip[fo[f]:fo[f] + fn[f]]), g[f"{name}_flip_{l}_{f}"].reshape(-1, 3))
    assert ibs[0].map.error_bits() == 0


# ------------------------------------------------------------------ 6. chained: CSR and pulls per level

def test_each_level_map_through_csr_and_pulls():
    """Every level's IndexBatch.map through shpl_build_csr and shpl_pull, both directions, 8 channels: bitwise the
    pulls over the map of the single-level call."""
    from sparse_pooling_amd import shpl_map as sm
    pts, vox, off, P, maxp, N = _stack()
    ibs = sm.build_index_levels(pts, vox, off, P, lc.IM_SIZE, lc.PAIR, maxp)
    C = 8
    for (stride, bv_size), ib in zip(lc.PAIR, ibs):
        one = sm.build_index_batch(pts, vox, off, P, lc.IM_SIZE, bv_size, stride, maxp)
        assert (ib.bev_hw, ib.img_hw) == (one.bev_hw, one.img_hw)
        (Hb, Wb), (Hi, Wi) = ib.bev_hw, ib.img_hw
        gen = torch.Generator(device=DEV).manual_seed(11)  # (drawn on the device: the stride-1 BEV map is 72 MB)
        img = torch.randn((4, Hi, Wi, C), generator=gen, device=DEV)
        bev = torch.randn((4, Hb, Wb, C), generator=gen, device=DEV)
        for smap in (ib.map, one.map):
            assert smap.error_bits() == 0
        got = (sm.pool_img_to_bev(ib.map, img, (4, Hb, Wb)), sm.pool_bev_to_img(ib.map, bev, (4, Hi, Wi)))
        want = (sm.pool_img_to_bev(one.map, img, (4, Hb, Wb)), sm.pool_bev_to_img(one.map, bev, (4, Hi, Wi)))
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert a.shape == b.shape and float(b.abs().sum()) > 0
            np.testing.assert_array_equal(_bits(_np(a)), _bits(_np(b)))


# ------------------------------------------------------------------ 7. the reference's list of dicts

def test_build_sparse_pooling_inputs_equals_per_level_calls():
    from sparse_pooling_amd import config as C, sparse_pool_utils as spu
    fr = _frames()[0]
    calib = synth.StereoCalib(fr.P)
    sps = spu.build_sparse_pooling_inputs(fr.points, fr.voxel_indices, calib, list(lc.IM_SIZE), lc.PAIR)
    assert len(sps) == 2
    for sp, (stride, bv_size) in zip(sps, lc.PAIR):
        one = spu.build_sparse_pooling_input(fr.points, fr.voxel_indices, calib, list(lc.IM_SIZE), bv_size,
                                             stride=stride)
        assert set(sp) == set(one)
        for k in one:
            a, b = sp[k], one[k]
            if isinstance(b, torch.Tensor):
                assert a.dtype == b.dtype and a.shape == b.shape
                a, b = _np(a), _np(b)
            else:
                assert np.asarray(a).dtype == np.asarray(b).dtype
            np.testing.assert_array_equal(a, b, err_msg=k)
    feed = C.fill_sparse_pooling_feed({}, sps, True, after_vgg=True, use_after_vgg=True)
    assert feed[C.PL_M_SIZE][1] == 2087 and feed[C.PL_M_SIZE_VGG][1] == 2098
