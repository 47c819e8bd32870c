"""The index build for several fusion levels over a batch of mixed image sizes (shpl_build_index_levels_ragged
and shpl_map.build_index_levels(im_sizes=)) on MI355X, against shpl_build_index_ragged called once per level --
bitwise, over the whole capacity of every array -- and against the oracle per frame and level at the frame's OWN
image size (tests/levels_ragged_cases.py; pinned to a reference run by tests/test_oracle_levels_ragged_golden.py).
shpl_build_index_ragged is the comparator because this work leaves it unchanged and the existing suite pins it.

The base batch (chunks are 1024 points): five frames of 2107 / 1030 / 307 / 7 / 307 points at 1224x370, 1238x374,
620x188, 1241x376 and 1242x375, drawn inside the padded 1242x376; every level has one padded image feature map,
floor((376, 1242) / s_img)."""
import functools
import os

import numpy as np
import pytest
import torch

import levels_cases as lc
import levels_ragged_cases as lrc
import ragged_cases as rc
from sparse_pooling_amd import synth

pytestmark = pytest.mark.gpu

DEV = "cuda"
GOLD = os.path.join(os.path.dirname(__file__), "golden")
FILL = -7
GUARD = 64


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _sizes(sizes):
    return torch.tensor([[float(w), float(h)] for w, h in sizes], dtype=torch.float64, device=DEV)


@functools.lru_cache(maxsize=None)
def _pre(name, pdt="f64"):
    """The oracle's preconditions on the base batch (asserted before any GPU result is compared) and its refs."""
    refs, clamped = lrc.base_preconditions(name, np.float64 if pdt == "f64" else np.float32)
    return refs


def _stack(frames=None, pdt="f64", vit="i64"):
    from sparse_pooling_amd import pipeline
    pts, vox, off, P, maxp, N = pipeline.stack_frames(frames or lrc.base_frames(), DEV)
    return (pts.to(torch.float64 if pdt == "f64" else torch.float32),
            vox.to(torch.int64 if vit == "i64" else torch.int32), off, P, maxp, N)


# ------------------------------------------------------------------ the C ABI over sentinel-filled arrays

def _guarded(n, dtype, fill, width=1):
    """n rows between GUARD rows of `fill` on either side: (whole, the view handed to the library)."""
    whole = torch.full(((n + 2 * GUARD) * width,), fill, dtype=dtype, device=DEV)
    view = whole[GUARD * width:(GUARD + n) * width]
    return whole, view if width == 1 else view.view(n, width)


class Outs:
    """One level's output arrays over N slots, filled with a sentinel pattern, each between guard bands."""
    KINDS = (("cell", torch.int32, FILL, 1), ("pix", torch.int32, FILL, 1), ("val", torch.float32, float("nan"), 1),
             ("mij", torch.int64, FILL, 2), ("flip", torch.int64, FILL, 3), ("nnz", torch.int64, FILL, 1))

    def __init__(self, N, B, ref_outputs=True):
        self.whole = {}
        for k, dt, fill, width in self.KINDS:
            if k in ("mij", "flip") and not ref_outputs:
                setattr(self, k, None)
                continue
            self.whole[k], view = _guarded(B if k == "nnz" else N, dt, fill, width)
            setattr(self, k, view)

    def arrays(self):
        return [(k, getattr(self, k)) for k, *_ in self.KINDS if getattr(self, k) is not None]

    def untouched(self):
        return all(np.isnan(_np(t)).all() if k == "val" else (_np(t) == FILL).all() for k, t in self.arrays())

    def guards_intact(self):
        for k, _, _, width in self.KINDS:
            if k not in self.whole:
                continue
            w, g = _np(self.whole[k]), GUARD * width
            for band in (w[:g], w[w.size - g:]):
                if not (np.isnan(band).all() if k == "val" else (band == FILL).all()):
                    return False
        return True


def _levels_call(batch, sizes, levels, maps, outs, counts=None, mval=None, n_levels=None):
    """shpl_build_index_levels_ragged: (status, err bits, frame_out_off)."""
    from sparse_pooling_amd import _lib as L
    pts, vox, off, P, maxp, N = batch
    B = off.numel() - 1
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    fo = torch.full((B + 1,), FILL, dtype=torch.int64, device=DEV)
    ws = L.workspace(L.index_levels_ws_bytes(B, maxp, min(max(len(levels), 1), L.MAX_INDEX_LEVELS)), DEV)
    arr = L.index_levels([(s, b, o.cell, o.pix, o.val, o.mij, o.flip, o.nnz) for (s, b), o in zip(levels, outs)])
    lead = L.index_args(B, off, counts, maxp, pts, vox, P, (0, 0), (0, 0), (1, 1), mval, None, None, None)
    tsz = None if sizes is None else sizes if isinstance(sizes, torch.Tensor) else _sizes(sizes)
    hw = None if maps is None else L.index_level_maps(maps)
    rc_ = L.lib().shpl_build_index_levels_ragged(*lead[:10], L.ptr(tsz), lead[16],
                                                 len(levels) if n_levels is None else n_levels, arr, hw, L.ptr(fo),
                                                 L.ptr(err), L.ptr(ws), ws.numel(), L.stream_of(DEV))
    torch.cuda.synchronize()
    return rc_, int(err.item()) & 0xFFFFFFFF, _np(fo)


def _single_call(batch, sizes, level, map_hw, out, counts=None, mval=None):
    """shpl_build_index_ragged at one level's arguments: (err bits, frame_out_off)."""
    from sparse_pooling_amd import _lib as L
    pts, vox, off, P, maxp, N = batch
    B = off.numel() - 1
    stride, bv_size = level
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    fo = torch.full((B + 1,), FILL, dtype=torch.int64, device=DEV)
    ws = L.workspace(L.index_ws_bytes(B, maxp), DEV)
    tsz = sizes if isinstance(sizes, torch.Tensor) else _sizes(sizes)
    lead = L.index_args_ragged(B, off, counts, maxp, pts, vox, P, tsz, map_hw, bv_size, stride, mval, out.cell,
                               out.pix, out.val)
    L.check(L.lib().shpl_build_index_ragged(*lead, L.ptr(out.mij), L.ptr(out.flip), L.ptr(out.nnz), L.ptr(fo),
                                            L.ptr(err), L.ptr(ws), ws.numel(), L.stream_of(DEV)),
            "shpl_build_index_ragged")
    torch.cuda.synchronize()
    return int(err.item()) & 0xFFFFFFFF, _np(fo)


def _assert_same(got, want, what):
    for (k, a), (k2, b) in zip(got.arrays(), want.arrays()):
        assert k == k2
        np.testing.assert_array_equal(_bits(_np(a)), _bits(_np(b)), err_msg=f"{what}: {k}")


def _against_singles(batch, sizes, levels, maps=None, ref_outputs=True, **kw):
    """The ragged levels call over sentinel-filled arrays against one shpl_build_index_ragged call per level, bit
    for bit over the whole capacity; returns the levels call's outputs, its error bits and each single call's."""
    from sparse_pooling_amd import _lib as L
    maps = lrc.level_maps(levels) if maps is None else maps
    N, B = batch[5], batch[2].numel() - 1
    outs = [Outs(N, B, ref_outputs) for _ in levels]
    rc_, bits, fo = _levels_call(batch, sizes, levels, maps, outs, **kw)
    assert rc_ == L.OK
    np.testing.assert_array_equal(fo, _np(batch[2]))
    each = []
    for l, level in enumerate(levels):
        one = Outs(N, B, ref_outputs)
        b1, fo1 = _single_call(batch, sizes, level, maps[l], one, **kw)
        np.testing.assert_array_equal(fo1, fo)
        _assert_same(outs[l], one, f"level {l} {level}")
        assert outs[l].guards_intact()
        each.append(b1)
    assert bits == functools.reduce(lambda a, b: a | b, each, 0)
    return outs, bits, each


def _assert_oracle(outs, levels, maps, refs, off):
    """Per level and frame: nnz, mij, flip, cell, pix (the padded pitch) and the holes against the oracle."""
    for l in range(len(levels)):
        nnz = _np(outs[l].nnz)
        hp, wp = maps[l]
        for f in range(len(refs)):
            ref = refs[f][l]
            a, b = off[f], off[f] + nnz[f]
            assert nnz[f] == ref["M_size"][1] == ref["Mij_pool"].shape[0], (l, f)
            np.testing.assert_array_equal(_np(outs[l].mij[a:b]), ref["Mij_pool"])
            np.testing.assert_array_equal(_np(outs[l].flip[a:b]), ref["img_index_flip_pool"])
            np.testing.assert_array_equal(_np(outs[l].cell[a:b]), ref["Mij_pool"][:, 0] + f * int(ref["M_size"][0]))
            np.testing.assert_array_equal(_np(outs[l].pix[a:b]), rc.pix_ids(ref["img_index_flip_pool"], f, hp, wp))
            assert (_np(outs[l].cell[b:off[f + 1]]) == -1).all() and (_np(outs[l].pix[b:off[f + 1]]) == -1).all()


# ------------------------------------------------------------------ 1. the two sets, every type pair

@pytest.mark.parametrize("vit", ["i64", "i32"])
@pytest.mark.parametrize("pdt", ["f64", "f32"])
@pytest.mark.parametrize("name", ["pair", "pyramid"])
def test_levels_ragged_equal_single_calls_and_oracle(name, pdt, vit):
    refs = _pre(name, pdt)
    levels, maps = lrc.SETS[name], lrc.level_maps(lrc.SETS[name])
    batch = _stack(pdt=pdt, vit=vit)
    outs, bits, _ = _against_singles(batch, lrc.BASE_SIZES, levels)
    assert bits == 0
    _assert_oracle(outs, levels, maps, refs, _np(batch[2]))


# ------------------------------------------------------------------ 2. the survivor-count edge

def test_one_survivor_at_own_size_selects_the_order_for_all_levels():
    """test_gpu_ragged_index.py's one-survivor frame (its own width leaves ONE clip survivor, the single_tie
    point, whose u rounds differently in dgemv's order) as one frame of a two-frame batch at the pair: the frame's
    own clip count selects the order, and the stride-1 level shows the own-count rounding."""
    _pre("pair")
    tie = np.load(os.path.join(GOLD, "index_single_tie.npz"))["points"].reshape(-1, 3)[:1]
    base = rc.make_frames([40], (1, 1), 900)[0]

    def u_of(p):
        uvw = synth.KITTI_P2 @ np.vstack((p.T, np.ones(p.shape[0])))
        return uvw[0] / uvw[2]
    u_tie = float(u_of(tie)[0])
    keep = u_of(base.points) > u_tie + 5  # every other point projects right of the survivor
    pts = np.concatenate([base.points[keep][:9], tie, base.points[keep][9:]])
    vox = np.concatenate([base.voxel_indices[keep][:9], [[300, 400]], base.voxel_indices[keep][9:]]).astype(np.int64)
    us = np.sort(u_of(pts))
    assert us[1] > u_tie + 5 and abs(us[0] - u_tie) < 1e-9
    own = ((us[0] + us[1]) / 2 + 1.0, 376.0)  # u < W - 1 holds for the smallest u alone
    edge = synth.Frame(pts, vox, synth.KITTI_P2, base.spec)
    other = rc.make_frames([50], (1, 1), 901)[0]
    frames, sizes = [other, edge], [rc.KITTI_SIZES[2], own]
    refs = [lrc.oracle_levels(fr.points, fr.voxel_indices, fr.P, lc.PAIR, size) for fr, size in zip(frames, sizes)]
    assert [r["Mij_pool"].shape[0] for r in refs[1]] == [1, 1]
    at_padded = lrc.oracle_levels(pts, vox, synth.KITTI_P2, lc.PAIR, rc.PADDED)[0]
    assert at_padded["Mij_pool"].shape[0] > 5
    row = np.flatnonzero(at_padded["Mij_pool"][:, 0] == refs[1][0]["Mij_pool"][0, 0])
    assert row.size == 1
    u_own = int(refs[1][0]["img_index_flip_pool"][0, 2])
    assert at_padded["img_index_flip_pool"][row[0], 2] != u_own  # the other order rounds u the other way
    batch = _stack(frames)
    outs, bits, _ = _against_singles(batch, sizes, lc.PAIR)
    assert bits == 0
    off = _np(batch[2])
    _assert_oracle(outs, lc.PAIR, lrc.level_maps(lc.PAIR), refs, off)
    assert int(_np(outs[0].flip[off[1]])[2]) == u_own  # stride 1: the rounded u itself


# ------------------------------------------------------------------ 3. equal sizes, one level

def test_all_sizes_equal_the_padded_size_is_the_uniform_levels_entry():
    """Every frame at the padded size: bitwise shpl_build_index_levels at that size, over every array's capacity."""
    from sparse_pooling_amd import _lib as L
    _pre("pyramid")
    batch = _stack()
    pts, vox, off, P, maxp, N = batch
    B = off.numel() - 1
    for levels in (lc.PAIR, lc.PYRAMID):
        outs, bits, _ = _against_singles(batch, [rc.PADDED] * B, levels)
        uni = [Outs(N, B) for _ in levels]
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        fo = torch.full((B + 1,), FILL, dtype=torch.int64, device=DEV)
        ws = L.workspace(L.index_levels_ws_bytes(B, maxp, len(levels)), DEV)
        arr = L.index_levels([(s, b, o.cell, o.pix, o.val, o.mij, o.flip, o.nnz) for (s, b), o in zip(levels, uni)])
        lead = L.index_args(B, off, None, maxp, pts, vox, P, rc.PADDED, (0, 0), (1, 1), None, None, None, None)
        L.check(L.lib().shpl_build_index_levels(*lead[:12], lead[16], len(levels), arr, L.ptr(fo), L.ptr(err),
                                                L.ptr(ws), ws.numel(), L.stream_of(DEV)), "shpl_build_index_levels")
        torch.cuda.synchronize()
        assert int(err.item()) == bits == 0
        for l in range(len(levels)):
            _assert_same(outs[l], uni[l], f"level {l}")
        assert int(_np(outs[0].nnz).sum()) > 3000


def test_one_level_equals_build_index_ragged():
    _pre("pair")
    batch = _stack()
    for level in (lc.PAIR[0], lc.PAIR[1], ((3, 5), (704, 800)), ((32, 32), (704, 800))):
        outs, bits, _ = _against_singles(batch, lrc.BASE_SIZES, [level])
        assert bits == 0 and int(_np(outs[0].nnz)[0]) > 2000


# ------------------------------------------------------------------ 4. counts, weights, optional outputs

def test_point_counts_mval_and_one_level_without_ref_outputs():
    from sparse_pooling_amd import _lib as L
    _pre("pair")
    batch = _stack()
    N = batch[5]
    frames = lrc.base_frames()
    counts = torch.tensor([2000, 1025, 307, 7, 100], dtype=torch.int64, device=DEV)  # frames 0, 1 and 4 shortened
    mval = torch.from_numpy(synth.make_features((N,), 7)).to(DEV)
    outs, bits, _ = _against_singles(batch, lrc.BASE_SIZES, lc.PAIR, counts=counts, mval=mval)
    assert bits == 0
    ref = lrc.oracle_levels(frames[0].points[:2000], frames[0].voxel_indices[:2000], synth.KITTI_P2, lc.PAIR,
                            lrc.BASE_SIZES[0])
    assert [int(_np(o.nnz)[0]) for o in outs] == [r["M_size"][1] for r in ref]
    # the values follow their points through the frame's own clip and each level's own compaction
    inside = synth._clip_mask(frames[0].points[:2000], synth.KITTI_P2, lrc.BASE_SIZES[0])
    z = frames[0].voxel_indices[:2000, 1]
    for o, rows in zip(outs, (700, 704)):
        np.testing.assert_array_equal(_np(o.val[:int(_np(o.nnz)[0])]), _np(mval[:2000])[inside & (z < rows)])
    # level 1 without mij / flip: every other array as before, level 0's mij / flip too
    mixed = [Outs(N, 5), Outs(N, 5, ref_outputs=False)]
    rc_, bits, _ = _levels_call(batch, lrc.BASE_SIZES, lc.PAIR, lrc.level_maps(lc.PAIR), mixed, counts=counts,
                                mval=mval)
    assert rc_ == L.OK and bits == 0
    _assert_same(mixed[0], outs[0], "level 0")
    for k in ("cell", "pix", "val", "nnz"):
        np.testing.assert_array_equal(_bits(_np(getattr(mixed[1], k))), _bits(_np(getattr(outs[1], k))))


# ------------------------------------------------------------------ 5. a map smaller than a frame, bad sizes

def test_level_map_smaller_than_a_frame_sets_the_pixel_bit_at_that_level_only():
    """Level 1's padded map fits 1224x370 only: entries of the larger frames whose strided pixel lies outside it
    get pix = -1 and SHPL_EBIT_PIXEL, exactly those; level 0's arrays are what they are with the full map."""
    from sparse_pooling_amd import _lib as L
    refs = _pre("pair")
    batch = _stack()
    off = _np(batch[2])
    full = lrc.level_maps(lc.PAIR)
    small = [full[0], rc.strided(rc.KITTI_SIZES[1], 8)]  # (46, 153) against (47, 155)
    base, bits0, _ = _against_singles(batch, lrc.BASE_SIZES, lc.PAIR)
    outs, bits, each = _against_singles(batch, lrc.BASE_SIZES, lc.PAIR, maps=small)
    assert bits0 == 0 and bits == L.EBIT_PIXEL and each == [0, L.EBIT_PIXEL]
    _assert_same(outs[0], base[0], "level 0")
    for k in ("cell", "val", "mij", "flip", "nnz"):  # level 1: only pix moves
        np.testing.assert_array_equal(_bits(_np(getattr(outs[1], k))), _bits(_np(getattr(base[1], k))))
    n_out = 0
    nnz = _np(outs[1].nnz)
    for f in range(5):
        flip = refs[f][1]["img_index_flip_pool"]
        want = rc.pix_ids(flip, f, *small[1])
        outside = (flip[:, 1] >= small[1][0]) | (flip[:, 2] >= small[1][1])
        assert ((want == -1) == outside).all()
        np.testing.assert_array_equal(_np(outs[1].pix[off[f]:off[f] + nnz[f]]), want)
        n_out += int(outside.sum())
    assert n_out >= 1


def test_bad_sizes_keep_nothing_at_any_level():
    """NaN, infinite, zero and negative sizes: nnz = 0 at every level, holes over the frame's whole capacity, no
    error bit, nothing outside the arrays (guard bands) -- and the good frames beside them as the oracle says."""
    sizes = [(1242.0, 376.0), (float("nan"), 376.0), (1242.0, 0.0), (-5.0, 376.0), (float("inf"), 376.0),
             (1242.0, float("inf")), (1242.0, float("-inf")), (1224.0, 370.0)]
    frames = rc.make_frames([1100] + [200] * 6 + [300], (1, 1), 400)
    batch = _stack(frames)
    off = _np(batch[2])
    for levels in (lc.PAIR, lc.PYRAMID):
        outs, bits, _ = _against_singles(batch, sizes, levels)
        assert bits == 0
        for l, o in enumerate(outs):
            nnz = _np(o.nnz)
            np.testing.assert_array_equal(nnz[1:7], 0)
            for f in range(1, 7):
                assert (_np(o.cell[off[f]:off[f + 1]]) == -1).all() and (_np(o.pix[off[f]:off[f + 1]]) == -1).all()
                assert (_np(o.val[off[f]:off[f + 1]]) == 0).all()
            for f in (0, 7):
                ref = lrc.oracle_levels(frames[f].points, frames[f].voxel_indices, frames[f].P, levels, sizes[f])[l]
                assert nnz[f] == ref["Mij_pool"].shape[0] > 0
                np.testing.assert_array_equal(_np(o.flip[off[f]:off[f] + nnz[f]]), ref["img_index_flip_pool"])


def test_refused_call_writes_nothing():
    from sparse_pooling_amd import _lib as L
    batch = _stack()
    N = batch[5]
    maps = lrc.level_maps(lc.PAIR)
    cases = [
        (dict(sizes=None), L.ERR_ARG),                                                    # NULL d_im_sizes
        (dict(maps=None), L.ERR_ARG),                                                     # NULL level_img_hw
        (dict(maps=[maps[0], (0, 155)]), L.ERR_BAD_SHAPE),                                # a map size < 1
        (dict(maps=[(-3, 1242), maps[1]]), L.ERR_BAD_SHAPE),
        (dict(maps=[maps[0], (1 << 20, 1 << 10)]), L.ERR_BAD_SHAPE),                      # 5 * 2^30 pixel ids
        (dict(levels=[lc.PAIR[0], ((0, 8), (704, 800))]), L.ERR_BAD_SHAPE),
        (dict(n_levels=0), L.ERR_BAD_SHAPE),
        (dict(n_levels=5), L.ERR_BAD_SHAPE),
    ]
    for kw, want in cases:
        args = dict(sizes=lrc.BASE_SIZES, maps=maps, levels=lc.PAIR, n_levels=None)
        args.update(kw)
        outs = [Outs(N, 5) for _ in args["levels"]]
        rc_, bits, fo = _levels_call(batch, args["sizes"], args["levels"], args["maps"], outs,
                                     n_levels=args["n_levels"])
        assert rc_ == want, (kw, rc_)
        assert bits == 0 and (fo == FILL).all() and all(o.untouched() and o.guards_intact() for o in outs), kw
    outs = [Outs(N, 5), Outs(N, 5)]
    outs[1].pix = None
    rc_, bits, fo = _levels_call(batch, lrc.BASE_SIZES, lc.PAIR, maps, outs)
    assert rc_ == L.ERR_ARG and (fo == FILL).all() and all(o.untouched() for o in outs)


# ------------------------------------------------------------------ 6. the reference fixture as a batch

@pytest.mark.parametrize("name", ["pair", "pyramid"])
def test_fixture_batch_equals_reference_arrays(name):
    from sparse_pooling_amd import shpl_map as sm
    g = lrc.golden()
    padded = tuple(int(v) for v in g["padded"])
    spec = synth.FrameSpec(0, padded, (704, 800), (1, 1))
    frames = [synth.Frame(g[f"points_{f}"], g[f"voxels_{f}"], g["P"], spec) for f in range(3)]
    pts, vox, off, P, maxp, N = _stack(frames)
    levels = lc.golden_levels(g, name)
    ibs = sm.build_index_levels(pts, vox, off, P, padded, levels, maxp, ref_outputs=True,
                                im_sizes=torch.from_numpy(g["sizes"]).to(DEV))
    for l, ib in enumerate(ibs):
        fo, fn = _np(ib.frame_off), _np(ib.frame_nnz)
        hp, wp = ib.img_hw
        assert (hp, wp) == rc.strided(padded, levels[l][0][0])
        for f in range(3):
            assert fn[f] == g[f"{name}_msize_{l}_{f}"][1]
            assert ib.bev_hw[0] * ib.bev_hw[1] == g[f"{name}_msize_{l}_{f}"][0]
            flip = g[f"{name}_flip_{l}_{f}"].reshape(-1, 3)
            np.testing.assert_array_equal(_np(ib.mij[fo[f]:fo[f] + fn[f]]), g[f"{name}_mij_{l}_{f}"].reshape(-1, 2))
            np.testing.assert_array_equal(_np(ib.flip[fo[f]:fo[f] + fn[f]]), flip)
            np.testing.assert_array_equal(_np(ib.map.pix[fo[f]:fo[f] + fn[f]]), rc.pix_ids(flip, f, hp, wp))
    assert ibs[0].map.error_bits() == 0


# ------------------------------------------------------------------ 7. chained: CSR and pulls per level

@pytest.mark.parametrize("name", ["pair", "pyramid"])
def test_each_level_map_through_csr_and_pulls(name):
    """Every level's map through the CSR builder and both pulls at 4 channels over padded features whose padding
    holds a non-zero pattern: frames 0 and 2 bitwise the oracle's layer at that level's stride under the window
    rule of ragged_cases."""
    from sparse_pooling_amd import shpl_map as sm
    refs = _pre(name)
    levels = lrc.SETS[name]
    pts, vox, off, P, maxp, N = _stack()
    ibs = sm.build_index_levels(pts, vox, off, P, rc.PADDED, levels, maxp, im_sizes=_sizes(lrc.BASE_SIZES))
    C, B, pick = 4, 5, [0, 2]
    sizes = [lrc.BASE_SIZES[f] for f in pick]
    for l, ((stride, bv_size), ib) in enumerate(zip(levels, ibs)):
        s = stride[0]
        (Hb, Wb), (hp, wp) = ib.bev_hw, ib.img_hw
        assert ib.map.n_pix == B * hp * wp and ib.map.n_cells == B * Hb * Wb
        bev = synth.make_features((B, Hb, Wb, C), 11 + l)
        img = rc.padded_features(B, hp, wp, C, lrc.BASE_SIZES, s, 21 + l)
        tb, ti = torch.from_numpy(bev).to(DEV), torch.from_numpy(img).to(DEV)
        got_b = sm.pool_img_to_bev(ib.map, ti, None, bev=tb)
        got_i = sm.pool_bev_to_img(ib.map, tb, None, img=ti)
        torch.cuda.synchronize()
        assert ib.map.error_bits() == 0
        want = rc.layer_oracle([refs[f][l] for f in pick], sizes, s, bev[pick], img[pick])
        for k, f in enumerate(pick):
            eb, ei = want[k][0], want[k][1]
            assert np.abs(eb[..., C:]).sum() > 0 and np.abs(ei[..., C:]).sum() > 0
            np.testing.assert_array_equal(_bits(_np(got_b[f:f + 1])), _bits(np.asarray(eb, np.float32)))
            np.testing.assert_array_equal(_bits(_np(got_i[f:f + 1])), _bits(np.asarray(ei, np.float32)))


# ------------------------------------------------------------------ 8. build_index_levels(im_sizes=)

def test_build_index_levels_im_sizes_equals_build_index_batch_per_level():
    from sparse_pooling_amd import shpl_map as sm
    _pre("pyramid")
    pts, vox, off, P, maxp, N = _stack()
    tsz = _sizes(lrc.BASE_SIZES)
    for levels, hws in ((lc.PAIR, None), (lc.PYRAMID, None), (lc.PAIR, [(380, 1250), (48, 160)])):
        ibs = sm.build_index_levels(pts, vox, off, P, rc.PADDED, levels, maxp, ref_outputs=True, im_sizes=tsz,
                                    img_hws=hws)
        assert len(ibs) == len(levels)
        for l, ((stride, bv_size), ib) in enumerate(zip(levels, ibs)):
            one = sm.build_index_batch(pts, vox, off, P, rc.PADDED, bv_size, stride, maxp, ref_outputs=True,
                                       im_sizes=tsz, img_hw=None if hws is None else hws[l])
            assert ib.map.err is ibs[0].map.err and ib.frame_off is ibs[0].frame_off
            assert (ib.bev_hw, ib.img_hw) == (one.bev_hw, one.img_hw)
            assert ib.img_hw == (rc.strided(rc.PADDED, stride[0]) if hws is None else hws[l])
            assert (ib.map.n_cells, ib.map.n_pix, ib.map.nnz_cap) == (one.map.n_cells, one.map.n_pix, one.map.nnz_cap)
            assert ib.map.n_pix == 5 * ib.img_hw[0] * ib.img_hw[1]
            assert ib.img_hw_frames.dtype == torch.int64 and tuple(ib.img_hw_frames.shape) == (5, 2)
            np.testing.assert_array_equal(_np(ib.img_hw_frames), _np(one.img_hw_frames))
            np.testing.assert_array_equal(_np(ib.img_hw_frames), [rc.strided(sz, stride[0]) for sz in lrc.BASE_SIZES])
            fo, fn = _np(one.frame_off), _np(one.frame_nnz)
            np.testing.assert_array_equal(_np(ib.frame_off), fo)
            np.testing.assert_array_equal(_np(ib.frame_nnz), fn)
            for x, y in ((ib.map.cell, one.map.cell), (ib.map.pix, one.map.pix), (ib.map.val, one.map.val)):
                np.testing.assert_array_equal(_bits(_np(x)), _bits(_np(y)))
            for f in range(5):  # mij / flip are written for the live entries
                for x, y in ((ib.mij, one.mij), (ib.flip, one.flip)):
                    np.testing.assert_array_equal(_np(x[fo[f]:fo[f] + fn[f]]), _np(y[fo[f]:fo[f] + fn[f]]))
        assert ibs[0].map.error_bits() == 0
    with pytest.raises(ValueError):
        sm.build_index_levels(pts, vox, off, P, rc.PADDED, lc.PAIR, maxp, img_hws=[(376, 1242), (47, 155)])
    # without either argument: today's call
    uni = sm.build_index_levels(pts, vox, off, P, rc.PADDED, lc.PAIR, maxp)
    assert all(ib.img_hw_frames is None for ib in uni) and uni[1].img_hw == (47, 155)
