"""The after-VGG upconv3 kernels -- k_upconv3x3 (shpl_upconv.hip), k_upconv3x3_dgrad, k_upconv3x3_wgrad and
k_upwgrad_reduce (shpl_upconv_grad.hip) -- pinned in every dispatch form on MI355X.

Every case makes three kinds of assertion: the result is within the derived bound of the float64 definition over
the oracle's fused map (upconv_ref / upconv_dx / upconv_dw, _bound, _within, the term counts and the bf16 store
term of tests/test_gpu_upconv.py and tests/test_gpu_upconv_grad.py, imported, not re-derived; the weight gradient
of the large cases as nine matmuls, dw9, which tests/test_upconv_forms_cases.py holds to upconv_dw); the bitwise
identities the project states hold where they apply (pooled over a CSR == the same call on the dense pulled map ==
the call on the materialised concat where c_a is a whole number of staging chunks, the materialised map itself
bitwise the oracle's; a split input gradient == the unsplit one's channels; a strided or offset view == the
contiguous call; taking statistics does not change the output); and the SHA-256 of every output's bytes equals the
value recorded in tests/golden/upconv_bits.json (tests/golden/make_upconv_bits.py, which runs these same case
functions). The table is self-referential: a pin for later refactors; the bounds and identities carry the
correctness claim. Where c_a is no whole number of chunks the two pooled identities are bounds only; whether they
came out bitwise is recorded beside the table ("identities"), not asserted.

Maps: dense_map of tests/test_gpu_conv_tiled.py (2 x 10 x 40, every cell of rows 0-8 holds 1..6 entries; cell-
and pixel-keyed), the planted map of tests/grouped_map.py (per-column order), rows_map.make(variant, shape) for
the other shapes. tests/test_upconv_forms_cases.py asserts without a GPU what these instantiations need of
dense_map: upconv halo rows y0-1 .. y0+7 over cells x0-1 .. x0+31 (find_runs<9, 33>), weight-gradient rows
y0 .. y0+3 over cells x0 .. x0+31 (find_runs<4, 32>).

k_upconv3x3<T, POOLED, STATS, GROUP> -> case id (dense_map, 32 + 16 -> 32; "cell": the cell-keyed CSR, "pixel":
the pixel-keyed CSR with ent_col)

    <float,0,0,0> fwd-dense-f32           <bf16,0,0,0> fwd-dense-bf16
    <float,0,1,0> fwd-dense-stats-f32     <bf16,0,1,0> fwd-dense-stats-bf16
    <float,1,0,0> fwd-cell-f32            <bf16,1,0,0> fwd-cell-bf16
    <float,1,1,0> fwd-cell-stats-f32      <bf16,1,1,0> fwd-cell-stats-bf16
    <float,1,0,1> fwd-pixel-f32           <bf16,1,0,1> fwd-pixel-bf16
    <float,1,1,1> fwd-pixel-stats-f32     <bf16,1,1,1> fwd-pixel-stats-bf16

  Further forward cases: fwd-planted[-stats] (<T,1,*,1> on the planted map, 16 + 32 -> 32, where the per-column
  and the plain sums differ), fwd-c40-bn-relu (<T,1,0,0>, c_out = 40 with a BatchNorm-inference epilogue and ReLU:
  block 0 stores 16-byte pieces, block 1 channel by channel, in one launch), fwd-stats-relu (<T,1,1,0>: statistics
  beside ReLU are those of the raw call), fwd-24+40 (<T,1,0,0>: at bf16 the tail of A's second chunk falls at the
  A/B boundary), fwd-1x1x1 (<T,1,0,0> on a one-cell map).

k_upconv3x3_dgrad<T, NB> -> case id; (n_cib, NB, n_cbg) asserted from dg_plan's rule (DGRAD_CASES)

    <float,1> dgrad-32-from-16-f32        <bf16,1> dgrad-32-from-16-bf16       (1, 1, 1)
    <float,2> dgrad-64-from-24-f32        <bf16,2> dgrad-64-from-24-bf16       (2, 2, 1); split at 20: vec_out false (bf16)
    <float,4> dgrad-128-from-64-f32       <bf16,4> dgrad-128-from-64-bf16      (4, 4, 1); split at 32, 64, 96

  Further NB = 4 cases: dgrad-96-from-40 (3, 4, 1: one zero-padded dx block, k_pack_w with n_blk > n_cib),
  dgrad-160-from-24 (5, 4, 2: the second workgroup column mostly padding), dgrad-70-from-40 (3, 4, 1: a ragged last
  block), dgrad-250-from-16 (8, 4, 2: ragged in the second column), all on 2 x 9 x 35, and dgrad-tile-96-from-24,
  dgrad-tile-70-from-64 on the one-tile map 1 x 8 x 32; dgrad-104-from-16 (4, 4, 1: three blocks of 16-byte stores
  and a ragged fourth, channel by channel, in one workgroup). Every case also reads gy through a wider row stride.

k_upconv3x3_wgrad<T, POOLED, GROUP> -> case id (dense_map; 32 + 32 -> 32, and 40 + 24 -> 40: the pooled chunks
start mid-block, the gy block of c0 = 32 is ragged, k_upwgrad_reduce maps channels at qa ck != c_a (bf16))

    <float,0,0> wgrad-32+32-32-dense-f32  <bf16,0,0> wgrad-32+32-32-dense-bf16
    <float,1,0> wgrad-32+32-32-cell-f32   <bf16,1,0> wgrad-32+32-32-cell-bf16
    <float,1,1> wgrad-32+32-32-pixel-f32  <bf16,1,1> wgrad-32+32-32-pixel-bf16

  wgrad-40+24-40-{dense,cell,pixel}: the same six on the second channel counts. wgrad-multi-{dense,cell,pixel}: the
  six on 7 x 12 x 32, 256 + 256 -> 128 (the reference's channel counts) through rows_map.make(variant, (7, 12, 32)):
  21 tiles, 64 block pairs, hence 11 groups of 2 tiles, the last of 1; group 1 walks (frame 0, tile 2) ->
  (frame 1, tile 0); k_upwgrad_reduce sums 8 + a tail of 3. wgrad-groups-{5,6,7}: F x 4 x 32, F = 5, 6, 7, the same
  channels: one tile per group, tails 1, 2, 3 past one whole round of 4. Every (n_tiles, tiles_per_group, n_groups)
  is asserted from wgrad_groups' formula (uw_plan below).

C ABI views (abi-*; a test-local caller of shpl_upconv3x3, _dgrad and _wgrad through _lib): A and B as channel
slices of wider buffers at an offset of a whole piece (8: LDS-DMA) and not (3: masked loads), both bitwise the
contiguous call; out_stride > c_out, gy_stride > c_out (by 8 and by 3); dx / dx_b rows wider than their channels;
c_a = 0 with a pooled B, forward and weight gradient (chunk_src's PAST addressing B). Every byte outside a view
keeps its sentinel.
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

import grouped_map as gm
import rows_map as rm
import test_gpu_conv_rows as R
import test_gpu_conv_tiled as T
import test_gpu_upconv as base
import test_gpu_upconv_grad as G
from oracle import shpl_oracle as orc

pytestmark = pytest.mark.gpu

DEV = base.DEV
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "upconv_bits.json")
TH, TW, WTH = 8, 32, 4  # the forward's and the input gradient's tile; the weight gradient's rows per tile
MULTI_SHAPE = (7, 12, 32)
SENTINEL = -77.0  # exact in bf16
# {case: {"dense": bool, "concat": bool}}: whether the pooled call came out bitwise the dense pulled map's / the
# materialised concat's where c_a is no whole number of chunks (recorded by make_upconv_bits.py, not asserted)
IDENT = {}


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from sparse_pooling_amd import _lib as L
    L.lib()
    assert torch.cuda.is_available()


# ------------------------------------------------------------------ the host plans, restated
def chunk(bf):
    return 16 if bf else 8  # Elem<T>::CK: channels per 32-byte staging chunk


def _up256(n):
    return (n + 255) // 256 * 256


def dg_plan(bf, c_gy, c_dx):
    """dg_plan of shpl_upconv_grad.hip: (n_cib, NB, n_cbg, workspace bytes)."""
    n_cib = (c_dx + 31) // 32
    nb = n_cib if n_cib <= 2 else 4
    n_cbg = (n_cib + nb - 1) // nb
    qa = (c_gy + chunk(bf) - 1) // chunk(bf)
    return n_cib, nb, n_cbg, _up256(n_cbg * nb * qa * 288 * 32)


def uw_plan(bf, n_frames, h, w, c_a, c_b, c_out, pooled):
    """uw_plan / wgrad_groups: {n_tiles, tiles_per_group, n_groups, n_cib, n_cob, tiles_per_frame, bytes}."""
    ck = chunk(bf)
    qa, qb = (c_a + ck - 1) // ck, (c_b + ck - 1) // ck
    n_cib, n_cob = ((qa + qb) * ck + 31) // 32, (c_out + 31) // 32
    tiles_per_frame = (w + TW - 1) // TW * ((h + WTH - 1) // WTH)
    n_tiles = n_frames * tiles_per_frame
    ng = min(max(1024 // (n_cib * n_cob), 1), max(n_tiles, 1))
    tpg = max((n_tiles + ng - 1) // ng, 1)
    n_groups = max((n_tiles + tpg - 1) // tpg, 1)
    nbytes = _up256(n_frames * (h + 1) * 4 if pooled else 0) + _up256(n_groups * n_cib * n_cob * 9 * 32 * 32 * 4)
    return {"n_tiles": n_tiles, "tiles_per_group": tpg, "n_groups": n_groups, "n_cib": n_cib, "n_cob": n_cob,
            "tiles_per_frame": tiles_per_frame, "bytes": nbytes}


def group_tiles(plan, grp):
    """The (frame, tile in frame) pairs group grp walks, t1 clamped to n_tiles."""
    t0 = grp * plan["tiles_per_group"]
    return [divmod(t, plan["tiles_per_frame"]) for t in range(t0, min(t0 + plan["tiles_per_group"], plan["n_tiles"]))]


def dw9(x, g):
    """base.upconv_dw as nine matmuls (float64)."""
    F, h, wd, ci = x.shape
    out = np.zeros((3, 3, g.shape[-1], ci))
    for ky in range(3):
        for kx in range(3):
            hh, ww = (h if ky < 2 else h - 1), (wd if kx < 2 else wd - 1)
            gs = g[:, ky:ky + 2 * hh:2, kx:kx + 2 * ww:2].reshape(-1, g.shape[-1])
            out[ky, kx] = gs.T @ x[:, :hh, :ww].reshape(-1, ci)
    return out


# ------------------------------------------------------------------ operands
def _dev(a, bf):
    t = base._t(np.asarray(a, np.float32))
    return t.to(torch.bfloat16) if bf else t


def _host(t):
    return t.detach().float().cpu().numpy()


def _weights(co, cin, seed, bf):
    w = np.random.default_rng(seed).uniform(-0.5, 0.5, (3, 3, co, cin)).astype(np.float32)
    return base._rd(w) if bf else w


def _grad(shape, co, seed, bf):
    F, h, w = shape
    g = np.random.default_rng(seed).standard_normal((F, 2 * h, 2 * w, co)).astype(np.float32)
    return base._rd(g) if bf else g


def oracle_fused(m, a, b, pixel, absval=False):
    """The oracle's [a || pooled b] of a map in the reference format, f32: cell-keyed (a the target map) or
    pixel-keyed (a the image); absval: |M|'s values (the bound's sum over absolute values)."""
    mv = np.abs(m["mval"]) if absval else m["mval"]
    ca, cb = a.shape[-1], b.shape[-1]
    if pixel:
        _, ref = orc.sparse_pool_layer(b.reshape(1, -1, b.shape[2], cb), a, m["mij"], mv, m["m_size"], m["idx"],
                                       dual=True)
    else:
        ref, _ = orc.sparse_pool_layer(a.reshape(1, -1, a.shape[2], ca), b, m["mij"], mv, m["m_size"], m["idx"])
    return ref.reshape(a.shape[:3] + (ca + cb,))


def _rows_f32(variant, ca, cb, shape):
    """R._pooled (bf16 only) for f32, over the same bf16-representable features: the materialised map is
    bitwise the oracle's, unrounded."""
    from sparse_pooling_amd import _lib as L, shpl_map as sm
    m, a, b, _ = R._pool_ref(variant, ca, cb, shape)
    ref = oracle_fused(m, a, b, variant == "pixel")
    ta, tb, smap = base._t(a), base._t(b), R._smap(m)
    if variant == "pixel":
        pool = smap.csr(L.BY_PIXEL, L.ORDER_COL_ROW)
        mat = sm.pool_bev_to_img(smap, tb, ta.shape, img=ta)
    else:
        pool = smap.csr(L.BY_CELL, L.ORDER_ENTRY)
        mat = sm.pool_img_to_bev(smap, tb, ta.shape, bev=ta)
    torch.cuda.synchronize()
    assert smap.error_bits() == 0
    np.testing.assert_array_equal(_host(mat), ref)
    return ta, tb, pool, smap.frame_off, mat, ref, m


def longest_run(which, key, m):
    if which != "planted":
        return int(m["counts"].max())
    mij, idx = m["mij"], m["idx"]
    return int(np.bincount(idx[mij[:, 1], 1] * gm.IMG_HW[1] + idx[mij[:, 1], 2]).max())


@functools.lru_cache(maxsize=None)
def _operand(which, key, ca, cb, bf, shape=None):
    """The inputs of a case, made once and left unchanged. which: "dense" (dense_map), "planted" (pixel-keyed),
    "rows" (rows_map.make(key, shape)) or "plain" (no map: a random [shape, ca + cb] input). Fields: ta, tb, pool,
    foff (None for "plain"), mat (the materialised [a || pooled] device map, bitwise the oracle's), x (that map,
    f32 on the host), xabs (the same over absolute values, float64), L (the longest run), shape (F, h, w)."""
    o = base.Case()
    o.ca, o.cb, o.bf, o.pixel = ca, cb, bf, key == "pixel"
    if which == "plain":
        x = np.random.default_rng(ca + cb + sum(shape)).standard_normal(shape + (ca + cb,)).astype(np.float32)
        o.x = base._rd(x) if bf else x
        o.ta = o.tb = o.pool = o.foff = None
        o.mat, o.xabs, o.L = _dev(o.x, bf), np.abs(o.x).astype(np.float64), 0
    else:
        if which == "rows":
            got = R._pooled(key, ca, cb, shape) if bf else _rows_f32(key, ca, cb, shape)
            o.ta, o.tb, o.pool, o.foff, o.mat, o.x, m = got
        else:
            o.ta, o.tb, o.pool, o.foff, o.mat, o.x = T._pooled(key, which, ca, cb, bf)
            m = gm.make() if which == "planted" else T.dense_map(o.pixel)
        assert (o.pool.ent_col is not None) == o.pixel  # GROUP
        o.L = longest_run(which, key, m)
        o.xabs = oracle_fused(m, np.abs(_host(o.ta)), np.abs(_host(o.tb)), o.pixel, True).astype(np.float64)
    o.shape = tuple(int(s) for s in o.mat.shape[:3])
    o.ma, o.mb = o.mat[..., :ca].contiguous(), o.mat[..., ca:].contiguous()
    o.store = (lambda ref: np.abs(ref) * 2.0 ** -8) if bf else (lambda ref: 0.0)
    o.whole = ca % chunk(bf) == 0
    return o


def _same(u, v):
    if u is None or v is None:
        return u is v
    if u.dtype == torch.bfloat16:
        u, v = u.contiguous().view(torch.int16), v.contiguous().view(torch.int16)
    return u.shape == v.shape and bool(torch.equal(u, v))


# ------------------------------------------------------------------ forward
def _up(a, tw, b=None, pool=None, foff=None, epi=None, relu=False, stats=False):
    from sparse_pooling_amd import fusion_upconv as fu
    kw = {} if epi is None else dict(center=base._t(epi[0]), scale=base._t(epi[1]), shift=base._t(epi[2]))
    st = torch.zeros((2, int(tw.shape[2])), dtype=torch.float64, device=DEV) if stats else None
    return fu.upconv3x3(a, tw, b=b, pool=pool, frame_off=foff, relu=relu, stats=st, **kw), st


FWD_SEED, GY_SEED = 4, 43  # the forward cases' weights, the weight gradient cases' gy


@functools.lru_cache(maxsize=None)
def _fwd_ref(o, cout, L, lo):
    """(the float64 definition, its bound of n = 4 c_in + L terms) over channels [lo, c_a + c_b) of o's map."""
    W = _weights(cout, o.ca + o.cb, FWD_SEED, o.bf)[..., lo:].astype(np.float64)
    raw = base.upconv_ref(o.x[..., lo:].astype(np.float64), W)
    return raw, base._bound(base.upconv_ref(o.xabs[..., lo:], np.abs(W)), 4 * W.shape[3] + L)


def _fwd_vs_oracle(what, o, cout, y, st, epi, relu, L, lo=0):
    """base.test_forward's bound (the bf16 store added), base.test_epilogue's with an epilogue, and
    base.test_forward's statistics bounds; lo: the first channel of o's map the call read."""
    raw, rb = _fwd_ref(o, cout, L, lo)
    if epi is None:
        ref = np.maximum(raw, 0.0) if relu else raw
        bound = rb + o.store(ref)
    else:
        ce, sc, sh = (v.astype(np.float64) for v in epi)
        ref = (raw - ce) * sc + sh
        ref = np.maximum(ref, 0.0) if relu else ref
        bound = sc * rb + base._bound(np.abs(raw) * sc + np.abs(ce) * sc + np.abs(sh), 3) + o.store(ref)
    base._within(what, base._np(y), ref, bound)
    if st is not None:
        flat, fb = raw.reshape(-1, cout), rb.reshape(-1, cout)
        base._within(what + " stats sum", st[0].cpu().numpy(), flat.sum(0), fb.sum(0))
        base._within(what + " stats sumsq", st[1].cpu().numpy(), (flat ** 2).sum(0),
                     ((2 * np.abs(flat) + fb) * fb).sum(0) + base._bound((flat ** 2).sum(0), 1))


def fwd_form(bf, key, pooled, stats):
    return "<%s,%d,%d,%d>" % ("bf16" if bf else "float", pooled, stats, pooled and key == "pixel")


def case_fwd(name, bf, which, key, ca, cb, cout, pooled, stats, relu=False, bn=False, shape=None):
    """k_upconv3x3<T, pooled, stats, key == "pixel">: pooled over the CSR, or dense over the materialised map's
    two halves."""
    o = _operand(which, key, ca, cb, bf, shape)
    tw = _dev(_weights(cout, ca + cb, FWD_SEED, bf), bf)
    epi = T._epilogue(cout, 5) if bn else None
    kw = dict(epi=epi, relu=relu)
    if pooled:
        y, st = _up(o.ta, tw, o.tb, o.pool, o.foff, stats=stats, **kw)
        yd, sd = _up(o.ta, tw, o.mb, stats=stats, **kw)
    else:
        y, st = _up(o.ma, tw, o.mb, stats=stats, **kw)
        yd, sd = y, st
    yc, sc = _up(o.mat, tw, stats=stats, **kw)
    torch.cuda.synchronize()
    L = o.L if pooled else 0
    _fwd_vs_oracle("fwd", o, cout, y, st, epi, relu, L)
    _fwd_vs_oracle("fwd dense pulled map", o, cout, yd, sd, epi, relu, L)
    _fwd_vs_oracle("fwd materialised", o, cout, yc, sc, epi, relu, L)
    if o.whole:
        assert _same(yd, y), "the pooled call differs from the call on the dense pulled map"
        assert _same(yc, y), "the call on the materialised concat differs"
        if stats:
            assert torch.equal(sd, st) and torch.equal(sc, st)
    else:
        IDENT[name] = {"dense": _same(yd, y), "concat": _same(yc, y)}
    if stats:  # taking statistics does not change the output; beside ReLU they are the raw call's
        args = (o.ta, tw, o.tb, o.pool, o.foff) if pooled else (o.ma, tw, o.mb)
        assert _same(_up(*args, **kw)[0], y), "taking statistics changes the output"
        if relu:
            yr, sr = _up(*args, epi=epi, relu=False, stats=True)
            assert torch.equal(sr, st), "ReLU changes the statistics"
            assert float(y.float().min()) >= 0.0 and bool((y == 0).any()) and bool((yr.float() < 0).any())
    return {"y": y} if st is None else {"y": y, "stats": st}


# ------------------------------------------------------------------ input gradient
DGRAD_SHAPE, TILE_SHAPE = (2, 9, 35), (1, 8, 32)
DGRAD_CASES = {  # name: (shape, c_gy, c_dx, splits, (n_cib, NB, n_cbg))
    "dgrad-32-from-16": (DGRAD_SHAPE, 16, 32, (), (1, 1, 1)),
    "dgrad-64-from-24": (DGRAD_SHAPE, 24, 64, (32, 20), (2, 2, 1)),
    "dgrad-96-from-40": (DGRAD_SHAPE, 40, 96, (32,), (3, 4, 1)),
    "dgrad-128-from-64": (DGRAD_SHAPE, 64, 128, (32, 64, 96), (4, 4, 1)),
    "dgrad-104-from-16": (DGRAD_SHAPE, 16, 104, (64,), (4, 4, 1)),
    "dgrad-160-from-24": (DGRAD_SHAPE, 24, 160, (128,), (5, 4, 2)),
    "dgrad-70-from-40": (DGRAD_SHAPE, 40, 70, (64,), (3, 4, 1)),
    "dgrad-250-from-16": (DGRAD_SHAPE, 16, 250, (), (8, 4, 2)),
    "dgrad-tile-96-from-24": (TILE_SHAPE, 24, 96, (), (3, 4, 1)),
    "dgrad-tile-70-from-64": (TILE_SHAPE, 64, 70, (35,), (3, 4, 1)),
}


def dgrad_form(bf, c_gy, c_dx):
    return "<%s,%d>" % ("bf16" if bf else "float", dg_plan(bf, c_gy, c_dx)[1])


def case_dgrad(name, bf, shape, cg, cdx, splits, plan):
    """k_upconv3x3_dgrad<T, NB> against upconv_dx (n = 9 c_gy terms, the bf16 store); gy through a wider row
    stride and every split bitwise the contiguous, unsplit call."""
    from sparse_pooling_amd import fusion_upconv as fu
    assert dg_plan(bf, cg, cdx)[:3] == plan
    g, w = _grad(shape, cg, 21, bf), _weights(cg, cdx, 22, bf)
    tg, tw = _dev(g, bf), _dev(w, bf)
    dx = fu.upconv3x3_dgrad(tg, tw, cdx)
    strided = fu.upconv3x3_dgrad(G._wide(tg), tw, cdx)
    parts = {c: fu.upconv3x3_dgrad(tg, tw, cdx, split=c) for c in splits}
    torch.cuda.synchronize()
    g64, W = g.astype(np.float64), w.astype(np.float64)
    ref = base.upconv_dx(g64, W)
    bound = base._bound(base.upconv_dx(np.abs(g64), np.abs(W)), 9 * cg) + (np.abs(ref) * 2.0 ** -8 if bf else 0.0)
    base._within("dx", base._np(dx), ref, bound)
    assert _same(strided, dx), "gy_stride > c_gy changes the result"
    outs = {"dx": dx}
    for c, (da, db) in parts.items():
        assert da.shape[-1] == c and db.shape[-1] == cdx - c
        assert _same(torch.cat([da, db], -1), dx), "the split at %d differs from the unsplit call" % c
        outs["da%d" % c], outs["db%d" % c] = da, db
    return outs


# ------------------------------------------------------------------ weight gradient
def wgrad_form(bf, key, pooled):
    return "<%s,%d,%d>" % ("bf16" if bf else "float", pooled, pooled and key == "pixel")


@functools.lru_cache(maxsize=None)
def _wgrad_ref(o, cout, lo):
    """(the float64 definition, its bound of n = F h w terms) over channels [lo, c_a + c_b) of o's map."""
    g64 = _grad(o.shape, cout, GY_SEED, o.bf).astype(np.float64)
    F, h, w = o.shape
    return (dw9(o.x[..., lo:].astype(np.float64), g64),
            base._bound(dw9(o.xabs[..., lo:], np.abs(g64)), F * h * w))


def _wgrad_vs_oracle(what, dw, o, cout, lo=0):
    base._within(what, base._np(dw), *_wgrad_ref(o, cout, lo))


def case_wgrad(name, bf, which, key, ca, cb, cout, pooled, shape=None, expect=None):
    """k_upconv3x3_wgrad<T, pooled, key == "pixel"> + k_upwgrad_reduce against upconv_dw over the oracle's fused
    map (n = F h w terms); expect: the (n_tiles, tiles_per_group, n_groups) the case is there for."""
    from sparse_pooling_amd import fusion_upconv as fu
    o = _operand(which, key, ca, cb, bf, shape)
    plan = uw_plan(bf, *o.shape, ca, cb, cout, pooled)
    if expect is not None:
        assert (plan["n_tiles"], plan["tiles_per_group"], plan["n_groups"]) == expect, plan
    tg = _dev(_grad(o.shape, cout, GY_SEED, bf), bf)
    if pooled:
        dw = fu.upconv3x3_wgrad(o.ta, tg, b=o.tb, pool=o.pool, frame_off=o.foff)
        dd = fu.upconv3x3_wgrad(o.ta, tg, b=o.mb)
    else:
        dw = dd = fu.upconv3x3_wgrad(o.ma, tg, b=o.mb)
    dc = fu.upconv3x3_wgrad(o.mat, tg)
    torch.cuda.synchronize()
    assert tuple(dw.shape) == (3, 3, cout, ca + cb) and dw.dtype == torch.float32
    _wgrad_vs_oracle("dW", dw, o, cout)
    _wgrad_vs_oracle("dW dense pulled map", dd, o, cout)
    _wgrad_vs_oracle("dW materialised", dc, o, cout)
    if o.whole:
        assert torch.equal(dd, dw), "the pooled call differs from the call on the dense pulled map"
        assert torch.equal(dc, dw), "the call on the materialised concat differs"
    else:
        IDENT[name] = {"dense": bool(torch.equal(dd, dw)), "concat": bool(torch.equal(dc, dw))}
    return {"dw": dw}


# ------------------------------------------------------------------ the C ABI through views
def _slot(t, off, extra):
    """t's channels at [off, off + C) of a buffer whose rows are off + C + extra wide, sentinels elsewhere."""
    buf = torch.full(tuple(t.shape[:-1]) + (off + t.shape[-1] + extra,), SENTINEL, dtype=t.dtype, device=t.device)
    buf[..., off:off + t.shape[-1]] = t
    return buf


def _kept(buf, off, c):
    """Every channel of buf outside [off, off + c) still holds the sentinel."""
    return bool((buf[..., :off].float() == SENTINEL).all()) and bool((buf[..., off + c:].float() == SENTINEL).all())


def _code(bf):
    from sparse_pooling_amd import _lib as L
    return L.BF16 if bf else L.F32


def abi_fwd(bf, shape, a, a_off, ca, b, b_off, cb, pool, foff, tw, out, cout, stats=None):
    """shpl_upconv3x3 as fusion_upconv.upconv3x3 calls it, raw (no epilogue); a, b: the whole buffers (rows of
    shape[-1] elements), of which the channels [off, off + c) are read; out: rows of out.shape[-1] elements."""
    from sparse_pooling_amd import _lib as L, fusion_upconv as fu
    F, h, w = shape
    ws = L.workspace(fu.upconv_ws_bytes(_code(bf), F, h, w, ca, cb, cout, None if pool is None else pool.nnz_cap,
                                        stats is not None), DEV)
    L.check(L.lib().shpl_upconv3x3(_code(bf), F, h, w, L.ptr(a), 0 if a is None else int(a.shape[-1]), a_off, ca,
                                   L.ptr(b), 0 if b is None else int(b.shape[-1]), b_off, cb,
                                   None if pool is None else pool.ref(), L.ptr(foff), L.ptr(tw), cout, None, None,
                                   None, L.ACT_NONE, L.ptr(out), int(out.shape[-1]), L.ptr(stats), L.ptr(ws),
                                   ws.numel(), L.stream_of(DEV)), "shpl_upconv3x3")
    return out


def abi_wgrad(bf, shape, a, a_off, ca, b, b_off, cb, pool, foff, gy, cout):
    """shpl_upconv3x3_wgrad as fusion_upconv.upconv3x3_wgrad calls it; gy: rows of gy.shape[-1] elements."""
    from sparse_pooling_amd import _lib as L, fusion_upconv as fu
    F, h, w = shape
    dw = torch.empty((3, 3, cout, ca + cb), dtype=torch.float32, device=DEV)
    ws = L.workspace(fu.upconv_grad_ws_bytes("wgrad", _code(bf), F, h, w, ca, cb, cout,
                                             None if pool is None else pool.nnz_cap), DEV)
    L.check(L.lib().shpl_upconv3x3_wgrad(_code(bf), F, h, w, L.ptr(a), 0 if a is None else int(a.shape[-1]), a_off,
                                         ca, L.ptr(b), 0 if b is None else int(b.shape[-1]), b_off, cb,
                                         None if pool is None else pool.ref(), L.ptr(foff), L.ptr(gy),
                                         int(gy.shape[-1]), cout, L.ptr(dw), L.ptr(ws), ws.numel(),
                                         L.stream_of(DEV)), "shpl_upconv3x3_wgrad")
    return dw


def abi_dgrad(bf, shape, gy, cg, tw, cdx, dx, split, dx_b):
    """shpl_upconv3x3_dgrad as fusion_upconv.upconv3x3_dgrad calls it; dx, dx_b: rows of their shape[-1]."""
    from sparse_pooling_amd import _lib as L, fusion_upconv as fu
    F, h, w = shape
    ws = L.workspace(fu.upconv_grad_ws_bytes("dgrad", _code(bf), F, h, w, cg, 0, cdx), DEV)
    L.check(L.lib().shpl_upconv3x3_dgrad(_code(bf), F, h, w, L.ptr(gy), int(gy.shape[-1]), cg, L.ptr(tw), cdx,
                                         L.ptr(dx), int(dx.shape[-1]), split, L.ptr(dx_b), int(dx_b.shape[-1]),
                                         L.ptr(ws), ws.numel(), L.stream_of(DEV)), "shpl_upconv3x3_dgrad")


def _unchanged(*pairs):
    for buf, keep in pairs:
        assert _same(buf, keep), "a source buffer was written"


def case_abi_offsets(name, bf, off, which):
    """A and B as channel slices at `off` of wider buffers (B pooled through the cell-keyed CSR, then the dense
    pulled map): bitwise the contiguous call's, forward or weight gradient; off = 8 is a whole piece at either
    type (LDS-DMA), off = 3 is not (vec16 false: masked loads of the same values)."""
    from sparse_pooling_amd import fusion_upconv as fu
    ca, cb, cout = 32, 16, 32
    o = _operand("dense", "cell", ca, cb, bf)
    F, h, w = o.shape
    tw = _dev(_weights(cout, ca + cb, FWD_SEED, bf), bf)
    tg = _dev(_grad(o.shape, cout, GY_SEED, bf), bf)
    va, vb, vm = _slot(o.ta, off, 8 - off), _slot(o.tb, off, 8 - off), _slot(o.mb, off, 8 - off)
    keep = [(v, v.clone()) for v in (va, vb, vm)]
    assert (off % (8 if bf else 4) == 0) == (off == 8) and va.shape[-1] == ca + 8
    if which == "fwd":
        want, _ = _up(o.ta, tw, o.tb, o.pool, o.foff)
        got = [abi_fwd(bf, o.shape, va, off, ca, vb, off, cb, o.pool, o.foff, tw, torch.empty_like(want), cout),
               abi_fwd(bf, o.shape, va, off, ca, vm, off, cb, None, None, tw, torch.empty_like(want), cout)]
    else:
        want = fu.upconv3x3_wgrad(o.ta, tg, b=o.tb, pool=o.pool, frame_off=o.foff)
        got = [abi_wgrad(bf, o.shape, va, off, ca, vb, off, cb, o.pool, o.foff, tg, cout),
               abi_wgrad(bf, o.shape, va, off, ca, vm, off, cb, None, None, tg, cout)]
    torch.cuda.synchronize()
    _unchanged(*keep)
    assert _same(got[0], want), "pooled B at an offset differs from the contiguous call"
    assert _same(got[1], want), "dense B at an offset differs from the contiguous call"
    return {"pooled": got[0], "dense": got[1]}


def case_abi_strides(name, bf, which):
    """out_stride > c_out (forward, c_out = 40: a fast and a slow block) and gy_stride > c_out (weight gradient,
    40 + 24 -> 40: a ragged gy block), by 8 (16-byte rows) and by 3 (not): bitwise the contiguous call's, the
    bytes between the rows untouched."""
    from sparse_pooling_amd import fusion_upconv as fu
    cout, outs = 40, {}
    if which == "fwd":
        o = _operand("dense", "cell", 32, 16, bf)
        tw = _dev(_weights(cout, 48, FWD_SEED, bf), bf)
        want, _ = _up(o.ta, tw, o.tb, o.pool, o.foff)
        for extra in (8, 3):
            buf = _slot(torch.zeros_like(want), 0, extra)
            buf[..., :cout] = SENTINEL
            abi_fwd(bf, o.shape, o.ta, 0, 32, o.tb, 0, 16, o.pool, o.foff, tw, buf, cout)
            torch.cuda.synchronize()
            assert _same(buf[..., :cout].contiguous(), want) and _kept(buf, 0, cout), extra
            outs["y+%d" % extra] = buf
    else:
        o = _operand("dense", "cell", 40, 24, bf)
        tg = _dev(_grad(o.shape, cout, GY_SEED, bf), bf)
        want = fu.upconv3x3_wgrad(o.ta, tg, b=o.tb, pool=o.pool, frame_off=o.foff)
        for extra in (8, 3):
            buf = _slot(tg, 0, extra)
            keep = buf.clone()
            dw = abi_wgrad(bf, o.shape, o.ta, 0, 40, o.tb, 0, 24, o.pool, o.foff, buf, cout)
            torch.cuda.synchronize()
            _unchanged((buf, keep))
            assert _same(dw, want), extra
            outs["dw+%d" % extra] = dw
    return outs


def case_abi_ca0(name, bf, which):
    """c_a = 0 with a pooled B (40 channels: the weight gradient's last block reaches past the last chunk, which
    chunk_src<PAST> addresses in B): within the bound of the definition over the pooled half of the oracle's
    fused map, and bitwise the one-source call on the dense pulled map."""
    from sparse_pooling_amd import fusion_upconv as fu
    ca, cb, cout = 24, 40, 32
    o = _operand("dense", "cell", ca, cb, bf)
    if which == "fwd":
        tw = _dev(np.ascontiguousarray(_weights(cout, ca + cb, FWD_SEED, bf)[..., ca:]), bf)
        want, _ = _up(o.mb, tw)
        y = abi_fwd(bf, o.shape, None, 0, 0, o.tb, 0, cb, o.pool, o.foff, tw, torch.empty_like(want), cout)
        torch.cuda.synchronize()
        _fwd_vs_oracle("fwd c_a = 0", o, cout, y, None, None, False, o.L, lo=ca)
        assert _same(y, want)
        return {"y": y}
    tg = _dev(_grad(o.shape, cout, GY_SEED, bf), bf)
    dw = abi_wgrad(bf, o.shape, None, 0, 0, o.tb, 0, cb, o.pool, o.foff, tg, cout)
    want = fu.upconv3x3_wgrad(o.mb, tg)
    torch.cuda.synchronize()
    _wgrad_vs_oracle("dW c_a = 0", dw, o, cout, lo=ca)
    assert torch.equal(dw, want)
    return {"dw": dw}


def case_abi_dgrad(name, bf):
    """dx and dx_b as the leading channels of wider rows, 24 -> 64: split at 32 (rows wider by 8: 16-byte pieces)
    and at 20 (by 3: channel by channel), bitwise the contiguous split call's, the bytes between untouched."""
    from sparse_pooling_amd import fusion_upconv as fu
    shape, cg, cdx = DGRAD_SHAPE, 24, 64
    tg, tw = _dev(_grad(shape, cg, 21, bf), bf), _dev(_weights(cg, cdx, 22, bf), bf)
    outs = {}
    for split, extra in ((32, 8), (20, 3)):
        da, db = fu.upconv3x3_dgrad(tg, tw, cdx, split=split)
        va, vb = _slot(torch.zeros_like(da), 0, extra), _slot(torch.zeros_like(db), 0, extra)
        va[..., :split], vb[..., :cdx - split] = SENTINEL, SENTINEL
        abi_dgrad(bf, shape, tg, cg, tw, cdx, va, split, vb)
        torch.cuda.synchronize()
        assert _same(va[..., :split].contiguous(), da) and _kept(va, 0, split), split
        assert _same(vb[..., :cdx - split].contiguous(), db) and _kept(vb, 0, cdx - split), split
        outs["da%d" % split], outs["db%d" % split] = va, vb
    return outs


# ------------------------------------------------------------------ the case table
CASES, FORMS = {}, {}  # name: (function, arguments after the name); name: the kernel instantiation it runs


def _add(name, form, fn, *args):
    assert name not in CASES
    CASES[name], FORMS[name] = (fn, args), form


WGRAD_EXPECT = {  # (n_tiles, tiles_per_group, n_groups)
    "dense_map": (12, 1, 12), "multi": (21, 2, 11), "groups-5": (5, 1, 5), "groups-6": (6, 1, 6), "groups-7": (7, 1, 7)}

for _bf in (False, True):
    _d = "bf16" if _bf else "f32"
    # forward: the twelve instantiations on dense_map, 32 + 16 -> 32
    for _key, _po in (("cell", False), ("cell", True), ("pixel", True)):
        for _st in (False, True):
            _n = "fwd-%s%s-%s" % (_key if _po else "dense", "-stats" if _st else "", _d)
            _add(_n, "k_upconv3x3" + fwd_form(_bf, _key, _po, _st), case_fwd, _bf, "dense", _key, 32, 16, 32, _po, _st)
    for _st in (False, True):
        _add("fwd-planted%s-%s" % ("-stats" if _st else "", _d), "k_upconv3x3" + fwd_form(_bf, "pixel", True, _st),
             case_fwd, _bf, "planted", "pixel", 16, 32, 32, True, _st)
    _add("fwd-c40-bn-relu-" + _d, "k_upconv3x3" + fwd_form(_bf, "cell", True, False), case_fwd, _bf, "dense", "cell",
         32, 16, 40, True, False, True, True)
    _add("fwd-stats-relu-" + _d, "k_upconv3x3" + fwd_form(_bf, "cell", True, True), case_fwd, _bf, "dense", "cell",
         32, 16, 32, True, True, True)
    _add("fwd-24+40-" + _d, "k_upconv3x3" + fwd_form(_bf, "cell", True, False), case_fwd, _bf, "dense", "cell",
         24, 40, 32, True, False)
    _add("fwd-1x1x1-" + _d, "k_upconv3x3" + fwd_form(_bf, "cell", True, False), case_fwd, _bf, "rows", "cell",
         8, 8, 8, True, False, False, False, (1, 1, 1))
    # input gradient
    for _n, (_shape, _cg, _cdx, _splits, _plan) in DGRAD_CASES.items():
        _add("%s-%s" % (_n, _d), "k_upconv3x3_dgrad" + dgrad_form(_bf, _cg, _cdx), case_dgrad, _bf, _shape, _cg, _cdx,
             _splits, _plan)
    # weight gradient: the six instantiations on dense_map at two channel counts, and on the multi-tile groups
    for _key, _po in (("cell", False), ("cell", True), ("pixel", True)):
        _form = "k_upconv3x3_wgrad" + wgrad_form(_bf, _key, _po)
        _v = _key if _po else "dense"
        for _ca, _cb, _co in ((32, 32, 32), (40, 24, 40)):
            _add("wgrad-%d+%d-%d-%s-%s" % (_ca, _cb, _co, _v, _d), _form, case_wgrad, _bf, "dense", _key, _ca, _cb,
                 _co, _po, None, WGRAD_EXPECT["dense_map"])
        _add("wgrad-multi-%s-%s" % (_v, _d), _form, case_wgrad, _bf, "rows", _key, 256, 256, 128, _po, MULTI_SHAPE,
             WGRAD_EXPECT["multi"])
    for _f in (5, 6, 7):
        _add("wgrad-groups-%d-%s" % (_f, _d), "k_upconv3x3_wgrad" + wgrad_form(_bf, None, False), case_wgrad, _bf,
             "plain", None, 256, 256, 128, False, (_f, 4, 32), WGRAD_EXPECT["groups-%d" % _f])
    # the C ABI through views
    for _w in ("fwd", "wgrad"):
        _k = "k_upconv3x3" if _w == "fwd" else "k_upconv3x3_wgrad"
        _f = fwd_form(_bf, "cell", True, False) if _w == "fwd" else wgrad_form(_bf, "cell", True)
        _add("abi-%s-off8-%s" % (_w, _d), _k + _f, case_abi_offsets, _bf, 8, _w)
        _add("abi-%s-off3-%s" % (_w, _d), _k + _f, case_abi_offsets, _bf, 3, _w)
        _add("abi-%s-strides-%s" % (_w, _d), _k + _f, case_abi_strides, _bf, _w)
        _add("abi-%s-ca0-%s" % (_w, _d), _k + _f, case_abi_ca0, _bf, _w)
    _add("abi-dgrad-strides-" + _d, "k_upconv3x3_dgrad" + dgrad_form(_bf, 24, 64), case_abi_dgrad, _bf)


def run_case(name):
    """{output name: digest} of a case, after its oracle and identity assertions."""
    fn, args = CASES[name]
    outs = fn(name, *args)
    torch.cuda.synchronize()
    return {k: T.digest(v) for k, v in outs.items()}


@functools.lru_cache(maxsize=None)
def _table():
    with open(TABLE) as fh:
        return json.load(fh)


def test_table_lists_every_case():
    t = _table()
    assert t["pinned_to"].startswith("self")
    assert sorted(t["cases"]) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_upconv_case(name):
    assert run_case(name) == _table()["cases"][name]
