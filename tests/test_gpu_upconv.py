"""shpl_upconv3x3 / FusionUpconv / AfterVggFusion -- the after-VGG upconv3 (3x3 stride-2 transposed conv) with the
SHPL fused into its staging -- against the CPU oracle on MI355X.

Reference: the oracle's bit-exact fused map of each side (orc.sparse_pool_layer(dual=True), both outputs; inputs
and weights pre-rounded to bf16 for the bf16 cases, and the fused map rounded once to bf16 there -- which the
materialised map equals bitwise), then the definition in float64:
    out[f, oy, ox, co] = sum over (i, ky): 2i + ky = oy, (j, kx): 2j + kx = ox, ci of x[f, i, j, ci] W[ky, kx, co, ci]

Tolerance (derived, not tuned): any summation order of n f32 terms satisfies |err| <= 1.01 (n + 2) 2^-24 S, S the
same expression over absolute values. Forward: n = 4 (c_a + c_b) + L -- an output pixel sums at most 4 taps over
all input channels, L the longest run of the map under the side's key. A bf16 store adds |ref| 2^-8.

Training step (restating tests/test_gpu_conv_grad.py's chain for this op, with term counts instead of its fixed
2^-19 / 2^-16 factors). N = F 2h 2w rows. The device's raw output is off by d_raw <= the forward bound (bf16: with
its store). To first order (second-order terms are far below 1 % of these at the test's sizes; the 1.01 covers them):
    mean    d_mean <= mean(d_raw);   var  d_var <= 2 mean(|raw - mean| (d_raw + d_mean))
    scale s = (var + eps)^-1/2:      d_s <= s^3 d_var / 2
    xhat = (raw - mean) s:           d_xhat <= s (d_raw + d_mean) + |raw - mean| d_s
    y = relu(xhat + beta):           d_y <= d_xhat (ReLU is 1-Lipschitz) + 3 roundings + the store
    g_bn = g [y > 0]:                d_gbn = |g| where |xhat + beta| <= d_xhat (either mask may be the device's)
    m1 = mean(g_bn), m2 = mean(g_bn xhat):   d_m1 <= mean(d_gbn),  d_m2 <= mean(d_gbn |xhat| + |g_bn| d_xhat)
    g_raw = s (g_bn - m1 - xhat m2): d_graw <= d_s |g_bn - m1 - xhat m2| + s (d_gbn + d_m1 + d_xhat |m2| + |xhat| d_m2)
                                               + 8 roundings of s (|g_bn| + |m1| + |xhat m2|) + the store
    dbeta = sum g_bn:                sum(d_gbn) + the bound of N terms
The gradients are linear in g_raw: each takes its reference operator over (d_graw, |W|) or (|x|, d_graw), plus the
summation bound of its own sum over absolute values: the input gradient n = 36 c_out (the phase conv's 9 taps over
4 c_out channels), its pooled half stored (bf16) and pulled back with L more terms; the weight gradient n = F h w
(one product per input pixel and tap).
"""
import functools

import numpy as np
import pytest
import torch

import grouped_map as gm
from oracle import shpl_oracle as orc
from sparse_pooling_amd import synth

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
EPS = 1e-3


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def _rd(a):
    return orc.from_bf16_bits(orc.to_bf16_bits(a))


def _bound(S, n):
    return 1.01 * (n + 2) * U * S


def _within(what, got, ref, bound):
    d = np.abs(got.reshape(ref.shape) - ref)
    worst = float(np.max(d / np.maximum(bound, 1e-300))) if d.size else 0.0
    print(f"{what}: max |err| {float(d.max()) if d.size else 0.0:.3e}, max err/bound {worst:.3e}")
    bad = d > bound
    assert not bad.any(), f"{what}: {int(bad.sum())} of {d.size} outside the bound (worst err/bound {worst:.3f})"


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from sparse_pooling_amd import _lib as L
    L.lib()
    assert torch.cuda.is_available()


# ------------------------------------------------------------------ the definition, float64
def upconv_ref(x, w):
    """x [F,h,w,ci], w HWOI [3,3,co,ci] -> [F,2h,2w,co]: tap (ky, kx) of input (i, j) lands on output (2i+ky, 2j+kx)."""
    F, h, wd, _ = x.shape
    out = np.zeros((F, 2 * h, 2 * wd, w.shape[2]))
    for ky in range(3):
        for kx in range(3):
            hh, ww = (h if ky < 2 else h - 1), (wd if kx < 2 else wd - 1)
            out[:, ky:ky + 2 * hh:2, kx:kx + 2 * ww:2] += x[:, :hh, :ww] @ w[ky, kx].T
    return out


def upconv_dx(g, w):
    """The adjoint of upconv_ref in x: g [F,2h,2w,co] -> [F,h,w,ci]."""
    F, h2, w2, _ = g.shape
    h, wd = h2 // 2, w2 // 2
    out = np.zeros((F, h, wd, w.shape[3]))
    for ky in range(3):
        for kx in range(3):
            hh, ww = (h if ky < 2 else h - 1), (wd if kx < 2 else wd - 1)
            out[:, :hh, :ww] += g[:, ky:ky + 2 * hh:2, kx:kx + 2 * ww:2] @ w[ky, kx]
    return out


def upconv_dw(x, g):
    """The adjoint of upconv_ref in w: HWOI [3,3,co,ci]."""
    F, h, wd, ci = x.shape
    out = np.zeros((3, 3, g.shape[-1], ci))
    for ky in range(3):
        for kx in range(3):
            hh, ww = (h if ky < 2 else h - 1), (wd if kx < 2 else wd - 1)
            out[ky, kx] = np.einsum("fijo,fijc->oc", g[:, ky:ky + 2 * hh:2, kx:kx + 2 * ww:2], x[:, :hh, :ww])
    return out


# ------------------------------------------------------------------ the maps
def _small_P(im_size):
    P = synth.KITTI_P2.copy()
    P[0] *= im_size[0] / 1200.0
    P[1] *= im_size[1] / 360.0
    return P


def _frames_map(n_points, bev_hw, img_hw, seed):
    """Frames of n_points[f] points over a bev_hw BEV map and an img_hw image: the index builder's device map and
    the oracle's reference-format map of every frame."""
    from sparse_pooling_amd import pipeline, shpl_map as sm
    im_size, bv_size = (img_hw[1] * 8, img_hw[0] * 8), (bev_hw[0] * 2, bev_hw[1] * 2)
    P = _small_P(im_size)
    frames = [synth.make_frame(synth.FrameSpec(n, im_size, bv_size, (8, 2)), seed=seed + f, P=P)
              for f, n in enumerate(n_points)]
    spec = frames[0].spec
    assert spec.bev_feat_hw == tuple(bev_hw) and spec.img_feat_hw == tuple(img_hw)
    pts, vox, off, Pd, maxp, _ = pipeline.stack_frames(frames, DEV)
    ib = sm.build_index_batch(pts, vox, off, Pd, spec.im_size, spec.bv_size, spec.stride, maxp)
    refs = []
    for fr in frames:
        gen = orc.gen_sparse_pooling_input_avod(fr.points, fr.voxel_indices, fr.P, list(spec.im_size),
                                                tuple(spec.bv_size))
        r = orc.produce_sparse_pooling_input(gen, stride=spec.stride)
        refs.append((r["Mij_pool"], r["M_val"], r["M_size"], r["img_index_flip_pool"]))
    return ib.map, refs


def _packed(mij, mval, m_size, idx, img_shape):
    from sparse_pooling_amd import shpl_map as sm
    return sm.pack_map(_t(mij), _t(mval), m_size, _t(idx), img_shape), [(mij, mval, m_size, idx)]


CORNER_BEV, CORNER_IMG = (3, 5), (2, 4)


def _corner_map():
    """Hand-built: one column per image pixel (column k -> pixel k); entries in all four corner cells of the 3 x 5
    BEV map (0, 4, 10, 14) and a run of three at cell 7; the image corners (pixels 0, 3, 4, 7) are occupied too."""
    rows = [0, 4, 10, 14, 7, 7, 7, 2, 12]
    cols = [0, 3, 4, 7, 1, 2, 5, 0, 7]
    rng = np.random.default_rng(11)
    mij = np.stack([np.array(rows, np.int64), np.array(cols, np.int64)], 1)
    mval = _rd(rng.uniform(0.25, 2.0, len(rows)).astype(np.float32))
    idx = np.array([[0, k // 4, k % 4] for k in range(8)], np.int64)
    return mij, mval, np.array([15, 8], np.int64), idx, (1,) + CORNER_IMG


# name -> (map kind, c_a, c_b, c_out, sides)
CASES = {
    "corners-5+6-7": ("corners", 5, 6, 7, ("bev", "img")),           # channel tails everywhere, scalar loads, zero halo
    "grouped-16+32-32": ("grouped", 16, 32, 32, ("bev", "img")),     # the image side through ent_col groups
    # the kernel's tile is 8 x 32 input pixels: 9 x 35 is one row and three columns over a whole tile in each
    # dimension and spans two tiles in each; frames of 40 and 3 points: frame offsets, parity rows 2h-2 and 2h-1
    "ragged-2frames-32+16-64": ("ragged", 32, 16, 64, ("bev", "img")),
    "k256+256-128": ("wide", 256, 256, 128, ("bev", "img")),         # the real K loop, four output blocks
    "plain-32-32": ("plain", 32, 0, 32, ("bev",)),                   # c_b = 0, no pool
}
PARAMS = [(c, s, d) for c, v in CASES.items() for s in v[4] for d in ("f32", "bf16")]
IDS = [f"{c}-{s}-{d}" for c, s, d in PARAMS]
TRAIN = [p for p in PARAMS if p[0].startswith(("ragged", "grouped"))]
TRAIN_IDS = [f"{c}-{s}-{d}" for c, s, d in TRAIN]


class Case:
    pass


@functools.lru_cache(maxsize=None)
def _map(kind):
    if kind == "corners":
        m = _corner_map()
        smap, refs = _packed(*m)
        return smap, refs, CORNER_BEV, CORNER_IMG
    if kind == "grouped":
        m = gm.make()
        smap, refs = _packed(m["mij"], m["mval"], m["m_size"], m["idx"], m["img_shape"])
        return smap, refs, gm.BEV_HW, gm.IMG_HW
    n_points, bev_hw, img_hw = ((40, 3), (9, 35), (3, 10)) if kind in ("ragged", "plain") else ((60,), (5, 6), (3, 10))
    smap, refs = _frames_map(n_points, bev_hw, img_hw, seed=900)
    return smap, refs, bev_hw, img_hw


@functools.lru_cache(maxsize=None)
def _case(name, side, dtype):
    """Inputs, the device map and the float64 forward reference of one case, computed once and left unchanged."""
    kind, ca, cb, co, _ = CASES[name]
    bf = dtype == "bf16"
    c = Case()
    c.bf, c.dt, c.ca, c.cb, c.co, c.side, c.pooled = bf, torch.bfloat16 if bf else torch.float32, ca, cb, co, side, cb > 0
    c.smap, c.refs, bev_hw, img_hw = _map(kind)
    c.F = F = len(c.refs)
    c.a_hw, c.b_hw = (bev_hw, img_hw) if side == "bev" else (img_hw, bev_hw)
    rng = np.random.default_rng(list(CASES).index(name) * 2 + (side == "img") + 31)
    if kind == "grouped":
        img, bev = gm.features(cb if side == "bev" else ca, ca if side == "bev" else cb)
        a, b = (bev, img) if side == "bev" else (img, bev)
    else:
        a = rng.standard_normal((F,) + c.a_hw + (ca,)).astype(np.float32)
        b = rng.standard_normal((F,) + c.b_hw + (max(cb, 1),)).astype(np.float32)
    w = rng.uniform(-0.5, 0.5, (3, 3, co, ca + cb)).astype(np.float32)
    g = rng.standard_normal((F, 2 * c.a_hw[0], 2 * c.a_hw[1], co)).astype(np.float32)
    if bf:
        a, b, w, g = _rd(a), _rd(b), _rd(w), _rd(g)
    c.a, c.b, c.w, c.g = a, b, w, g

    # the longest run of the map under the side's key
    L = 0
    for mij, mval, m_size, idx in c.refs:
        mij, idx = np.asarray(mij).reshape(-1, 2), np.asarray(idx).reshape(-1, 3)
        if len(mij) and c.pooled:
            key = mij[:, 0] if side == "bev" else idx[mij[:, 1], 1] * img_hw[1] + idx[mij[:, 1], 2]
            L = max(L, int(np.bincount(key).max()))
    c.L = L

    def fused_of(av, bv, absval):
        """The oracle's fused map of this side: [a || pooled b], [F, h, w, ca + cb] f32."""
        if not c.pooled:
            return av
        out = []
        for f, (mij, mval, m_size, idx) in enumerate(c.refs):
            mv = np.abs(mval) if absval else mval
            bev_, img_ = (av, bv) if side == "bev" else (bv, av)
            fb, fi = orc.sparse_pool_layer(bev_[f:f + 1], img_[f:f + 1], mij, mv, m_size, idx, dual=True)
            out.append(fb if side == "bev" else fi)
        return np.concatenate(out)

    def pull_back(d, absval):
        """The oracle's gradient of the pooled half back to the pooled source: d [F,h,w,cb] -> b's shape."""
        out = []
        for f, (mij, mval, m_size, idx) in enumerate(c.refs):
            mv = np.abs(mval) if absval else mval
            df = np.ascontiguousarray(d[f:f + 1], np.float32)
            if side == "bev":
                o = orc.sparse_pool_grad_img(mij, mv, m_size, df.reshape(-1, cb), idx, (1,) + tuple(c.b_hw))
            else:
                o = orc.sparse_pool_trans_grad_bev(mij, mv, m_size, df, idx)
            out.append(o.reshape((1,) + tuple(c.b_hw) + (cb,)))
        return np.concatenate(out).astype(np.float64)

    c.pull_back = pull_back
    x = fused_of(a, b, False)
    c.x32 = _rd(x) if bf else x                  # the storage dtype's fused map (bf16: rounded once)
    c.x = c.x32.astype(np.float64)
    c.xabs = fused_of(np.abs(a), np.abs(b), True).astype(np.float64)
    c.W = w.astype(np.float64)
    c.store = (lambda ref: np.abs(ref) * 2.0 ** -8) if bf else (lambda ref: 0.0)
    c.raw = upconv_ref(c.x, c.W)
    c.S = upconv_ref(c.xabs, np.abs(c.W))
    c.raw_bound = _bound(c.S, 4 * (ca + cb) + L)
    return c


def _dev(c):
    ta = _t(c.a).to(c.dt)
    tb = _t(c.b).to(c.dt) if c.pooled else None
    return ta, tb, _t(c.w).to(c.dt)


def _side(c):
    from sparse_pooling_amd import fusion_conv as fc
    return fc.SIDE_BEV if c.side == "bev" else fc.SIDE_IMG


def _module(c, **kw):
    from sparse_pooling_amd import fusion_upconv as fu
    up = fu.FusionUpconv(c.ca + c.cb, c.co, dtype=c.dt, device=DEV, seed=5, **kw)
    assert tuple(up.weights.shape) == (3, 3, c.co, c.ca + c.cb) and up.weights.dtype == c.dt
    lim = np.sqrt(6.0 / (9 * (c.ca + c.cb) + 9 * c.co))  # xavier-uniform over the variable's fans
    assert float(up.weights.float().abs().max()) <= lim * 1.01
    up.weights = _t(c.w).to(c.dt)
    return up


def _fused(up, c, ta, tb, **kw):
    if not c.pooled:
        return up(ta, **kw)
    return (up.fused if c.side == "bev" else up.fused_img)(ta, tb, c.smap, **kw)


def test_corner_map_is_what_the_case_needs():
    mij, mval, m_size, idx, img_shape = _corner_map()
    cells = np.bincount(mij[:, 0], minlength=15)
    assert all(cells[r] > 0 for r in (0, 4, 10, 14)), "an entry in every corner cell"
    assert cells.max() >= 3, "a run of three entries"
    pix = np.bincount(idx[mij[:, 1], 1] * 4 + idx[mij[:, 1], 2], minlength=8)
    assert all(pix[p] > 0 for p in (0, 3, 4, 7))


@pytest.mark.parametrize("name,side,dtype", PARAMS, ids=IDS)
def test_forward(name, side, dtype):
    """shpl_upconv3x3 (pooled) against the definition over the oracle's fused map; bitwise the same call on the
    dense pulled map (c_a a whole number of staging chunks); d_stats; forward_phases within twice the bound."""
    from sparse_pooling_amd import fusion_upconv as fu, shpl_map as sm
    c = _case(name, side, dtype)
    ta, tb, tw = _dev(c)
    pool = c.smap.csr(*_side(c).fwd) if c.pooled else None
    fo = c.smap.frame_off if c.pooled else None
    st = torch.zeros((2, c.co), dtype=torch.float64, device=DEV)
    raw = fu.upconv3x3(ta, tw, b=tb, pool=pool, frame_off=fo, relu=False, stats=st)
    plain = fu.upconv3x3(ta, tw, b=tb, pool=pool, frame_off=fo, relu=False)
    assert tuple(raw.shape) == (c.F, 2 * c.a_hw[0], 2 * c.a_hw[1], c.co) and raw.dtype == c.dt
    up = _module(c, batch_norm=False, relu=False)
    y = _fused(up, c, ta, tb)
    yp = up.forward_phases(ta, tb, pool, fo)
    dense = None
    if c.pooled:
        mat = _side(c).pool(c.smap, tb, ta.shape[:3] + (c.cb,))
        dense = fu.upconv3x3(ta, tw, b=mat, relu=False)
        cat = torch.cat([ta, mat], -1)
        one = up(cat)
    torch.cuda.synchronize()
    assert c.smap.error_bits() == 0
    bound = c.raw_bound + c.store(c.raw)
    _within("raw", _np(raw), c.raw, bound)
    assert torch.equal(raw, plain), "taking statistics changes the output"
    assert torch.equal(y, raw), "FusionUpconv without an epilogue differs from the raw call"
    _within("fused vs phases", _np(y), _np(yp), 2 * bound)
    if c.pooled:
        np.testing.assert_array_equal(_np(cat).reshape(c.x.shape), c.x)  # the oracle's fused map, bitwise
        _within("dense pulled map", _np(dense), c.raw, bound)
        _within("materialised", _np(one), c.raw, bound)
        if c.ca % (16 if c.bf else 8) == 0:
            assert torch.equal(dense, raw), "the pooled call differs from the call on the dense pulled map"
            assert torch.equal(one, raw), "the pooled call differs from the call on the materialised concat"
    # statistics of the pre-epilogue output (f32 accumulators, not the stored values), the bound summed over rows
    flat, fb = c.raw.reshape(-1, c.co), c.raw_bound.reshape(-1, c.co)
    _within("stats sum", st[0].cpu().numpy(), flat.sum(0), fb.sum(0))
    _within("stats sumsq", st[1].cpu().numpy(), (flat ** 2).sum(0), ((2 * np.abs(flat) + fb) * fb).sum(0)
            + _bound((flat ** 2).sum(0), 1))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_epilogue(dtype):
    """BatchNorm inference with non-trivial moving statistics and beta: relu((raw - mean) * scale + beta), one
    rounding; and ReLU on the bit pattern: -0 -> +0, as shpl_conv3x3's."""
    from sparse_pooling_amd import fusion_upconv as fu
    c = _case("grouped-16+32-32", "bev", dtype)
    ta, tb, tw = _dev(c)
    rng = np.random.default_rng(77)
    up = _module(c)
    up.moving_mean.copy_(_t(rng.standard_normal(c.co).astype(np.float32)))
    up.moving_var.copy_(_t(rng.uniform(0.5, 4.0, c.co).astype(np.float32)))
    up.beta.copy_(_t(rng.standard_normal(c.co).astype(np.float32)))
    up._refresh_scale()
    y = _fused(up, c, ta, tb)
    torch.cuda.synchronize()
    sc, mm, beta = (_np(v) for v in (up._scale, up.moving_mean, up.beta))
    np.testing.assert_allclose(sc, 1.0 / np.sqrt(_np(up.moving_var) + EPS), rtol=4 * U)
    ref = np.maximum((c.raw - mm) * sc + beta, 0.0)
    mag = np.abs(c.raw) * sc + np.abs(mm) * sc + np.abs(beta)
    _within("BN inference", _np(y), ref, sc * c.raw_bound + _bound(mag, 3) + c.store(ref))
    assert float(_np(y).min()) >= 0.0 and float((_np(y) == 0).mean()) > 0.05
    # (+0) * -1 + (-0 - (-0 * -1)) = -0 + -0 = -0: stored as -0 without the activation, +0 (all bits clear) with it
    z = torch.zeros_like(ta)
    neg0 = torch.full((c.co,), -0.0, device=DEV)
    kw = dict(center=neg0, scale=-torch.ones(c.co, device=DEV), shift=neg0)
    ints = torch.int32 if dtype == "f32" else torch.int16
    keep = fu.upconv3x3(z, tw[..., :c.ca].contiguous(), relu=False, **kw).view(ints)
    act = fu.upconv3x3(z, tw[..., :c.ca].contiguous(), relu=True, **kw).view(ints)
    torch.cuda.synchronize()
    assert bool((keep < 0).all()) and bool((keep << 1 == 0).all()), "the epilogue's -0 is stored as -0"
    assert bool((act == 0).all()), "ReLU leaves a sign bit on -0"


def _train_reference(c, beta, mm0, mv0, decay=0.999):
    """The training step in float64 (torch CPU autograd over the oracle's fused map) and every bound of the module
    docstring."""
    ca, cb, co = c.ca, c.cb, c.co
    x = torch.from_numpy(c.x).requires_grad_(True)
    W = torch.from_numpy(c.W).requires_grad_(True)
    bt = torch.from_numpy(beta.astype(np.float64)).requires_grad_(True)
    conv = torch.nn.functional.conv_transpose2d(x.permute(0, 3, 1, 2), W.permute(3, 2, 0, 1), stride=2)
    raw = conv[..., :2 * x.shape[1], :2 * x.shape[2]].permute(0, 2, 3, 1)
    N = raw.numel() // co
    mean = raw.reshape(-1, co).mean(0)
    var = raw.reshape(-1, co).var(0, unbiased=False)
    s = (var + EPS).rsqrt()
    xhat = (raw - mean) * s
    y = torch.relu(xhat + bt)
    g = torch.from_numpy(c.g.astype(np.float64))
    (y * g).sum().backward()
    r = Case()
    r.y, r.mean, r.var_b = y.detach().numpy(), mean.detach().numpy(), var.detach().numpy() * N / (N - 1)
    r.mm = mm0 - (mm0 - r.mean) * (1 - decay)
    r.mv = mv0 - (mv0 - r.var_b) * (1 - decay)
    r.dx, r.dW, r.dbeta = x.grad.numpy(), W.grad.numpy(), bt.grad.numpy()
    np.testing.assert_allclose(raw.detach().numpy(), c.raw, rtol=0, atol=1e-9 * np.abs(c.raw).max())
    # ---- the bounds
    raw, s, xhat, mean = c.raw, s.detach().numpy(), xhat.detach().numpy(), r.mean
    gn = c.g.astype(np.float64)
    cm = lambda v: v.reshape(-1, co).mean(0)  # noqa: E731
    d_raw = c.raw_bound + c.store(raw)
    d_mean = cm(d_raw)
    d_var = 2 * cm(np.abs(raw - mean) * (d_raw + d_mean))
    d_s = s ** 3 * d_var / 2
    d_xhat = s * (d_raw + d_mean) + np.abs(raw - mean) * d_s
    pre = xhat + beta
    r.y_bound = d_xhat + _bound(np.abs(xhat) + np.abs(beta), 3) + c.store(r.y)
    r.mean_bound = d_mean + _bound(np.abs(mean), 1)
    r.var_bound = d_var * N / (N - 1) + _bound(r.var_b, 2)
    r.mm_bound = r.mean_bound * (1 - decay) + _bound(np.abs(mm0) + np.abs(r.mean), 3)
    r.mv_bound = r.var_bound * (1 - decay) + _bound(np.abs(mv0) + r.var_b, 3)
    g_bn = gn * (pre > 0)
    d_gbn = np.abs(gn) * (np.abs(pre) <= d_xhat + _bound(np.abs(xhat) + np.abs(beta), 3))
    m1, m2 = cm(g_bn), cm(g_bn * xhat)
    d_m1 = cm(d_gbn) + _bound(cm(np.abs(g_bn)), 1)
    d_m2 = cm(d_gbn * np.abs(xhat) + np.abs(g_bn) * d_xhat) + _bound(cm(np.abs(g_bn * xhat)), 2)
    g_raw = s * (g_bn - m1 - xhat * m2)
    mag = s * (np.abs(g_bn) + np.abs(m1) + np.abs(xhat * m2))
    d_graw = (d_s * np.abs(g_bn - m1 - xhat * m2) + s * (d_gbn + d_m1 + d_xhat * np.abs(m2) + np.abs(xhat) * d_m2)
              + _bound(mag, 8) + c.store(g_raw))
    r.dbeta_bound = d_gbn.reshape(-1, co).sum(0) + _bound(np.abs(g_bn).reshape(-1, co).sum(0), N)
    aW = np.abs(c.W)
    dx_bound = upconv_dx(d_graw, aW) + _bound(upconv_dx(np.abs(g_raw), aW), 36 * co)
    r.da, r.da_bound = r.dx[..., :ca], dx_bound[..., :ca] + c.store(r.dx[..., :ca])
    if c.pooled:
        dxb = r.dx[..., ca:]
        r.db = c.pull_back(dxb, False)
        r.db_bound = (c.pull_back(dx_bound[..., ca:] + c.store(dxb), True)
                      + _bound(c.pull_back(np.abs(dxb), True), c.L) + c.store(r.db))
    F, h, wd = c.x.shape[:3]
    r.dW_bound = (upconv_dw(np.abs(c.x), d_graw) + _bound(upconv_dw(np.abs(c.x), np.abs(g_raw)), F * h * wd)
                  + c.store(r.dW))
    return r


@pytest.mark.parametrize("name,side,dtype", TRAIN, ids=TRAIN_IDS)
def test_training_step(name, side, dtype):
    """FusionUpconv.fused / fused_img with is_training: the output, the batch moments through the updated moving
    statistics, and the gradients to both inputs, the weights and beta."""
    c = _case(name, side, dtype)
    rng = np.random.default_rng(5)
    beta = rng.standard_normal(c.co).astype(np.float32) * 0.5
    mm0 = rng.standard_normal(c.co).astype(np.float32)
    mv0 = rng.uniform(0.5, 2.0, c.co).astype(np.float32)
    # decay 0.5 (a constructor argument) instead of slim's 0.999: the batch moments are half of the updated moving
    # statistics, not a thousandth, so the check below sees them
    r = _train_reference(c, beta, mm0.astype(np.float64), mv0.astype(np.float64), decay=0.5)
    up = _module(c, decay=0.5)
    up.beta.copy_(_t(beta))
    up.moving_mean.copy_(_t(mm0))
    up.moving_var.copy_(_t(mv0))
    ta, tb, _ = _dev(c)
    leaves = [ta.requires_grad_(True), tb.requires_grad_(True), up.weights.requires_grad_(True),
              up.beta.requires_grad_(True)]
    y = _fused(up, c, ta, tb, is_training=True)
    y.backward(_t(c.g).to(c.dt))
    torch.cuda.synchronize()
    assert c.smap.error_bits() == 0
    da, db, dW, dbeta = (t.grad for t in leaves)
    assert da.dtype == c.dt and db.dtype == c.dt and dW.dtype == c.dt and dbeta.dtype == torch.float32
    assert tuple(dW.shape) == (3, 3, c.co, c.ca + c.cb) and tuple(db.shape) == tuple(tb.shape)
    _within("y", _np(y), r.y, r.y_bound)
    _within("moving_mean", _np(up.moving_mean), r.mm, r.mm_bound)
    _within("moving_var", _np(up.moving_var), r.mv, r.mv_bound)
    np.testing.assert_allclose(_np(up._scale), 1.0 / np.sqrt(_np(up.moving_var) + EPS), rtol=4 * U)
    _within("d_a", _np(da), r.da, r.da_bound)
    _within("d_b", _np(db), r.db, r.db_bound)
    _within("dW", _np(dW), r.dW, r.dW_bound)
    _within("dbeta", _np(dbeta), r.dbeta, r.dbeta_bound)


@pytest.mark.parametrize("dual", [True, False])
def test_after_vgg_fusion_equals_its_scopes(dual):
    """AfterVggFusion (the two scopes side by side on two streams) gives each scope's own bits."""
    from sparse_pooling_amd import fusion_upconv as fu
    c = _case("ragged-2frames-32+16-64", "bev", "bf16")
    bev, img, _ = _dev(c)
    av = fu.AfterVggFusion(c_bev=c.ca, c_img=c.cb, c_out=c.co, dual=dual, dtype=c.dt, device=DEV, seed=3)
    assert av.bev.c_in == c.ca + c.cb and av.img.c_in == c.cb + (c.ca if dual else 0)
    for training in (False, True):
        keep = [(m.moving_mean.clone(), m.moving_var.clone()) for m in (av.bev, av.img)]
        ob, oi = av(bev, img, c.smap, is_training=training)
        torch.cuda.synchronize()
        for m, (mm, mv) in zip((av.bev, av.img), keep):  # the scopes alone start from the same moving statistics
            m.moving_mean.copy_(mm)
            m.moving_var.copy_(mv)
            m._refresh_scale()
        rb = av.bev.fused(bev, img, c.smap, is_training=training)
        ri = av.img.fused_img(img, bev, c.smap, is_training=training) if dual else av.img(img, is_training=training)
        torch.cuda.synchronize()
        assert tuple(ob.shape) == (c.F, 18, 70, c.co) and tuple(oi.shape) == (c.F, 6, 20, c.co)
        assert torch.equal(ob, rb) and torch.equal(oi, ri)


def test_inference_call_is_capturable():
    """An inference .fused call recorded with torch.cuda.graph on a side stream and replayed twice gives the
    eager bits: no allocation, no host synchronisation inside the library call."""
    c = _case("ragged-2frames-32+16-64", "bev", "bf16")
    bev, img, _ = _dev(c)
    up = _module(c)
    eager = up.fused(bev, img, c.smap)  # builds the CSR and the module's workspace outside the capture
    out = torch.empty_like(eager)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            up.fused(bev, img, c.smap, out=out)
    torch.cuda.synchronize()
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
