"""The post-fusion BatchNorm kernels (shpl_batch_norm / shpl_batch_norm_backward:
k_bn_finalize, k_bn_apply[_vec], k_bn_bwd_partial[_vec], k_bn_bwd_finalize,
k_bn_bwd_apply[_vec]) on their own against the CPU oracle in double, in every
form the dispatch can reach, on MI355X.

The forward is fed per-channel statistics [sum x, sum x^2] computed on the
host in double with count = rows, so nothing of the conv is in the comparison.
bf16 inputs are rounded through the oracle's bf16 first: device and oracle read
the same values.

Which kernel runs is decided by `bn_vector_form` of csrc/shpl_bn.hip,
restated in vform() below: the 16-byte vector kernels need c a multiple of
VEC (4 f32 / 8 bf16 elements), stride a multiple of VEC, c / VEC a power of
two of at most SHPL_BLOCK = 256, and every map 16-byte aligned. Every entry
of CHANNELS states the form it selects; the module asserts that against the
predicate when it is imported.

Instances reached: k_bn_apply_vec<T, BETA, ACT> -- all 4 per dtype
(test_forward_vs_oracle). k_bn_bwd_apply_vec<T, ACT, HASY, BETA, TRAIN> -- the
dispatch hands the kernels beta only when act is ReLU and y is NULL, so of
the 16 instances per dtype 10 can be launched: ACT = 0 with HASY x TRAIN (4),
ACT = 1, HASY = 1 with TRAIN (2), ACT = 1, HASY = 0 with BETA x TRAIN (4);
test_backward_vs_oracle runs all 10 in both dtypes (the other 6 are BETA = 1
beside ACT = 0 or HASY = 1). The scalar kernels take the same switches at run
time and run the same matrix.

Bounds. Forward: 2^-20 * ((|x| + |mean|) * k + |beta|) per element with k =
|gamma| / sqrt(var + eps): at most 16 roundings of 2^-24 (mean and var to
f32, + eps, sqrt, divide, * gamma, subtract, multiply, add); bf16 storage adds
2^-8 * |y_ref|. Backward: the bounds of test_gpu_conv_grad.py, g_raw 1e-5 +
1e-5 * |scale| * (|g| + 1) (+ 2^-8 * |ref| in bf16), dbeta 1e-4 + 1e-6 * sum
|g|, dgamma 1e-4 + 1e-6 * sum |g * xhat|.

ReLU mask: the oracle masks in double, the device in f32, and a pre-activation
within rounding of zero can flip and move the sums by |g|. Nothing is left out
of the comparison: g is set to zero wherever |u| < 1e-3 (u = gamma * xhat +
beta in double), so the outputs do not depend on the mask there; at most 1 %
of the elements may be zeroed so (asserted).
"""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

from oracle import shpl_oracle as orc

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = 1e-3
BLOCK = 256  # SHPL_BLOCK
F32, BF16 = "f32", "bf16"
VEC = {F32: 4, BF16: 8}  # elements of a 16-byte piece
TORCH = {F32: torch.float32, BF16: torch.bfloat16}
NEAR = 1e-3  # |u| below which g is zeroed (module docstring)
SEED = 4  # checked on the host: no case of this seed zeroes more than 1 % of its elements (the worst: 0.4 %)


def vform(dt, c, stride=None, aligned=True):
    """The vector-form predicate of shpl_batch_norm / shpl_batch_norm_backward."""
    vec = VEC[dt]
    stride = c if stride is None else stride
    pr = c // vec
    return c % vec == 0 and stride % vec == 0 and pr <= BLOCK and (pr & (pr - 1)) == 0 and aligned


CHANNELS = [  # dtype, c, vector form
    (F32, 4, True),      # pr = 1: every thread a row lane
    (F32, 32, True),     # pr = 8: the training workload's channel count
    (F32, 64, True),     # pr = 16
    (F32, 1024, True),   # pr = 256 = SHPL_BLOCK: one row lane per block
    (F32, 7, False),     # scalar: 7 % 4 != 0
    (F32, 40, False),    # scalar: pr = 10 is no power of two
    (F32, 2048, False),  # scalar: pr = 512 > SHPL_BLOCK
    (BF16, 8, True),     # pr = 1
    (BF16, 32, True),    # pr = 4: the training workload's
    (BF16, 256, True),   # pr = 32
    (BF16, 2048, True),  # pr = 256 = SHPL_BLOCK: one row lane per block
    (BF16, 12, False),   # scalar: 12 % 8 != 0
    (BF16, 24, False),   # scalar: pr = 3 is no power of two
    (BF16, 4096, False),  # scalar: pr = 512 > SHPL_BLOCK
]
for _dt, _c, _v in CHANNELS:
    assert vform(_dt, _c) == _v, (_dt, _c)
CH_IDS = [f"{dt}-c{c}-{'vec' if v else 'scalar'}" for dt, c, v in CHANNELS]
VEC_CHANNELS = [e for e in CHANNELS if e[2]]
VEC_IDS = [i for i, e in zip(CH_IDS, CHANNELS) if e[2]]


def rows_for(c):
    """c = 32: one row (count 1), two, a count that ends the unrolled row loops mid-iteration, the
    bn_bwd_blocks boundary (4096: one partial block, 4097: two of 2049 rows), several blocks with ragged
    tails; wide rows: a few, and enough for several rows per lane."""
    if c == 32:
        return (1, 2, 63, 4096, 4097, 9001)
    return (37, 300) if c >= 1024 else (63, 300)


def _bf(a):
    return orc.from_bf16_bits(orc.to_bf16_bits(a))


def _frozen(**kw):
    for v in kw.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return types.SimpleNamespace(**kw)


@functools.lru_cache(maxsize=None)
def _data(dt, rows, c):
    """Inputs of one shape (host, read-only): x with its own mean and spread per channel, g, gamma with both
    signs and |gamma| >= 0.25, beta, moving statistics, and the host statistics of x in double."""
    rng = np.random.default_rng([SEED, rows, c, VEC[dt]])
    mu = rng.standard_normal(c)
    sig = rng.uniform(0.5, 3.0, c)
    x = (rng.standard_normal((rows, c)) * sig + mu).astype(np.float32)
    g = rng.standard_normal((rows, c)).astype(np.float32)
    gamma = (rng.uniform(0.25, 2.0, c) * np.where(rng.random(c) < 0.5, -1.0, 1.0)).astype(np.float32)
    beta = rng.standard_normal(c).astype(np.float32)
    beta[np.abs(beta) < 0.01] = 0.01
    if dt == BF16:
        x, g = _bf(x), _bf(g)
    x64 = x.astype(np.float64)
    stats = np.stack([x64.sum(0), (x64 * x64).sum(0)])
    mm0 = rng.standard_normal(c).astype(np.float32)
    mv0 = rng.uniform(0.5, 2.0, c).astype(np.float32)
    # inference: moving statistics near the data's, as after training
    imean = mu + 0.3 * sig * rng.standard_normal(c)
    ivar = sig * sig * rng.uniform(0.5, 2.0, c)
    return _frozen(x=x, x64=x64, g=g, gamma=gamma, beta=beta, stats=stats, mm0=mm0, mv0=mv0, imean=imean,
                   ivar=ivar)


def _host_moments(stats, rows):
    """mean and biased variance as k_bn_finalize forms them from the statistics (clamped at zero)."""
    mean = stats[0] / rows
    return mean, np.maximum(stats[1] / rows - mean * mean, 0.0)


@functools.lru_cache(maxsize=16)
def _ref_fwd(dt, rows, c, use_gamma, use_beta, relu):
    d = _data(dt, rows, c)
    y, bm, bv, mm, mv = orc.batch_norm_train(d.x64, EPS, d.gamma if use_gamma else None,
                                             d.beta if use_beta else None, relu, d.mm0, d.mv0, 0.999)
    return _frozen(y=y, bm=bm, bv=bv, mm=mm, mv=mv)


def _fwd_bound(dt, x, stats, rows, gamma, beta, y_ref):
    mean, var = _host_moments(stats, rows)
    k = (1.0 if gamma is None else np.abs(gamma.astype(np.float64))) / np.sqrt(var + EPS)
    b = 2.0 ** -20 * ((np.abs(x.astype(np.float64)) + np.abs(mean)) * k + (0.0 if beta is None else np.abs(beta)))
    if dt == BF16:
        b = b + 2.0 ** -8 * np.abs(y_ref)
    return b


@functools.lru_cache(maxsize=8)
def _bwd_case(dt, rows, c, relu, use_gamma, beta_in_u, training):
    """Inputs and oracle outputs of one backward case. u = gamma * xhat + beta is the pre-activation in
    double; g is zeroed where |u| < NEAR (ReLU only: without it no mask is taken)."""
    d = _data(dt, rows, c)
    gamma = d.gamma if use_gamma else None
    beta = d.beta if beta_in_u else None
    if training:
        mean, var = d.x64.mean(0), d.x64.var(0)
    else:
        mean, var = d.imean, d.ivar
    r = 1.0 / np.sqrt(var + EPS)
    gm = 1.0 if gamma is None else gamma.astype(np.float64)
    xhat = (d.x64 - mean) * r
    u = gm * xhat + (0.0 if beta is None else beta.astype(np.float64))
    g = d.g.copy()
    near = np.abs(u) < NEAR if relu else np.zeros(u.shape, bool)
    g[near] = 0.0
    e_raw, e_db, e_dg = orc.batch_norm_backward(d.x64, g, training, mean, var, EPS, gamma, beta, relu)
    y = (np.maximum(u, 0.0) if relu else u).astype(np.float32)
    if dt == BF16:
        y = _bf(y)
    return _frozen(x=d.x, g=g, y=y, gamma=gamma, beta=beta, mean32=mean.astype(np.float32),
                   scale32=(gm * r * np.ones(c)).astype(np.float32), xhat=xhat, frac=float(near.mean()),
                   e_raw=e_raw, e_db=e_db, e_dg=e_dg)


def _mask_ok(case, rows, relu, beta_in_u, training):
    """At most 1 % of the elements zeroed. One combination is degenerate: one row in training without beta
    has xhat = 0 and so u = 0 identically (every element is zeroed); there the mask is [0 > 0] on the device
    and in the oracle alike, with no rounding in it, and every output is exactly zero."""
    if rows == 1 and relu and training and not beta_in_u:
        return True
    return case.frac <= 0.01


def _t(a, dt=None):
    """Host array -> device tensor (the maps in dtype dt, parameters f32 / f64 as they are)."""
    if a is None:
        return None
    t = torch.from_numpy(np.array(a)).to(DEV)  # a copy: the cached arrays are read-only
    return t if dt is None else t.to(TORCH[dt])


def _np(t):
    return t.detach().float().cpu().numpy() if t.dtype == torch.bfloat16 else t.detach().cpu().numpy()


def _misaligned(t):
    """The same values in a view one element into a larger buffer: off 16-byte alignment -> scalar form."""
    buf = torch.empty(t.numel() + 16, dtype=t.dtype, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0
    return v


def _within(got, ref, bound, what):
    err = np.abs(np.asarray(got, np.float64) - ref)
    bad = ~(err <= bound)
    assert not bad.any(), (what, float(err.max()), float((err / bound).max()), int(bad.sum()))


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from sparse_pooling_amd import _lib as L
    L.lib()
    assert torch.cuda.is_available()


# ---------------------------------------------------------------- forward

def _run_fwd(dt, d, rows, c, use_gamma, use_beta, relu, x=None, in_place=True):
    from sparse_pooling_amd import fusion_conv as fc
    x = _t(d.x, dt) if x is None else x
    mm, mv = _t(d.mm0), _t(d.mv0)
    bm, bv = (torch.empty(c, dtype=torch.float32, device=DEV) for _ in range(2))
    ws = torch.empty(2 * c, dtype=torch.float32, device=DEV)
    out = None if in_place else torch.empty_like(x)
    y = fc.batch_norm_train(x, _t(d.stats), rows, eps=EPS, gamma=_t(d.gamma) if use_gamma else None,
                            beta=_t(d.beta) if use_beta else None, relu=relu, moving_mean=mm, moving_var=mv,
                            decay=0.999, batch_mean=bm, batch_var=bv, out=out, ws=ws)
    return y, mm, mv, bm, bv, ws


def _check_fwd(dt, d, rows, c, use_gamma, use_beta, relu, got, what):
    y, mm, mv, bm, bv, _ = got
    ref = _ref_fwd(dt, rows, c, use_gamma, use_beta, relu)
    bound = _fwd_bound(dt, d.x, d.stats, rows, d.gamma if use_gamma else None, d.beta if use_beta else None, ref.y)
    _within(_np(y), ref.y, bound, (what, "y"))
    np.testing.assert_allclose(_np(mm), ref.mm, rtol=1e-6, atol=1e-7, err_msg=str(what))
    np.testing.assert_allclose(_np(mv), ref.mv, rtol=1e-6, atol=1e-7, err_msg=str(what))
    np.testing.assert_allclose(_np(bm), ref.bm, rtol=1e-6, atol=1e-7, err_msg=str(what))
    np.testing.assert_allclose(_np(bv), ref.bv, rtol=1e-6, atol=1e-7, err_msg=str(what))


@pytest.mark.parametrize("use_gamma", [True, False], ids=["gamma", "nogamma"])
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "noact"])
@pytest.mark.parametrize("use_beta", [True, False], ids=["beta", "nobeta"])
@pytest.mark.parametrize("dt,c,vec", CHANNELS, ids=CH_IDS)
def test_forward_vs_oracle(dt, c, vec, use_beta, relu, use_gamma):
    """dtype x form x {beta, none} x {ReLU, none} x {gamma, none}: with the vector channel counts, the four
    k_bn_apply_vec<T, BETA, ACT> instances per dtype; with the others, k_bn_apply. Rows of rows_for(c), in
    place at odd row counts and into a second map at even ones (rows = 1: count 1, y = beta)."""
    for rows in rows_for(c):
        d = _data(dt, rows, c)
        got = _run_fwd(dt, d, rows, c, use_gamma, use_beta, relu, in_place=rows % 2 == 1)
        _check_fwd(dt, d, rows, c, use_gamma, use_beta, relu, got, (dt, c, rows))


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "noact"])
@pytest.mark.parametrize("dt,c,vec", [(F32, 32, True), (F32, 40, False), (BF16, 32, True), (BF16, 24, False)],
                         ids=["f32-c32-vec", "f32-c40-scalar", "bf16-c32-vec", "bf16-c24-scalar"])
def test_forward_constant_channel(dt, c, vec, relu):
    """A constant channel whose statistics give E[x^2] - mean^2 slightly below zero (the sum of squares a few
    ulps low, as another summation order can leave it): the clamp makes var = 0, x - mean = 0 exactly, and y
    is beta exactly (max(beta, 0) after ReLU); the other channels are untouched by it."""
    assert vform(dt, c) == vec
    rows, ch, v = 63, 5, np.float32(1.71875)  # exact in bf16
    d = _data(dt, rows, c)
    x = d.x.copy()
    x[:, ch] = v
    x64 = x.astype(np.float64)
    stats = np.stack([x64.sum(0), (x64 * x64).sum(0)])
    stats[1, ch] *= 1.0 - 2.0 ** -50
    mean = stats[0] / rows
    assert mean[ch] == v and stats[1, ch] / rows - mean[ch] * mean[ch] < 0.0  # the clamp runs
    dd = types.SimpleNamespace(x=x, stats=stats, gamma=d.gamma, beta=d.beta, mm0=d.mm0, mv0=d.mv0)
    y, mm, mv, bm, bv, ws = _run_fwd(dt, dd, rows, c, True, True, relu)
    ey, ebm, ebv, emm, emv = orc.batch_norm_train(x64, EPS, d.gamma, d.beta, relu, d.mm0, d.mv0, 0.999)
    _within(_np(y), ey, _fwd_bound(dt, x, stats, rows, d.gamma, d.beta, ey), "y")
    want = max(d.beta[ch], np.float32(0.0)) if relu else d.beta[ch]
    want = _bf(np.float32(want).reshape(1))[0] if dt == BF16 else want
    assert (_np(y)[:, ch] == want).all()
    assert _np(bv)[ch] == 0.0 and _np(bm)[ch] == v
    assert _np(ws)[ch] == v  # the mean the backward takes
    np.testing.assert_allclose(_np(bv), ebv, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(_np(mm), emm, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(_np(mv), emv, rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "noact"])
@pytest.mark.parametrize("use_beta", [True, False], ids=["beta", "nobeta"])
@pytest.mark.parametrize("dt,c,vec", VEC_CHANNELS, ids=VEC_IDS)
def test_forward_vector_equals_scalar_bitwise(dt, c, vec, use_beta, relu):
    """The same data from a 16-byte aligned map (vector form) and from a view one element into a larger buffer
    (misaligned: k_bn_apply): both do the same rounded operations per element, so y is bit-identical -- and
    so are the moving and batch statistics and the saved mean / scale, which k_bn_finalize writes."""
    for rows in rows_for(c):
        d = _data(dt, rows, c)
        x = _t(d.x, dt)
        assert x.data_ptr() % 16 == 0 and vform(dt, c, aligned=True) and not vform(dt, c, aligned=False)
        a = _run_fwd(dt, d, rows, c, True, use_beta, relu, x=x.clone())
        b = _run_fwd(dt, d, rows, c, True, use_beta, relu, x=_misaligned(x))
        for name, u, v in zip(("y", "moving_mean", "moving_var", "batch_mean", "batch_var", "ws"), a, b):
            assert torch.equal(u, v), (name, rows)
        _check_fwd(dt, d, rows, c, True, use_beta, relu, b, (dt, c, rows, "misaligned"))
        # only the output misaligned: scalar as well
        out = _misaligned(torch.empty_like(x))
        from sparse_pooling_amd import fusion_conv as fc
        fc.batch_norm_train(x, _t(d.stats), rows, eps=EPS, gamma=_t(d.gamma), beta=_t(d.beta) if use_beta else None,
                            relu=relu, out=out)
        assert torch.equal(out, a[0]), ("y misaligned", rows)


SENT = {F32: (torch.int32, 0x7FC0DEAD), BF16: (torch.int16, 0x7FC1)}  # NaN patterns no kernel here produces


def _strided(t, stride, dt):
    """The rows of t [rows, c] at a row stride of `stride` elements in a buffer filled with a sentinel bit
    pattern; returns (buffer [rows, stride], its integer view)."""
    ity, pat = SENT[dt]
    rows, c = t.shape
    buf = torch.empty((rows, stride), dtype=t.dtype, device=t.device)
    bits = buf.view(ity)
    bits.fill_(pat)
    buf[:, :c].copy_(t)
    return buf, bits


def _padding_intact(bits, c, dt):
    return bool((bits[:, c:] == SENT[dt][1]).all())


@pytest.mark.parametrize("in_place", [True, False], ids=["inplace", "outofplace"])
@pytest.mark.parametrize("pad", ["vec", 1], ids=["stride=c+vec:vector", "stride=c+1:scalar"])
@pytest.mark.parametrize("dt,c", [(F32, 32), (F32, 8), (BF16, 32), (BF16, 8)])
def test_forward_stride(dt, c, pad, in_place):
    """stride > c through the C ABI (the Python wrapper fixes stride = c): rows of c + VEC elements keep the
    vector form, rows of c + 1 must drop to the scalar one; both match the oracle and leave the padding
    columns' sentinel bits as they were, in place (d_y NULL) and into a second map."""
    from sparse_pooling_amd import _lib as L
    rows = 63
    stride = c + (VEC[dt] if pad == "vec" else 1)
    assert vform(dt, c, stride) == (pad == "vec")
    d = _data(dt, rows, c)
    xb, xbits = _strided(_t(d.x, dt), stride, dt)
    yb, ybits = _strided(torch.zeros((rows, c), dtype=TORCH[dt], device=DEV), stride, dt)
    ws = torch.empty(2 * c, dtype=torch.float32, device=DEV)
    mm, mv = _t(d.mm0), _t(d.mv0)
    bm, bv = (torch.empty(c, dtype=torch.float32, device=DEV) for _ in range(2))
    gamma, beta, stats = _t(d.gamma), _t(d.beta), _t(d.stats)
    L.check(L.lib().shpl_batch_norm(L.dtype_code(xb), rows, L.ptr(xb), None if in_place else L.ptr(yb), stride, c,
                                    L.ptr(stats), float(rows), EPS, L.ptr(gamma), L.ptr(beta), L.ACT_RELU,
                                    L.ptr(mm), L.ptr(mv), 0.999, L.ptr(bm), L.ptr(bv), L.ptr(ws),
                                    L.stream_of(xb.device)), "shpl_batch_norm")
    y = (xb if in_place else yb)[:, :c]
    _check_fwd(dt, d, rows, c, True, True, True, (y, mm, mv, bm, bv, ws), (dt, c, stride))
    assert _padding_intact(xbits, c, dt) and _padding_intact(ybits, c, dt)
    if not in_place:  # the input is read only
        assert torch.equal(xb[:, :c], _t(d.x, dt))


# ---------------------------------------------------------------- backward

YMODES = ["y", "raw+beta", "raw"]  # the mask from y; y NULL: from raw with beta, from raw without


def _run_bwd(dt, case, relu, ymode, training, g=None, x=None, y=None, bias_form=False):
    from sparse_pooling_amd import fusion_conv as fc
    g = _t(case.g, dt) if g is None else g
    x = _t(case.x, dt) if x is None else x
    if ymode == "y":
        y = _t(case.y, dt) if y is None else y
    else:
        y = None
    return fc.batch_norm_backward(g, y=y, raw=x, mean=None if bias_form else _t(case.mean32),
                                  scale=None if bias_form else _t(case.scale32), gamma=_t(case.gamma), relu=relu,
                                  training=training, beta=_t(case.beta) if ymode == "raw+beta" else None)


def _check_bwd(dt, case, got, what):
    gr, db, dg = got
    g64 = case.g.astype(np.float64)
    b_raw = 1e-5 + 1e-5 * np.abs(case.scale32.astype(np.float64)) * (np.abs(g64) + 1.0)
    if dt == BF16:
        b_raw = b_raw + 2.0 ** -8 * np.abs(case.e_raw)
    _within(_np(gr), case.e_raw, b_raw, (what, "g_raw"))
    _within(_np(db), case.e_db, 1e-4 + 1e-6 * np.abs(g64).sum(0), (what, "dbeta"))
    _within(_np(dg), case.e_dg, 1e-4 + 1e-6 * np.abs(g64 * case.xhat).sum(0), (what, "dgamma"))


@pytest.mark.parametrize("use_gamma", [True, False], ids=["gamma", "nogamma"])
@pytest.mark.parametrize("training", [True, False], ids=["training", "inference"])
@pytest.mark.parametrize("ymode", YMODES)
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "noact"])
@pytest.mark.parametrize("dt,c,vec", CHANNELS, ids=CH_IDS)
def test_backward_vs_oracle(dt, c, vec, relu, ymode, training, use_gamma):
    """dtype x form x {ReLU, none} x {y, y NULL with beta, y NULL without} x {training, inference} x {gamma,
    none}: g_raw, dbeta and dgamma against the oracle. With the vector channel counts these are the 10
    k_bn_bwd_apply_vec instances the dispatch can launch (module docstring) and k_bn_bwd_partial_vec; with the
    others k_bn_bwd_partial / k_bn_bwd_apply. Without ReLU y and beta are handed over and must be ignored.
    Rows of rows_for(c): 4096 is one partial block, 4097 two; one row in training has g_raw = 0 exactly."""
    beta_in_u = ymode != "raw"
    for rows in rows_for(c):
        case = _bwd_case(dt, rows, c, relu, use_gamma, beta_in_u, training)
        assert _mask_ok(case, rows, relu, beta_in_u, training), (rows, case.frac)
        got = _run_bwd(dt, case, relu, ymode, training)
        _check_bwd(dt, case, got, (dt, c, rows))
        if rows == 1 and training:
            assert not got[0].float().any(), "one row in training: g_raw is identically zero"


@pytest.mark.parametrize("ymode", YMODES)
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "noact"])
@pytest.mark.parametrize("dt,c,vec", CHANNELS, ids=CH_IDS)
def test_backward_bias_form(dt, c, vec, relu, ymode):
    """mean = scale = NULL (a conv bias in place of BatchNorm): g_raw = g_bn, bit for bit g under the mask
    [raw + bias > 0]; dbeta is the bias gradient, dgamma = sum g_bn * raw. The oracle's inference form with
    mean 0 and var = 1 - eps (scale 1) is the reference."""
    beta_in_u = ymode != "raw"
    for rows in rows_for(c):
        d = _data(dt, rows, c)
        beta = d.beta if beta_in_u else None
        u = d.x64 + (0.0 if beta is None else beta.astype(np.float64))
        g = d.g.copy()
        near = np.abs(u) < NEAR if relu else np.zeros(u.shape, bool)
        assert near.mean() <= 0.01
        g[near] = 0.0
        e_raw, e_db, e_dg = orc.batch_norm_backward(d.x64, g, False, np.zeros(c), np.full(c, 1.0 - EPS), EPS, None,
                                                    beta, relu)
        y = (np.maximum(u, 0.0) if relu else u).astype(np.float32)
        case = types.SimpleNamespace(x=d.x, g=g, y=_bf(y) if dt == BF16 else y, gamma=None, beta=beta,
                                     mean32=None, scale32=np.ones(c, np.float32), xhat=d.x64, e_raw=e_raw,
                                     e_db=e_db, e_dg=e_dg)
        got = _run_bwd(dt, case, relu, ymode, False, bias_form=True)
        _check_bwd(dt, case, got, (dt, c, rows, "bias"))
        want = np.where(u > 0.0, g, np.float32(0.0)) if relu else g
        assert np.array_equal(_np(got[0]), want), (rows, "g_raw = g_bn")


@pytest.mark.parametrize("use_gamma", [True, False], ids=["gamma", "nogamma"])
@pytest.mark.parametrize("training", [True, False], ids=["training", "inference"])
@pytest.mark.parametrize("dt,c,vec", CHANNELS, ids=CH_IDS)
def test_backward_mask_from_raw_equals_mask_from_y_bitwise(dt, c, vec, training, use_gamma):
    """The ReLU mask recomputed from raw (y NULL) is bitwise the mask read from y, in the vector and scalar
    forms, both dtypes, with gamma: all three outputs are equal bit for bit. Training: y, mean and scale are
    the device forward's (shpl_batch_norm and its workspace). Inference: y is (raw - mean) * scale + beta one
    rounded f32 operation at a time, as the forward kernels compute it, stored in the map's dtype."""
    from sparse_pooling_amd import fusion_conv as fc
    for rows in rows_for(c):
        d = _data(dt, rows, c)
        x, g, beta = _t(d.x, dt), _t(d.g, dt), _t(d.beta)
        gamma = _t(d.gamma) if use_gamma else None
        if training:
            ws = torch.empty(2 * c, dtype=torch.float32, device=DEV)
            y = fc.batch_norm_train(x, _t(d.stats), rows, eps=EPS, gamma=gamma, beta=beta, relu=True,
                                    out=torch.empty_like(x), ws=ws)
            mean, scale = ws[:c], ws[c:]
        else:
            gm = d.gamma.astype(np.float64) if use_gamma else 1.0
            mean = _t(d.imean.astype(np.float32))
            scale = _t((gm / np.sqrt(d.ivar + EPS)).astype(np.float32))
            y = torch.clamp_min((x.float() - mean) * scale + beta, 0.0).to(TORCH[dt])
        a1 = fc.batch_norm_backward(g, y=y, raw=x, mean=mean, scale=scale, gamma=gamma, relu=True, training=training)
        a2 = fc.batch_norm_backward(g, y=None, raw=x, mean=mean, scale=scale, gamma=gamma, relu=True,
                                    training=training, beta=beta)
        for name, u, v in zip(("g_raw", "dbeta", "dgamma"), a1, a2):
            assert torch.equal(u, v), (name, rows)


@pytest.mark.parametrize("training", [True, False], ids=["training", "inference"])
@pytest.mark.parametrize("ymode", ["y", "raw+beta"])
@pytest.mark.parametrize("dt,c,vec", VEC_CHANNELS, ids=VEC_IDS)
def test_backward_vector_vs_misaligned_scalar(dt, c, vec, ymode, training):
    """The same data aligned (vector kernels) and from views one element into larger buffers (scalar
    kernels). Inference: g_raw = scale * g_bn is bit-identical. Training, and dbeta / dgamma in both modes: the
    two forms group the partial sums differently, so each stays within its bound of the oracle."""
    for rows in rows_for(c):
        case = _bwd_case(dt, rows, c, True, True, True, training)
        g, x, y = _t(case.g, dt), _t(case.x, dt), _t(case.y, dt)
        a = _run_bwd(dt, case, True, ymode, training, g=g, x=x, y=y)
        b = _run_bwd(dt, case, True, ymode, training, g=_misaligned(g), x=_misaligned(x), y=_misaligned(y))
        _check_bwd(dt, case, a, (dt, c, rows, "aligned"))
        _check_bwd(dt, case, b, (dt, c, rows, "misaligned"))
        if not training:
            assert torch.equal(a[0], b[0]), rows
        # one misaligned map is enough to leave the vector form
        b1 = _run_bwd(dt, case, True, ymode, training, g=g, x=_misaligned(x), y=y)
        for u, v in zip(b, b1):
            assert torch.equal(u, v), rows


@pytest.mark.parametrize("training", [True, False], ids=["training", "inference"])
@pytest.mark.parametrize("ymode", ["y", "raw+beta"])
@pytest.mark.parametrize("pad", ["vec", 1], ids=["stride=c+vec:vector", "stride=c+1:scalar"])
@pytest.mark.parametrize("dt,c", [(F32, 32), (BF16, 32)])
def test_backward_stride(dt, c, pad, ymode, training):
    """stride > c through the C ABI: every map at a row stride of c + VEC (vector form) or c + 1 (scalar);
    the outputs match the oracle and the padding columns of g_raw, and of the inputs, keep their sentinel bits.
    4097 rows: two partial blocks."""
    from sparse_pooling_amd import _lib as L
    rows = 4097
    stride = c + (VEC[dt] if pad == "vec" else 1)
    assert vform(dt, c, stride) == (pad == "vec")
    case = _bwd_case(dt, rows, c, True, True, True, training)
    gb, gbits = _strided(_t(case.g, dt), stride, dt)
    xb, xbits = _strided(_t(case.x, dt), stride, dt)
    yb, ybits = _strided(_t(case.y, dt), stride, dt)
    ob, obits = _strided(torch.zeros((rows, c), dtype=TORCH[dt], device=DEV), stride, dt)
    dbeta, dgamma = (torch.empty(c, dtype=torch.float32, device=DEV) for _ in range(2))
    nb = ctypes.c_size_t()
    L.check(L.lib().shpl_batch_norm_backward_workspace_bytes(rows, c, ctypes.byref(nb)), "workspace_bytes")
    ws = L.workspace(nb.value, DEV)
    mean, scale, gamma, beta = _t(case.mean32), _t(case.scale32), _t(case.gamma), _t(case.beta)
    L.check(L.lib().shpl_batch_norm_backward(L.dtype_code(gb), rows, L.ptr(yb) if ymode == "y" else None, L.ptr(xb),
                                             L.ptr(gb), stride, c, L.ptr(mean), L.ptr(scale), L.ptr(gamma),
                                             L.ptr(beta) if ymode == "raw+beta" else None, L.ACT_RELU,
                                             int(training), L.ptr(ob), L.ptr(dbeta), L.ptr(dgamma), L.ptr(ws),
                                             nb.value, L.stream_of(gb.device)), "shpl_batch_norm_backward")
    _check_bwd(dt, case, (ob[:, :c], dbeta, dgamma), (dt, c, stride))
    for bits in (gbits, xbits, ybits, obits):
        assert _padding_intact(bits, c, dt)


def test_argument_errors():
    """stride < c: SHPL_ERR_BAD_SHAPE; an activation code other than NONE / RELU: SHPL_ERR_ARG; a workspace
    smaller than shpl_batch_norm_backward_workspace_bytes: SHPL_ERR_WORKSPACE (include/shpl.h). Each returns
    before anything is launched, and _lib.check raises on it."""
    from sparse_pooling_amd import _lib as L
    rows, c = 8, 32
    x = torch.zeros((rows, c), device=DEV)
    out = torch.zeros_like(x)
    stats = torch.ones((2, c), dtype=torch.float64, device=DEV)
    vec = torch.ones(c, device=DEV)
    dbeta, dgamma = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
    ws_f = torch.empty(2 * c, device=DEV)
    s = L.stream_of(x.device)

    def fwd(stride, act):
        return L.lib().shpl_batch_norm(L.F32, rows, L.ptr(x), L.ptr(out), stride, c, L.ptr(stats), float(rows), EPS,
                                       None, None, act, None, None, 0.999, None, None, L.ptr(ws_f), s)

    nb = ctypes.c_size_t()
    L.check(L.lib().shpl_batch_norm_backward_workspace_bytes(rows, c, ctypes.byref(nb)), "workspace_bytes")
    ws = L.workspace(nb.value, DEV)

    def bwd(stride, act, ws_bytes):
        return L.lib().shpl_batch_norm_backward(L.F32, rows, None, L.ptr(x), L.ptr(x), stride, c, L.ptr(vec),
                                                L.ptr(vec), None, None, act, 1, L.ptr(out), L.ptr(dbeta),
                                                L.ptr(dgamma), L.ptr(ws), ws_bytes, s)

    assert fwd(c, L.ACT_RELU) == L.OK and bwd(c, L.ACT_RELU, nb.value) == L.OK
    for rc, status in ((fwd(c - 1, L.ACT_RELU), L.ERR_BAD_SHAPE), (fwd(c, 2), L.ERR_ARG),
                       (bwd(c - 1, L.ACT_RELU, nb.value), L.ERR_BAD_SHAPE), (bwd(c, 2, nb.value), L.ERR_ARG),
                       (bwd(c, L.ACT_RELU, nb.value - 1), L.ERR_WORKSPACE)):
        assert rc == status
        with pytest.raises(L.ShplLibraryError):
            L.check(rc, "shpl_batch_norm")
    torch.cuda.synchronize()
