"""The 1x1 head kernels (shpl_head.hip, shpl_head_drop.hip) pinned bit for bit on MI355X, one case per dispatch
form: the K loop's three exits, every padded c_out, a dense and a pooled second source, one source, channel
tails, more than one GEMM workgroup and input-gradient block, grid.y of 2, the weight gradient's chunking above its
minimum and a second batch trip, strided and offset operands (aligned and not), and the same under dropout.

A case calls the C entry points directly (forward, input gradient, weight gradient) and makes three kinds of
assertion:

1. The oracle bound. Cases over a case of test_gpu_head.py use its float64 references and bounds (and
   test_gpu_head_dropout._ref's under dropout), imported. The other cases state theirs in `_own_ref` by the same
   rule -- a sum of n f32 terms in any order with k further roundings: |err| <= 1.01 (n + k) 2^-24 S, S the
   expression over absolute values, plus |ref| 2^-8 for a bf16 store:
       plain     forward n = c_a + c_b + L, inputs n = c_out + L, dw n = the rows a channel sums + L, k = 2
       dropout   forward n = c_a + c_b, k = 3; d_a n = c_out, k = 1; pooled d_b n = c_out + L, k = 2; dw n = rows, k = 2
       dbias     n = rows + L, k = 2
   (L: the longest run of the map, 0 without one; dw and dbias are f32: no store term.)
2. Bitwise identities: two runs; operands cut at channel offset 8 (16-byte aligned) and 3 (not) from tensors 8
   channels wider against their contiguous copies; a CSR without key_range against one with it; the raw calls
   against FusionHead.fused / fused_dropout and their autograd; each input gradient alone against both, and the
   weight gradient without the bias gradient against the one with it; at keep_prob 1 another seed.
3. The SHA-256 of every output's bytes equals tests/golden/head_bits.json (tests/golden/make_head_bits.py, which
   runs these same case functions), recorded from the library before the heads' clean-up (docs/HISTORY.md §13).
"""
import ctypes
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import dropout_mask_ref as mref
import grouped_map as gm
import test_gpu_head as base
import test_gpu_head_dropout as drop
from oracle import shpl_oracle as orc

pytestmark = pytest.mark.gpu

DEV = base.DEV
U = 2.0 ** -24
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "head_bits.json")
SEED, OTHER_SEED = drop.SEED, drop.OTHER_SEED
_t, _rd, _within = base._t, base._rd, base._within


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from sparse_pooling_amd import _lib as L
    L.lib()
    assert torch.cuda.is_available()


# ------------------------------------------------------------------ operands and the raw calls
class View:
    """Channels [off, off + c) of the rows of a 2-D tensor `t`."""

    def __init__(self, t, off, c):
        assert t.dim() == 2 and t.is_contiguous() and 0 <= off and off + c <= t.shape[1]
        self.t, self.off, self.c, self.stride = t, off, c, int(t.shape[1])

    def start(self):
        return ctypes.c_void_p(self.t.data_ptr() + self.off * self.t.element_size())

    def get(self):
        return self.t[:, self.off:self.off + self.c].contiguous()


def _view(x, off):
    """x [rows, c] as it is (off None), or cut at channel `off` from a tensor 8 channels wider."""
    if off is None:
        return View(x.contiguous(), 0, int(x.shape[1]))
    wide = torch.full((x.shape[0], x.shape[1] + 8), 3.0, dtype=x.dtype, device=x.device)
    wide[:, off:off + x.shape[1]] = x
    return View(wide, off, int(x.shape[1]))


def _blank(rows, c, dt, off):
    """An output of NaNs: [rows, c], or that slice of a tensor 8 channels wider."""
    t = torch.full((rows, c if off is None else c + 8), float("nan"), dtype=dt, device=DEV)
    return View(t, off or 0, c)


def _taken(v):
    """The output a call wrote into the view; nothing outside it was touched."""
    outside = torch.ones(v.t.shape[1], dtype=torch.bool, device=v.t.device)
    outside[v.off:v.off + v.c] = False
    assert bool(torch.isnan(v.t[:, outside]).all()), "a store outside the output's channels"
    got = v.get()
    assert not bool(torch.isnan(got).any()), "an element of the output was not written"
    return got


class Ops:
    """One case's operands on the device: a [rows, ca], b [rows_b, cb] or None, w [ca + cb, co], bias f32 [co],
    gy [rows, co]; pool_fwd / pool_grad: the cell- and the pixel-keyed CSR of the pooled form, or None."""
    pool_fwd = pool_grad = c = None


def _mask_args(kp, seed):
    from sparse_pooling_amd import fusion_head as fh
    return [] if kp is None else [float(kp), fh._u64(seed)]


def _ws(d, pooled, kp, wgrad):
    from sparse_pooling_amd import _lib as L, fusion_head as fh
    q = fh.head_ws_bytes if kp is None else fh.head_drop_ws_bytes
    return L.workspace(q(L.dtype_code(d.a), d.rows, d.ca, d.rows_b, d.cb, d.co, pooled, wgrad=wgrad), DEV)


def _src_args(v):
    return [None, 0, 0, 0] if v is None else [ctypes.c_void_p(v.t.data_ptr()), v.stride, v.off, v.c]


def raw_forward(d, a, b, pool, kp, seed, out):
    from sparse_pooling_amd import _lib as L
    name = "shpl_head1x1" if kp is None else "shpl_head1x1_drop"
    ws = _ws(d, pool is not None, kp, False)
    L.check(getattr(L.lib(), name)(L.dtype_code(d.a), d.rows, *_src_args(a), *_src_args(b), d.rows_b,
                                   None if pool is None else pool.ref(), L.ptr(d.w), d.co, L.ptr(d.bias), out.start(),
                                   out.stride, *_mask_args(kp, seed), L.ptr(ws), ws.numel(), L.stream_of(DEV)), name)
    return _taken(out)


def raw_dgrad(d, gy, pool_grad, kp, seed, da, db):
    """(d_a, d_b); da / db: the output views, None for a gradient that is not wanted."""
    from sparse_pooling_amd import _lib as L
    name = "shpl_head1x1_dgrad" if kp is None else "shpl_head1x1_drop_dgrad"
    ws = _ws(d, pool_grad is not None, kp, False)
    L.check(getattr(L.lib(), name)(L.dtype_code(d.a), d.rows, gy.start(), gy.stride, d.co, L.ptr(d.w), d.ca, d.cb,
                                   None if da is None else da.start(), d.ca if da is None else da.stride,
                                   None if db is None else db.start(), max(d.cb, 1) if db is None else db.stride,
                                   d.rows_b, None if pool_grad is None else pool_grad.ref(), *_mask_args(kp, seed),
                                   L.ptr(ws), ws.numel(), L.stream_of(DEV)), name)
    return None if da is None else _taken(da), None if db is None else _taken(db)


def raw_wgrad(d, a, b, gy, pool, kp, seed, bias=True):
    """(dw, dbias); pool: the pixel-keyed CSR for the plain form, the forward's cell-keyed one under dropout."""
    from sparse_pooling_amd import _lib as L
    name = "shpl_head1x1_wgrad" if kp is None else "shpl_head1x1_drop_wgrad"
    ws = _ws(d, pool is not None, kp, True)
    dw = torch.full((d.ca + d.cb, d.co), float("nan"), dtype=torch.float32, device=DEV)
    dbias = torch.full((d.co,), float("nan"), dtype=torch.float32, device=DEV) if bias else None
    L.check(getattr(L.lib(), name)(L.dtype_code(d.a), d.rows, *_src_args(a), *_src_args(b), d.rows_b,
                                   None if pool is None else pool.ref(), gy.start(), gy.stride, d.co, L.ptr(dw),
                                   L.ptr(dbias), *_mask_args(kp, seed), L.ptr(ws), ws.numel(), L.stream_of(DEV)), name)
    return dw, dbias


def _outputs(d, kp, seed, off=None, pools=None):
    """Every output of the three raw calls over d's operands (cut at channel `off` from wider tensors)."""
    pool_fwd, pool_grad = pools or (d.pool_fwd, d.pool_grad)
    a, gy = _view(d.a, off), _view(d.gy, off)
    b = None if d.b is None else _view(d.b, off)
    o = {"out": raw_forward(d, a, b, pool_fwd, kp, seed, _blank(d.rows, d.co, d.a.dtype, off))}
    o["d_a"], d_b = raw_dgrad(d, gy, pool_grad, kp, seed, _blank(d.rows, d.ca, d.a.dtype, off),
                              None if d.b is None else _blank(d.rows_b, d.cb, d.a.dtype, off))
    if d_b is not None:
        o["d_b"] = d_b
    o["dw"], o["dbias"] = raw_wgrad(d, a, b, gy, pool_fwd if kp is not None else pool_grad, kp, seed)
    return o


def _same(what, got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        assert torch.equal(got[k], want[k]), f"{what}: {k} differs"


# ------------------------------------------------------------------ references
class Ref:
    pass


def _own_ref(x, xabs, W, B, G, ca, bf, kp, seed, L=0, to_pixels=None, n_b=None):
    """The float64 references and bounds of the module docstring. x [rows, ca + cb]: the map the heads see, [a || b]
    or the oracle's bv_fused (xabs: the same over absolute values); to_pixels(dY, absval): the image half of a
    gradient pulled back to the pixels; n_b: the rows a b-channel of dw sums (the pixels of the pooled form)."""
    rows, cc = x.shape
    co = W.shape[1]
    aW, aG, pooled = np.abs(W), np.abs(G), to_pixels is not None
    store = (lambda ref: np.abs(ref) * 2.0 ** -8) if bf else (lambda ref: 0.0)

    def bound(S, n, k):
        return 1.01 * (n + k) * U * S

    r = Ref()
    if kp is None:
        K, s = 1.0, 1.0
        (nf, kf), (nd, kd), ndb = (cc + L, 2), (co + L, 2), co + L
        nw = np.concatenate([np.full(ca, rows), np.full(cc - ca, rows if n_b is None else n_b)]).reshape(-1, 1) + L
    else:
        K, s = mref.mask(rows, cc, kp, seed).astype(np.float64), mref.scale(kp)
        if bf and pooled:  # the pooled operand is the run sum rounded to bf16; in f32 it is the run sum itself
            x = _rd(x.astype(np.float32)).astype(np.float64)
        xabs = np.abs(x)
        (nf, kf), (nd, kd), ndb, nw = (cc, 3), (co, 1), co + L, rows
    r.out = s * ((K * x) @ W) + B
    r.out_bound = bound(s * ((K * xabs) @ aW) + np.abs(B), nf, kf) + store(r.out)
    d_x, d_abs = s * K * (G @ W.T), s * K * (aG @ aW.T)
    r.d_a = d_x[:, :ca]
    r.d_a_bound = bound(d_abs[:, :ca], nd, kd) + store(r.d_a)
    if cc > ca:
        r.d_b = to_pixels(d_x[:, ca:], False) if pooled else d_x[:, ca:]
        r.d_b_bound = (bound(to_pixels(d_abs[:, ca:], True), ndb, 2) if pooled else bound(d_abs[:, ca:], nd, kd)) \
            + store(r.d_b)
    r.dW = s * ((K * x).T @ G)
    r.dW_bound = bound(s * ((K * xabs).T @ aG), nw, 2)
    r.dB = G.sum(0)
    r.dB_bound = bound(aG.sum(0), rows + L, 2)
    return r


def _base_ref(name, dtype, kp):
    """The references of a case of test_gpu_head.py, as it and test_gpu_head_dropout.py hold them."""
    c = base._case(name, dtype)
    r = Ref()
    if kp is None:
        r.out, r.out_bound, r.d_a, r.d_a_bound = c.out, c.out_bound, c.d_lidar, c.d_lidar_bound
        r.d_b, r.d_b_bound, r.dW, r.dW_bound = c.d_img, c.d_img_bound, c.dW, c.dW_bound
    else:
        d = drop._ref(name, kp, dtype)
        r.out, r.out_bound, r.d_a, r.d_a_bound = d.out, d.out_bound, d.d_x[:, :c.ca], d.d_x_bound[:, :c.ca]
        r.d_b, r.d_b_bound, r.dW, r.dW_bound = d.d_img, d.d_img_bound, d.dW, d.dW_bound
    r.dB, r.dB_bound = c.dB, c.dB_bound
    return r


def _held(what, o, r):
    f64 = base._np
    _within(what + " out", f64(o["out"]), r.out, r.out_bound)
    _within(what + " d_a", f64(o["d_a"]), r.d_a, r.d_a_bound)
    if "d_b" in o:
        _within(what + " d_b", f64(o["d_b"]), r.d_b, r.d_b_bound)
    _within(what + " dw", f64(o["dw"]), r.dW, r.dW_bound)
    _within(what + " dbias", f64(o["dbias"]), r.dB, r.dB_bound)


# ------------------------------------------------------------------ the cases over a map
FRAMES = {"frames266": (3, 10), "frames266-img27": (3, 9)}  # kind -> the image map's (H, W); BEV 7 x 19, 2 frames
FRAMES_POINTS, FRAMES_BEV = (120, 2), (7, 19)               # one sparse frame


def _runs(refs, R, img_hw):
    """Entries per cell and per pixel of a batch of reference-format maps, over the batch's rows."""
    Pn = img_hw[0] * img_hw[1]
    cells, pix = np.zeros(len(refs) * R, np.int64), np.zeros(len(refs) * Pn, np.int64)
    for f, (mij, mval, m_size, idx) in enumerate(refs):
        mij, idx = np.asarray(mij).reshape(-1, 2), np.asarray(idx).reshape(-1, 3)
        if len(mij):
            cells += np.bincount(f * R + mij[:, 0], minlength=len(cells))
            pix += np.bincount(f * Pn + idx[mij[:, 1], 1] * img_hw[1] + idx[mij[:, 1], 2], minlength=len(pix))
    return cells, pix


@functools.lru_cache(maxsize=None)
def _map_case(kind, ca, cb, heads, dtype):
    """A case in the shape of test_gpu_head.Case (inputs, the device map, the oracle's bv_fused), for the maps and
    head widths that module has no case of."""
    bf = dtype == "bf16"
    c = base.Case()
    c.bf, c.dt, c.ca, c.cb, c.heads = bf, torch.bfloat16 if bf else torch.float32, ca, cb, heads
    rng = np.random.default_rng(sum(heads) * 131 + ca)
    if kind == "grouped":
        c.smap, c.refs, c.rebuild = base._grouped_map()
        img, lidar = gm.features(cb, ca)
        c.bev_hw, c.img_hw = gm.BEV_HW, gm.IMG_HW
    else:
        c.bev_hw, c.img_hw = FRAMES_BEV, FRAMES[kind]
        c.smap, c.refs, c.rebuild = base._frames_map(FRAMES_POINTS, c.bev_hw, c.img_hw, seed=900)
        F = len(FRAMES_POINTS)
        lidar = rng.standard_normal((F,) + c.bev_hw + (ca,)).astype(np.float32)
        img = rng.standard_normal((F,) + c.img_hw + (cb,)).astype(np.float32)
    F, R, Pn = len(c.refs), int(np.prod(c.bev_hw)), int(np.prod(c.img_hw))
    c.F, c.R, c.Pn = F, R, Pn
    cells, pix = _runs(c.refs, R, c.img_hw)
    c.L = int(max(cells.max(), pix.max()))
    if kind != "grouped":  # what the case is there for, from the oracle-format map
        assert F * R == 266 and F * R > 2 * 128 and (F * R) % 32 != 0
        assert any(cells[t:t + 32].sum() == 0 for t in range(0, F * R, 32)), "no 32-row tile without an entry"
        assert (cells % 2 == 1).any() and (pix % 2 == 1).any(), "no run of odd length"
        assert (pix == 0).any() and (cells == 0).any()
        assert (F * Pn) % 4 == (0 if kind == "frames266" else 2)
    w = [rng.uniform(-0.5, 0.5, (1, 1, ca + cb, n)).astype(np.float32) for n in heads]
    bias = [rng.standard_normal(n).astype(np.float32) * 0.5 for n in heads]
    g = [rng.standard_normal((F,) + c.bev_hw + (n,)).astype(np.float32) for n in heads]
    if bf:
        lidar, img, w, g = _rd(lidar), _rd(img), [_rd(v) for v in w], [_rd(v) for v in g]
    c.lidar, c.img, c.w, c.bias, c.g = lidar, img, w, bias, g
    c.W = np.concatenate([v.reshape(ca + cb, -1) for v in w], 1).astype(np.float64)
    c.B = np.concatenate(bias).astype(np.float64)
    c.G = np.concatenate([v.reshape(-1, v.shape[-1]) for v in g], 1).astype(np.float64)

    def fused_of(lid, im, absval):
        out = []
        for f, (mij, mval, m_size, idx) in enumerate(c.refs):
            bv, _ = orc.sparse_pool_layer(lid[f:f + 1], im[f:f + 1], mij, np.abs(mval) if absval else mval, m_size, idx)
            out.append(bv.reshape(R, ca + cb))
        return np.concatenate(out).astype(np.float64)

    def to_pixels(dY, absval):  # entry (cell, column) of frame f adds m * dY[cell] to the pixel of its column
        out = np.zeros((F * Pn, dY.shape[1]))
        for f, (mij, mval, m_size, idx) in enumerate(c.refs):
            mij, idx = np.asarray(mij).reshape(-1, 2), np.asarray(idx).reshape(-1, 3)
            if len(mij):
                mv = np.asarray(mval, dtype=np.float64)
                at = idx[mij[:, 1], 1] * c.img_hw[1] + idx[mij[:, 1], 2]
                np.add.at(out, f * Pn + at, (np.abs(mv) if absval else mv)[:, None] * dY[f * R + mij[:, 0]])
        return out

    c.fused, c.fabs, c.to_pixels = fused_of(lidar, img, False), fused_of(np.abs(lidar), np.abs(img), True), to_pixels
    return c


def _map_ops(c):
    from sparse_pooling_amd import _lib as L
    d = Ops()
    d.c, d.ca, d.cb, d.co = c, c.ca, c.cb, sum(c.heads)
    d.rows, d.rows_b = c.F * c.R, c.F * c.Pn
    d.a, d.b = _t(c.lidar).to(c.dt).reshape(d.rows, c.ca), _t(c.img).to(c.dt).reshape(d.rows_b, c.cb)
    d.w = torch.cat([_t(w).to(c.dt).reshape(c.ca + c.cb, -1) for w in c.w], 1).contiguous()
    d.bias = torch.cat([_t(b) for b in c.bias])
    d.gy = torch.cat([_t(g).to(c.dt).reshape(d.rows, -1) for g in c.g], 1).contiguous()
    d.pool_fwd, d.pool_grad = c.smap.csr(L.BY_CELL, L.ORDER_ENTRY), c.smap.csr(L.BY_PIXEL, L.ORDER_COL_ENTRY)
    assert d.pool_fwd.key_range is not None
    return d


def _method(c, kp, seed):
    """The same outputs through FusionHead.fused / fused_dropout and autograd."""
    head = base._head(c)
    tl, ti = _t(c.lidar).to(c.dt).requires_grad_(True), _t(c.img).to(c.dt).requires_grad_(True)
    for p in (*head.weights, *head.biases):
        p.requires_grad_(True)
        p.grad = None
    outs = head.fused(tl, ti, c.smap) if kp is None else head.fused_dropout(tl, ti, c.smap, kp, seed=seed)
    torch.autograd.backward(outs, [_t(g).to(c.dt) for g in c.g])
    cc = c.ca + c.cb
    return {"out": base._cat(outs).detach(), "d_a": tl.grad.reshape(-1, c.ca), "d_b": ti.grad.reshape(-1, c.cb),
            "dw": torch.cat([w.grad.reshape(cc, -1) for w in head.weights], 1),
            "dbias": torch.cat([b.grad for b in head.biases])}


def case_map(kind, ca, cb, heads, dtype, kp, seed=SEED, strided=False):
    from sparse_pooling_amd import _lib as L
    name = ("k768+768" if kind == "k768" else f"{kind}-{ca}+{cb}") + "-" + ",".join(str(n) for n in heads)
    own = name not in base.CASES
    c = _map_case(kind, ca, cb, heads, dtype) if own else base._case(name, dtype)
    d = _map_ops(c)
    o = _outputs(d, kp, seed)
    _same("a second run", _outputs(d, kp, seed), o)
    flat = c.rebuild()
    flat.ROW_PULLS = False  # the CSRs of the flat builders: no key_range, the calls build the ranges themselves
    pools = (flat.csr(L.BY_CELL, L.ORDER_ENTRY), flat.csr(L.BY_PIXEL, L.ORDER_COL_ENTRY))
    assert pools[0].key_range is None
    _same("a CSR without key_range", _outputs(d, kp, seed, pools=pools), o)
    m = _method(c, kp, seed)
    _same("FusionHead", m, dict(o, dw=o["dw"].to(c.dt)))
    if strided:
        for off in (8, 3):
            _same(f"cut at channel {off}", _outputs(d, kp, seed, off=off), o)
    if kp == 1.0:
        _same("another seed at keep_prob 1", _outputs(d, kp, OTHER_SEED), o)
    torch.cuda.synchronize()
    assert c.smap.error_bits() == 0 and flat.error_bits() == 0
    if own:
        r = _own_ref(c.fused, c.fabs, c.W, c.B, c.G, ca, c.bf, kp, seed, L=c.L, to_pixels=c.to_pixels, n_b=c.F * c.Pn)
    else:
        r = _base_ref(name, dtype, kp)
    _held(name, o, r)
    return o


# ------------------------------------------------------------------ the dense cases
def case_dense(rows, ca, cb, co, dtype, kp, seed=SEED, strided=False):
    """One source (cb 0) or a dense second source of as many rows."""
    bf = dtype == "bf16"
    dt = torch.bfloat16 if bf else torch.float32
    rng = np.random.default_rng(rows * 7 + ca * 3 + cb)
    x = rng.standard_normal((rows, ca + cb)).astype(np.float32)
    w = rng.uniform(-0.5, 0.5, (ca + cb, co)).astype(np.float32)
    bias = rng.standard_normal(co).astype(np.float32) * 0.5
    g = rng.standard_normal((rows, co)).astype(np.float32)
    if bf:
        x, w, g = _rd(x), _rd(w), _rd(g)
    d = Ops()
    d.rows = d.rows_b = rows
    d.ca, d.cb, d.co = ca, cb, co
    d.a = _t(x[:, :ca]).to(dt)
    d.b = _t(x[:, ca:]).to(dt) if cb else None
    d.w, d.bias, d.gy = _t(w).to(dt), _t(bias), _t(g).to(dt)
    o = _outputs(d, kp, seed)
    _same("a second run", _outputs(d, kp, seed), o)
    a, b, gy = _view(d.a, None), (_view(d.b, None) if cb else None), _view(d.gy, None)
    # each input gradient alone, and the weight gradient without the bias gradient
    only_a, none = raw_dgrad(d, gy, None, kp, seed, _blank(rows, ca, dt, None), None)
    assert none is None and torch.equal(only_a, o["d_a"]), "d_a alone differs"
    if cb:
        none, only_b = raw_dgrad(d, gy, None, kp, seed, None, _blank(rows, cb, dt, None))
        assert none is None and torch.equal(only_b, o["d_b"]), "d_b alone differs"
    dw, none = raw_wgrad(d, a, b, gy, None, kp, seed, bias=False)
    assert none is None and torch.equal(dw, o["dw"]), "dw without the bias gradient differs"
    if strided:
        for off in (8, 3):
            _same(f"cut at channel {off}", _outputs(d, kp, seed, off=off), o)
    if kp == 1.0:
        _same("another seed at keep_prob 1", _outputs(d, kp, OTHER_SEED), o)
    torch.cuda.synchronize()
    x64 = x.astype(np.float64)
    _held(f"dense-{rows}x{ca}+{cb}-{co}", o, _own_ref(x64, np.abs(x64), w.astype(np.float64), bias.astype(np.float64),
                                                      g.astype(np.float64), ca, bf, kp, seed))
    return o


# name -> (function, arguments)
CASES = {}
for _dt in ("f32", "bf16"):
    for _kp in (None, 0.5):
        _k = "" if _kp is None else "-keep0.5"
        # the K loop's exits: 1, 2 and 3 steps of 32 (f32) / 64 (bf16) channels
        for _ca in ((5, 64, 96) if _dt == "f32" else (5, 128, 192)):
            CASES[f"ksteps-{_ca}+0-18{_k}-{_dt}"] = (case_dense, (40, _ca, 0, 18, _dt, _kp))
        # c_out padded to 4, 8, 20, 32 columns (32: two rows side by side in the dropout weight gradient)
        for _heads in ((1,), (6,), (4, 14), (32,)):
            CASES[f"grouped-16+24-{sum(_heads)}{_k}-{_dt}"] = (case_map, ("grouped", 16, 24, _heads, _dt, _kp))
        # a dense second source; strided and offset operands
        CASES[f"dense-16+24-18{_k}-{_dt}"] = (case_dense, (40, 16, 24, 18, _dt, _kp, SEED, True))
        CASES[f"dense-5+6-18{_k}-{_dt}"] = (case_dense, (40, 5, 6, 18, _dt, _kp))
        # channel tails in both sources; the mask group of 8 across the boundary, unpaired
        CASES[f"grouped-5+6-18{_k}-{_dt}"] = (case_map, ("grouped", 5, 6, (4, 14), _dt, _kp))
        # 266 rows over two frames: three GEMM workgroups, three input-gradient blocks; strided and offset
        CASES[f"frames266-64+128-18{_k}-{_dt}"] = (case_map, ("frames266", 64, 128, (4, 14), _dt, _kp, SEED, True))
        CASES[f"frames266-img27-64+128-18{_k}-{_dt}"] = (case_map, ("frames266-img27", 64, 128, (4, 14), _dt, _kp))
        # more than 64 * COLS channels: grid.y of 2 in the backward kernels
        CASES[f"wide-260+0-18{_k}-{_dt}"] = (case_dense, (40, 260, 0, 18, _dt, _kp))
        # the weight gradient's chunks: 65 rows each (plain) and two batch trips of a wave (dropout); 70 rows:
        # chunk 1 holds 6, so most of its waves hold none
        CASES[f"rows16448-8+4-4{_k}-{_dt}"] = (case_dense, (16448, 8, 4, 4, _dt, _kp))
        CASES[f"rows70-8+4-4{_k}-{_dt}"] = (case_dense, (70, 8, 4, 4, _dt, _kp))
        CASES[f"k768+768-18{_k}-{_dt}"] = (case_map, ("k768", 768, 768, (4, 14), _dt, _kp))  # the real K loop
    CASES[f"frames266-64+128-18-keep0.8-{_dt}"] = (case_map, ("frames266", 64, 128, (4, 14), _dt, 0.8))
    CASES[f"frames266-64+128-18-keep1.0-{_dt}"] = (case_map, ("frames266", 64, 128, (4, 14), _dt, 1.0))
    CASES[f"frames266-64+128-18-keep0.5-seed2-{_dt}"] = (case_map, ("frames266", 64, 128, (4, 14), _dt, 0.5, OTHER_SEED))


def digest(t):
    """SHA-256 of a tensor's bytes."""
    t = t.detach().contiguous()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def run_case(name):
    """{output name: digest} of a case, after its oracle and identity assertions."""
    fn, args = CASES[name]
    outs = fn(*args)
    torch.cuda.synchronize()
    return {k: digest(v) for k, v in outs.items()}


@functools.lru_cache(maxsize=None)
def _table():
    with open(TABLE) as fh:
        return json.load(fh)


def test_table_lists_every_case():
    """Every case has a recorded hash of every output: none is left without."""
    assert sorted(_table()) == sorted(CASES)
    for name, row in _table().items():
        assert set(row) in ({"out", "d_a", "d_b", "dw", "dbias"}, {"out", "d_a", "dw", "dbias"}), name
        assert all(len(v) == 64 for v in row.values())


@pytest.mark.parametrize("name", list(CASES))
def test_head_case(name):
    assert run_case(name) == _table()[name]
