"""shpl_upconv3x3_dgrad / shpl_upconv3x3_wgrad and FusionUpconv(backward="direct") -- the upconv3's own gradient
kernels -- against the float64 adjoints of tests/test_gpu_upconv.py (its cases, oracle maps and bounds, imported,
not copied) on MI355X.

Tolerances (derived, not tuned): any summation order of n f32 terms satisfies |err| <= 1.01 (n + 2) 2^-24 S, S the
same expression over absolute values (base._bound). Input gradient: an element sums at most 9 c_out products, and
a bf16 store adds |ref| 2^-8. Weight gradient: n = F h w (one product per input pixel and tap), f32 output. The
training step takes base._train_reference's bounds unchanged (its input gradient's term count, 36 c_out, covers
the direct route's 9 c_out).

One shape of this file's own, 8 x 32 input pixels in one frame: exactly one tile of the input gradient, so the gy
halo row 2*8 and column 2*32 lie outside the map (and, one frame, outside the buffer) and must read as zeros.
"""
import functools

import numpy as np
import pytest
import torch

import test_gpu_upconv as base

pytestmark = pytest.mark.gpu

DEV = base.DEV
TILE = "tile-8x32-32+16-32"
TILE_BEV, TILE_IMG = (8, 32), (3, 10)

# the tile case rides base._case: registered beside base's cases (base.PARAMS, computed at its import, is unchanged)
base.CASES.setdefault(TILE, ("tile", 32, 16, 32, ("bev",)))
_base_map = base._map


@functools.lru_cache(maxsize=None)
def _map(kind):
    if kind != "tile":
        return _base_map(kind)
    smap, refs = base._frames_map((50,), TILE_BEV, TILE_IMG, seed=900)
    return smap, refs, TILE_BEV, TILE_IMG


base._map = _map

PARAMS = list(base.PARAMS) + [(TILE, "bev", d) for d in ("f32", "bf16")]
IDS = [f"{c}-{s}-{d}" for c, s, d in PARAMS]
RAGGED = [p for p in base.PARAMS if p[0].startswith("ragged")]
RAGGED_IDS = [f"{c}-{s}-{d}" for c, s, d in RAGGED]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from sparse_pooling_amd import _lib as L
    L.lib()
    assert torch.cuda.is_available()


def _pool(c):
    return (c.smap.csr(*base._side(c).fwd), c.smap.frame_off) if c.pooled else (None, None)


def _wide(g, extra=8):
    """g as a view into a buffer whose rows are `extra` channels wider."""
    buf = torch.full(tuple(g.shape[:3]) + (g.shape[3] + extra,), 7.0, dtype=g.dtype, device=g.device)
    buf[..., :g.shape[3]] = g
    view = buf[..., :g.shape[3]]
    assert view.stride(2) == g.shape[3] + extra
    return view


@pytest.mark.parametrize("name,side,dtype", PARAMS, ids=IDS)
def test_dgrad(name, side, dtype):
    """upconv3x3_dgrad against upconv_dx in float64; the split call's two maps are the unsplit call's channels,
    bitwise; gy through a wider row stride gives the same bits."""
    from sparse_pooling_amd import fusion_upconv as fu
    c = base._case(name, side, dtype)
    g, tw = base._t(c.g).to(c.dt), base._t(c.w).to(c.dt)
    cin = c.ca + c.cb
    whole = fu.upconv3x3_dgrad(g, tw, cin)
    strided = fu.upconv3x3_dgrad(_wide(g), tw, cin)
    parts = fu.upconv3x3_dgrad(g, tw, cin, split=c.ca) if c.cb else None
    torch.cuda.synchronize()
    assert tuple(whole.shape) == (c.F,) + tuple(c.a_hw) + (cin,) and whole.dtype == c.dt
    g64 = c.g.astype(np.float64)
    ref = base.upconv_dx(g64, c.W)
    bound = base._bound(base.upconv_dx(np.abs(g64), np.abs(c.W)), 9 * c.co) + c.store(ref)
    base._within("dx", base._np(whole), ref, bound)
    assert torch.equal(strided, whole), "gy_stride > c_gy changes the result"
    if parts is not None:
        assert tuple(parts[0].shape)[-1] == c.ca and tuple(parts[1].shape)[-1] == c.cb
        assert torch.equal(torch.cat(parts, -1), whole), "the split call differs from the unsplit one"


@pytest.mark.parametrize("name,side,dtype", PARAMS, ids=IDS)
def test_wgrad(name, side, dtype):
    """upconv3x3_wgrad (pooled in the staging) against upconv_dw over the oracle's fused map; bitwise the call on the
    dense pulled map and on the materialised concat where c_a is a whole number of staging chunks."""
    from sparse_pooling_amd import fusion_upconv as fu
    c = base._case(name, side, dtype)
    ta, tb, _ = base._dev(c)
    g = base._t(c.g).to(c.dt)
    pool, fo = _pool(c)
    dw = fu.upconv3x3_wgrad(ta, g, b=tb, pool=pool, frame_off=fo)
    dense = cat = None
    if c.pooled:
        mat = base._side(c).pool(c.smap, tb, ta.shape[:3] + (c.cb,))
        dense = fu.upconv3x3_wgrad(ta, g, b=mat)
        cat = fu.upconv3x3_wgrad(torch.cat([ta, mat], -1), g)
    torch.cuda.synchronize()
    assert c.smap.error_bits() == 0
    assert tuple(dw.shape) == (3, 3, c.co, c.ca + c.cb) and dw.dtype == torch.float32
    g64 = c.g.astype(np.float64)
    ref = base.upconv_dw(c.x, g64)
    F, h, w = c.x.shape[:3]
    bound = base._bound(base.upconv_dw(np.abs(c.x), np.abs(g64)), F * h * w)
    base._within("dW", base._np(dw), ref, bound)
    if c.pooled:
        base._within("dW dense pulled map", base._np(dense), ref, bound)
        base._within("dW materialised", base._np(cat), ref, bound)
        if c.ca % (16 if c.bf else 8) == 0:
            assert torch.equal(dense, dw), "the pooled call differs from the call on the dense pulled map"
            assert torch.equal(cat, dw), "the pooled call differs from the call on the materialised concat"


@pytest.mark.parametrize("name,side,dtype", RAGGED, ids=RAGGED_IDS)
def test_repeatable(name, side, dtype):
    from sparse_pooling_amd import fusion_upconv as fu
    c = base._case(name, side, dtype)
    ta, tb, tw = base._dev(c)
    g = base._t(c.g).to(c.dt)
    pool, fo = _pool(c)
    dx = [fu.upconv3x3_dgrad(g, tw, c.ca + c.cb, split=c.ca) for _ in range(2)]
    dw = [fu.upconv3x3_wgrad(ta, g, b=tb, pool=pool, frame_off=fo) for _ in range(2)]
    torch.cuda.synchronize()
    assert torch.equal(dx[0][0], dx[1][0]) and torch.equal(dx[0][1], dx[1][1])
    assert torch.equal(dw[0], dw[1])


def _train(c, r, beta, mm0, mv0, backward):
    """base.test_training_step's checks for one module."""
    up = base._module(c, decay=0.5, backward=backward)
    assert up.backward == backward
    up.beta.copy_(base._t(beta))
    up.moving_mean.copy_(base._t(mm0))
    up.moving_var.copy_(base._t(mv0))
    ta, tb, _ = base._dev(c)
    leaves = [ta.requires_grad_(True), tb.requires_grad_(True), up.weights.requires_grad_(True),
              up.beta.requires_grad_(True)]
    y = base._fused(up, c, ta, tb, is_training=True)
    y.backward(base._t(c.g).to(c.dt))
    torch.cuda.synchronize()
    assert c.smap.error_bits() == 0
    da, db, dW, dbeta = (t.grad for t in leaves)
    assert da.dtype == c.dt and db.dtype == c.dt and dW.dtype == c.dt and dbeta.dtype == torch.float32
    assert tuple(dW.shape) == (3, 3, c.co, c.ca + c.cb) and tuple(db.shape) == tuple(tb.shape)
    what = lambda s: f"{backward} {s}"  # noqa: E731
    base._within(what("y"), base._np(y), r.y, r.y_bound)
    base._within(what("moving_mean"), base._np(up.moving_mean), r.mm, r.mm_bound)
    base._within(what("moving_var"), base._np(up.moving_var), r.mv, r.mv_bound)
    np.testing.assert_allclose(base._np(up._scale), 1.0 / np.sqrt(base._np(up.moving_var) + base.EPS),
                               rtol=4 * base.U)
    base._within(what("d_a"), base._np(da), r.da, r.da_bound)
    base._within(what("d_b"), base._np(db), r.db, r.db_bound)
    base._within(what("dW"), base._np(dW), r.dW, r.dW_bound)
    base._within(what("dbeta"), base._np(dbeta), r.dbeta, r.dbeta_bound)


@pytest.mark.parametrize("name,side,dtype", base.TRAIN, ids=base.TRAIN_IDS)
def test_training_step_direct(name, side, dtype):
    """FusionUpconv(backward="direct").fused / fused_img with is_training: every quantity of
    base.test_training_step within base._train_reference's bounds; backward="phases" within the same bounds."""
    from sparse_pooling_amd import fusion_upconv as fu
    c = base._case(name, side, dtype)
    rng = np.random.default_rng(5)
    beta = rng.standard_normal(c.co).astype(np.float32) * 0.5
    mm0 = rng.standard_normal(c.co).astype(np.float32)
    mv0 = rng.uniform(0.5, 2.0, c.co).astype(np.float32)
    r = base._train_reference(c, beta, mm0.astype(np.float64), mv0.astype(np.float64), decay=0.5)
    _train(c, r, beta, mm0, mv0, "direct")
    _train(c, r, beta, mm0, mv0, "phases")
    with pytest.raises(ValueError):
        fu.FusionUpconv(c.ca + c.cb, c.co, dtype=c.dt, device=DEV, backward="x")


def test_gradients_are_capturable():
    """upconv3x3_dgrad and the pooled upconv3x3_wgrad recorded with torch.cuda.graph on one side stream, one after
    the other, and replayed twice give the eager bits: no allocation by the library, no host synchronisation."""
    from sparse_pooling_amd import _lib as L, fusion_upconv as fu
    c = base._case("ragged-2frames-32+16-64", "bev", "bf16")
    ta, tb, tw = base._dev(c)
    g = base._t(c.g).to(c.dt)
    pool, fo = _pool(c)  # the CSR, built outside the capture
    B, H, W = (int(s) for s in ta.shape[:3])
    dt = L.dtype_code(ta)
    ws_d = L.workspace(fu.upconv_grad_ws_bytes("dgrad", dt, B, H, W, c.co, 0, c.ca + c.cb), ta.device)
    ws_w = L.workspace(fu.upconv_grad_ws_bytes("wgrad", dt, B, H, W, c.ca, c.cb, c.co, pool.nnz_cap), ta.device)
    e_da, e_db = fu.upconv3x3_dgrad(g, tw, c.ca + c.cb, split=c.ca, ws=ws_d)
    e_dw = fu.upconv3x3_wgrad(ta, g, b=tb, pool=pool, frame_off=fo, ws=ws_w)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            da, db = fu.upconv3x3_dgrad(g, tw, c.ca + c.cb, split=c.ca, ws=ws_d)
            dw = fu.upconv3x3_wgrad(ta, g, b=tb, pool=pool, frame_off=fo, ws=ws_w)
    torch.cuda.synchronize()
    for _ in range(2):
        for t in (da, db, dw):
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(da, e_da) and torch.equal(db, e_db) and torch.equal(dw, e_dw)
