"""The fused SHPL concat with BatchNorm on both halves (shpl_concat_bn / shpl_concat_bn_backward and
fusion_bn.FusionConcatBN) against the CPU oracle in double, on MI355X.

Reference. oracle.sparse_pool_op / sparse_pool_trans_op give the dense pooled map; their f32 run sums are the
device's bit for bit (bf16: the oracle is fed the bf16-rounded inputs and its f32 sums are kept unrounded, as
the device keeps them). x = [pass || pooled] in double then goes through oracle.batch_norm_train(relu=False)
and oracle.batch_norm_backward(relu=False) -- every channel has its own BatchNorm, so one call over the
concatenated channels is the per-half computation -- and the source gradient is
oracle.sparse_pool_grad_img / sparse_pool_trans_grad_bev of the oracle's g_pool.

Bounds. Forward, per element (tests/test_gpu_batch_norm.py): 2^-20 * ((|x| + |mean|) * k + |beta|) with k =
|gamma| / sqrt(var + eps), x the pass-through value or the run sum (0 at empty rows); bf16 storage adds
2^-8 * |y_ref|. Moments: rtol 1e-6, atol 1e-7. Backward (that file's): g_x 1e-5 + 1e-5 * |scale| * (|g| + 1)
(+ 2^-8 * |ref| in bf16), dbeta 1e-4 + 1e-6 * sum |g|, dgamma 1e-4 + 1e-6 * sum |g * xhat|.
Source gradient: element (s, c) is sum_e m_e * g_pool[d_e, c] over the entries e whose source row is s, k of
them. The device's g_pool[d_e] is within b_x[d_e] (the g_x bound at that row) of the oracle's, so the exact
sums differ by at most sum_e |m_e| * b_x[d_e]; the device adds its k products one after the other in f32,
each product and each of the k partial sums rounded once, at most 2^-24 * (k + 1) * sum_e |m_e * g_pool| <=
2^-23 * k * sum_e |m_e * g_pool|. Hence
    b_src[s] = sum_e |m_e| * b_x[d_e] + 2^-23 * k * sum_e |m_e * g_pool[d_e]|.
A bf16 rounding is up to 2^-8 relative (half an ulp of 2^-7 at the bottom of a binade), so b_x's 2^-8 * |ref|
pays for exactly one; the source gradient therefore stays f32 through the C ABI in both dtypes -- g_pool is
written unrounded into an f32 scratch and pulled in f32 -- and is rounded once where a bf16 tensor is wanted
(a bf16 scratch pulled into a bf16 map rounds twice and measured 1.27 times this bound).
Nothing is left out of any comparison.

Largest observed error / bound per output (MI355X, this file's cases): docs/HISTORY.md.
"""
import functools
import json
import types

import numpy as np
import pytest
import torch

from oracle import shpl_oracle as orc

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS, DECAY = 1e-3, 0.999
F32, BF16 = "f32", "bf16"
TORCH = {F32: torch.float32, BF16: torch.bfloat16}
SMALL = dict(bev_hw=(6, 7), img_hw=(10, 40), frames=1)
LARGE = dict(bev_hw=(70, 64), img_hw=(24, 80), frames=2)  # 8960 rows: three blocks of partial sums, ragged tail
# 66560 cells in one frame: past the range builder's 65536 destinations per frame, where the key ranges come from
# the frame builder (the form config 2's 563200 cells per frame take)
WIDE = dict(bev_hw=(260, 256), img_hw=(24, 80), frames=1)
LONG = 40  # a run past SHPL_CSR_MAX_HEAD = 32
RATIOS = {}


def _bf(a):
    return orc.from_bf16_bits(orc.to_bf16_bits(a))


def _frozen(**kw):
    for v in kw.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return types.SimpleNamespace(**kw)


# ---------------------------------------------------------------- maps
@functools.lru_cache(maxsize=None)
def make_map(kind, shape):
    """A seeded hand-made M in the reference format over `frames` frames (frame f's cells meet frame f's
    pixels only). kind "sparse": about a tenth of the cells occupied, runs of 1, 2 and 40 entries, values of
    both signs; the pixels are drawn from a pool a third of the entries' size, so pixels are fed by several
    columns, and a fifth of the entries share a column with another cell's entry (per-column partials on
    the pixel side); with two frames the second has no entry at all. "once": every cell occupied exactly
    once. "empty": no entries."""
    sh = {"small": SMALL, "large": LARGE, "wide": WIDE}[shape]
    (hb, wb), (hi, wi), F = sh["bev_hw"], sh["img_hw"], sh["frames"]
    nc, npx = hb * wb, hi * wi
    rng = np.random.default_rng([7, len(kind), nc])
    rows, pix = [], []
    if kind == "sparse":
        occ = rng.choice(nc, max(nc // 10, 4), replace=False)  # frame 0 only: a later frame stays empty
        runs = np.array([1, 2, LONG, 1] + list(rng.choice([1, 2, 3, LONG], len(occ) - 4, p=[0.5, 0.3, 0.15, 0.05])))
        for cell, n in zip(occ, runs):
            rows += [int(cell)] * int(n)
        pool = rng.choice(npx, min(max(len(rows) // 3, 2), npx), replace=False)
        pix = [int(p) for p in rng.choice(pool, len(rows))]
    elif kind == "once":
        for f in range(F):
            rows += [f * nc + r for r in range(nc)]
            pix += [f * npx + int(p) for p in rng.choice(npx, nc)]
    nnz = len(rows)
    # columns: four fifths of the entries get one of their own, the rest join another entry's (and its pixel)
    n_cols = nnz if kind != "sparse" else max(nnz * 4 // 5, 1)
    cols = list(range(n_cols)) + [int(k) for k in rng.integers(0, max(n_cols, 1), nnz - n_cols)]
    col_pix = np.asarray(pix[:n_cols], np.int64)
    order = rng.permutation(nnz)
    mij = np.stack([np.asarray(rows, np.int64), np.asarray(cols, np.int64)], 1).reshape(-1, 2)[order]
    mval = rng.uniform(0.25, 2.0, nnz) * np.where(rng.random(nnz) < 0.5, -1.0, 1.0)
    idx = np.stack([col_pix // npx, col_pix % npx // wi, col_pix % wi], 1).reshape(-1, 3)
    ent_pix = col_pix[mij[:, 1]] if nnz else np.zeros(0, np.int64)
    cell_run = np.bincount(mij[:, 0], minlength=F * nc)
    pix_run = np.bincount(ent_pix, minlength=F * npx)
    if kind == "sparse":
        assert {1, 2, LONG} <= set(cell_run.tolist()) and (mval > 0).any() and (mval < 0).any()
        assert 0.05 < (cell_run[:nc] > 0).mean() < 0.2 and pix_run.max() > 2
        assert np.bincount(mij[:, 1]).max() > 1  # a column with several entries
        # pixels fed by several columns
        assert max(len(set(mij[ent_pix == p, 1])) for p in np.flatnonzero(pix_run > 1)) > 1
        assert F == 1 or (cell_run[nc:].sum() == 0 and pix_run[npx:].sum() == 0)
    if kind == "once":
        assert (cell_run == 1).all()
    return _frozen(mij=np.ascontiguousarray(mij), mval=mval.astype(np.float32), idx=np.ascontiguousarray(idx),
                   m_size=np.array([F * nc, n_cols], np.int64), bev_shape=(F, hb, wb), img_shape=(F, hi, wi),
                   ent_cell=mij[:, 0].copy(), ent_pix=ent_pix, cell_run=cell_run, pix_run=pix_run)


MAPS = [("sparse", "small"), ("once", "small"), ("empty", "small"), ("sparse", "large")]
MAP_IDS = ["b-sparse-6x7", "c-once-6x7", "d-empty-6x7", "a-two-frames-70x64"]
CHANNELS = [(F32, 32, 32, True), (F32, 16, 32, True), (F32, 7, 7, False), (BF16, 32, 32, True),
            (BF16, 12, 12, False)]  # dtype, c_bev, c_img, vector form
CH_IDS = [f"{dt}-{cb}+{ci}-{'vec' if v else 'scalar'}" for dt, cb, ci, v in CHANNELS]


@functools.lru_cache(maxsize=None)
def _smap(kind, shape):
    from sparse_pooling_amd import shpl_map as sm
    m = make_map(kind, shape)
    t = lambda a: torch.from_numpy(np.array(a)).to(DEV)  # noqa: E731
    return sm.pack_map(t(m.mij), t(m.mval), m.m_size, t(m.idx), m.img_shape)


@functools.lru_cache(maxsize=None)
def _case(kind, shape, dt, c_bev, c_img, side):
    """Inputs and the dense oracle map x = [pass || pooled] of one side (host, read-only)."""
    m = make_map(kind, shape)
    rng = np.random.default_rng([11, c_bev, c_img, len(kind), len(shape), side == "bv"])
    F, hb, wb = m.bev_shape
    _, hi, wi = m.img_shape
    bev = (rng.standard_normal((F, hb, wb, c_bev)) * rng.uniform(0.5, 3.0, c_bev) + rng.standard_normal(c_bev))
    img = (rng.standard_normal((F, hi, wi, c_img)) * rng.uniform(0.5, 3.0, c_img) + rng.standard_normal(c_img))
    bev, img = bev.astype(np.float32), img.astype(np.float32)
    if dt == BF16:
        bev, img = _bf(bev), _bf(img)
    if side == "bv":
        pass_, src = bev, img
        pooled = orc.sparse_pool_op(m.mij, m.mval, m.m_size, img, m.idx)
        occ = m.cell_run > 0
    else:
        pass_, src = img, bev
        pooled = orc.sparse_pool_trans_op(m.mij, m.mval, m.m_size, bev.reshape(-1, c_bev), m.idx, img.shape)
        occ = m.pix_run > 0
    c_pass, c_pool = pass_.shape[-1], src.shape[-1]
    c = c_pass + c_pool
    x32 = np.concatenate([pass_.reshape(-1, c_pass), pooled.reshape(-1, c_pool)], 1)
    assert not x32[~occ, c_pass:].any()
    x64 = x32.astype(np.float64)
    rows = x64.shape[0]
    g = rng.standard_normal((rows, c)).astype(np.float32)
    if dt == BF16:
        g = _bf(g)
    gamma = (rng.uniform(0.25, 2.0, c) * np.where(rng.random(c) < 0.5, -1.0, 1.0)).astype(np.float32)
    beta = rng.standard_normal(c).astype(np.float32)
    beta[np.abs(beta) < 0.01] = 0.01
    mm0 = (x64.mean(0) + 0.3 * rng.standard_normal(c)).astype(np.float32)
    mv0 = (x64.var(0) * rng.uniform(0.5, 2.0, c) + 0.1).astype(np.float32)
    return _frozen(m=m, pass_=pass_, src=src, x64=x64, occ=occ, rows=rows, c_pass=c_pass, c_pool=c_pool, c=c, g=g,
                   gamma=gamma, beta=beta, mm0=mm0, mv0=mv0)


def _t(a, dt=None):
    if a is None:
        return None
    t = torch.from_numpy(np.array(a)).to(DEV)
    return t if dt is None else t.to(TORCH[dt])


def _np(t):
    return t.detach().float().cpu().numpy() if t.dtype == torch.bfloat16 else t.detach().cpu().numpy()


def _misaligned(t):
    buf = torch.empty(t.numel() + 16, dtype=t.dtype, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


def _within(got, ref, bound, what, name):
    err = np.abs(np.asarray(got, np.float64) - ref)
    ratio = float((err / bound).max()) if err.size else 0.0
    print("ratio", name, what, ratio)
    RATIOS[name] = max(RATIOS.get(name, 0.0), ratio)
    bad = ~(err <= bound)
    assert not bad.any(), (what, name, float(err.max()), ratio, int(bad.sum()))


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from sparse_pooling_amd import _lib as L
    L.lib()
    assert torch.cuda.is_available()
    yield
    print("concat_bn max error/bound ratios:", json.dumps(RATIOS, sort_keys=True))


# ---------------------------------------------------------------- references
def _moments(d, training):
    """(mean, biased var) the normalisation uses, in double."""
    if training:
        return d.x64.mean(0), d.x64.var(0)
    return d.mm0.astype(np.float64), d.mv0.astype(np.float64)


def _ref_fwd(d, training, use_gamma):
    gamma = d.gamma if use_gamma else None
    if training:
        y, bm, bv, mm, mv = orc.batch_norm_train(d.x64, EPS, gamma, d.beta, False, d.mm0, d.mv0, DECAY)
        return _frozen(y=y, bm=bm, bv=bv, mm=mm, mv=mv)
    mean, var = _moments(d, False)
    gm = 1.0 if gamma is None else gamma.astype(np.float64)
    y = ((d.x64 - mean) * (gm / np.sqrt(var + EPS)) + d.beta.astype(np.float64)).astype(np.float32)
    return _frozen(y=y, bm=None, bv=None, mm=d.mm0, mv=d.mv0)


def _fwd_bound(dt, d, training, use_gamma, y_ref):
    mean, var = _moments(d, training)
    k = (np.abs(d.gamma.astype(np.float64)) if use_gamma else 1.0) / np.sqrt(var + EPS)
    b = 2.0 ** -20 * ((np.abs(d.x64) + np.abs(mean)) * k + np.abs(d.beta))
    return b + 2.0 ** -8 * np.abs(y_ref) if dt == BF16 else b


def _run_fwd(kind, shape, dt, d, side, training, use_gamma, misalign=False):
    from sparse_pooling_amd import fusion_bn as fb
    al = _misaligned if misalign else (lambda t: t)
    mm, mv = _t(d.mm0), _t(d.mv0)
    bm, bv = (torch.zeros(d.c, dtype=torch.float32, device=DEV) for _ in range(2))
    out, save = fb.concat_bn_forward(_smap(kind, shape), side, al(_t(d.pass_, dt)), al(_t(d.src, dt)),
                                     _t(d.gamma) if use_gamma else None, _t(d.beta), mm, mv, eps=EPS, decay=DECAY,
                                     training=training, batch_mean=bm, batch_var=bv)
    return out.reshape(-1, d.c), save, mm, mv, bm, bv


def _check_fwd(dt, d, training, use_gamma, got, what):
    y, save, mm, mv, bm, bv = got
    ref = _ref_fwd(d, training, use_gamma)
    _within(_np(y), ref.y, _fwd_bound(dt, d, training, use_gamma, ref.y), what, "y")
    tol = dict(rtol=1e-6, atol=1e-7, err_msg=str(what))
    np.testing.assert_allclose(_np(mm), ref.mm, **tol)
    np.testing.assert_allclose(_np(mv), ref.mv, **tol)
    if training:
        np.testing.assert_allclose(_np(bm), ref.bm, **tol)
        np.testing.assert_allclose(_np(bv), ref.bv, **tol)
    # the saved mean the backward takes is the batch (moving) mean
    mean, _ = _moments(d, training)
    np.testing.assert_allclose(_np(save[0]), mean, **tol)
    # empty rows: one bit pattern per channel across the whole map
    if (~d.occ).any():
        e = y[torch.from_numpy(~d.occ).to(DEV)][:, d.c_pass:]
        bits = e.view(torch.int32 if dt == F32 else torch.int16)
        assert bool((bits == bits[:1]).all()), what


@pytest.mark.parametrize("kind,shape", MAPS, ids=MAP_IDS)
@pytest.mark.parametrize("dt,c_bev,c_img,vec", CHANNELS, ids=CH_IDS)
def test_forward_vs_oracle(dt, c_bev, c_img, vec, kind, shape):
    """Both directions, training and inference, gamma NULL in training and set in inference: every output
    element, the batch and moving moments, the saved mean; the empty rows' pooled half is one bit pattern per
    channel. On the map without entries the pooled half is exactly beta and its batch mean and variance are
    exactly 0."""
    for side in ("bv", "img"):
        d = _case(kind, shape, dt, c_bev, c_img, side)
        for training in (True, False):
            use_gamma = not training
            got = _run_fwd(kind, shape, dt, d, side, training, use_gamma)
            _check_fwd(dt, d, training, use_gamma, got, (kind, shape, side, training))
            if kind == "empty" and training:
                y, _, _, _, bm, bv = got
                want = _t(d.beta[d.c_pass:]).to(TORCH[dt])
                assert torch.equal(y[:, d.c_pass:], want.expand(d.rows, -1)), side
                assert not bm[d.c_pass:].any() and not bv[d.c_pass:].any(), side


def test_forward_misaligned_inputs():
    """f32 32 + 32 with both inputs one element off 16-byte alignment: the scalar form. Training matches the
    oracle; inference does the same rounded operations per element as the vector form: bit-identical."""
    kind, shape, dt = "sparse", "small", F32
    for side in ("bv", "img"):
        d = _case(kind, shape, dt, 32, 32, side)
        for training in (True, False):
            got = _run_fwd(kind, shape, dt, d, side, training, True, misalign=True)
            _check_fwd(dt, d, training, True, got, (side, training, "misaligned"))
            if not training:
                assert torch.equal(got[0], _run_fwd(kind, shape, dt, d, side, False, True)[0])


# ---------------------------------------------------------------- backward
def _ref_bwd(d, side, training, use_gamma):
    m = d.m
    gamma = d.gamma if use_gamma else None
    mean, var = _moments(d, training)
    e_raw, e_db, e_dg = orc.batch_norm_backward(d.x64, d.g, training, mean, var, EPS, gamma, None, False)
    gm = 1.0 if gamma is None else gamma.astype(np.float64)
    scale = gm / np.sqrt(var + EPS) * np.ones(d.c)
    xhat = (d.x64 - mean) / np.sqrt(var + EPS)
    g_pool = e_raw[:, d.c_pass:].astype(np.float32)
    if side == "bv":
        e_src = orc.sparse_pool_grad_img(m.mij, m.mval, m.m_size, g_pool, m.idx, m.img_shape)
        dst, src_row, n_src = m.ent_cell, m.ent_pix, int(np.prod(m.img_shape))
    else:
        e_src = orc.sparse_pool_trans_grad_bev(m.mij, m.mval, m.m_size, g_pool.reshape(m.img_shape + (-1,)), m.idx)
        dst, src_row, n_src = m.ent_pix, m.ent_cell, int(np.prod(m.bev_shape))
    return _frozen(e_raw=e_raw, e_db=e_db, e_dg=e_dg, e_src=e_src.reshape(n_src, -1).astype(np.float64), scale=scale,
                   xhat=xhat, dst=dst, src_row=src_row, n_src=n_src)


def _run_bwd(kind, shape, dt, d, side, training, use_gamma, save):
    from sparse_pooling_amd import fusion_bn as fb
    return fb.concat_bn_backward(_smap(kind, shape), side, _t(d.pass_, dt), _t(d.src, dt), _t(d.g, dt), save,
                                 gamma=_t(d.gamma) if use_gamma else None, training=training)


def _check_bwd(dt, d, side, training, use_gamma, got, what):
    g_pass, g_src, dbeta, dgamma = got
    r = _ref_bwd(d, side, training, use_gamma)
    g64 = d.g.astype(np.float64)
    b_x = 1e-5 + 1e-5 * np.abs(r.scale) * (np.abs(g64) + 1.0)
    if dt == BF16:
        b_x = b_x + 2.0 ** -8 * np.abs(r.e_raw)
    _within(_np(g_pass).reshape(d.rows, -1), r.e_raw[:, :d.c_pass], b_x[:, :d.c_pass], what, "g_pass")
    _within(_np(dbeta), r.e_db, 1e-4 + 1e-6 * np.abs(g64).sum(0), what, "dbeta")
    _within(_np(dgamma), r.e_dg, 1e-4 + 1e-6 * np.abs(g64 * r.xhat).sum(0), what, "dgamma")
    # the source gradient (module docstring)
    mabs = np.abs(d.m.mval.astype(np.float64))[:, None]
    b_src = np.zeros((r.n_src, d.c_pool))
    np.add.at(b_src, r.src_row, mabs * b_x[r.dst][:, d.c_pass:])
    k = np.bincount(r.src_row, minlength=r.n_src).astype(np.float64)[:, None]
    mg = np.zeros((r.n_src, d.c_pool))
    np.add.at(mg, r.src_row, mabs * np.abs(r.e_raw[r.dst][:, d.c_pass:]))
    b_src = b_src + 2.0 ** -23 * k * mg
    got_src = _np(g_src).reshape(r.n_src, -1)
    assert not got_src[k[:, 0] == 0].any(), what  # a source row no entry names gets exactly 0
    _within(got_src, r.e_src, np.maximum(b_src, 1e-300), what, "g_src")


@pytest.mark.parametrize("kind,shape", MAPS, ids=MAP_IDS)
@pytest.mark.parametrize("dt,c_bev,c_img,vec", CHANNELS, ids=CH_IDS)
def test_backward_vs_oracle(dt, c_bev, c_img, vec, kind, shape):
    """Both directions, training (gamma set) and inference (gamma NULL), after the device's own forward (its
    saved mean and scale): g_pass, dbeta, dgamma and the source gradient."""
    for side in ("bv", "img"):
        d = _case(kind, shape, dt, c_bev, c_img, side)
        for training in (True, False):
            use_gamma = training
            save = _run_fwd(kind, shape, dt, d, side, training, use_gamma)[1]
            got = _run_bwd(kind, shape, dt, d, side, training, use_gamma, save)
            _check_bwd(dt, d, side, training, use_gamma, got, (kind, shape, side, training))


def test_more_than_65536_keys_per_frame():
    """BEV 260 x 256 in one frame: ShplMap.csr(key_range=True) leaves the range builder for the frame builder
    followed by k_key_range (the branch config 2's maps take). Forward and backward, training, against the
    oracle with the same bounds; 17 blocks of partial sums."""
    from sparse_pooling_amd import _lib as L
    kind, shape, dt, side = "sparse", "wide", F32, "bv"
    smap = _smap(kind, shape)
    assert smap.n_cells // smap.n_frames > L.ROWS_MAX_KEYS
    d = _case(kind, shape, dt, 16, 32, side)
    got = _run_fwd(kind, shape, dt, d, side, True, True)
    assert smap.csr(L.BY_CELL, L.ORDER_ENTRY, key_range=True).key_range is not None
    _check_fwd(dt, d, True, True, got, (shape, side))
    _check_bwd(dt, d, side, True, True, _run_bwd(kind, shape, dt, d, side, True, True, got[1]), (shape, side))


def test_backward_misaligned_streams():
    """f32 32 + 32 (the vector form by its channel counts) with g alone, and with every map, one element off
    16-byte alignment: cbn_chunks drops to the scalar form. Training matches the oracle; inference's g_pass =
    scale * g is the vector form's bit for bit."""
    from sparse_pooling_amd import fusion_bn as fb
    kind, shape, dt = "sparse", "small", F32
    smap = _smap(kind, shape)
    for side in ("bv", "img"):
        d = _case(kind, shape, dt, 32, 32, side)
        for training in (True, False):
            save = _run_fwd(kind, shape, dt, d, side, training, True)[1]
            ref = _run_bwd(kind, shape, dt, d, side, training, True, save)
            for all_maps in (False, True):
                al = _misaligned if all_maps else (lambda t: t)
                got = fb.concat_bn_backward(smap, side, al(_t(d.pass_, dt)), al(_t(d.src, dt)),
                                            _misaligned(_t(d.g, dt)), save, gamma=_t(d.gamma), training=training,
                                            scratch=_misaligned(torch.empty(d.rows * d.c_pool, device=DEV)))
                _check_bwd(dt, d, side, training, True, got, (side, training, all_maps, "misaligned"))
                if not training:
                    assert torch.equal(got[0], ref[0])


@pytest.mark.parametrize("dt,c_bev,c_img", [(F32, 32, 32), (BF16, 12, 12)], ids=["f32-vec", "bf16-scalar"])
def test_two_runs_are_bit_identical(dt, c_bev, c_img):
    """No floating-point atomics anywhere: two calls on the same inputs give the same bits, forward (output,
    moments, saved mean and scale) and backward (all four outputs), over 8960 rows (three partial blocks)."""
    kind, shape = "sparse", "large"
    for side in ("bv", "img"):
        d = _case(kind, shape, dt, c_bev, c_img, side)
        a, b = (_run_fwd(kind, shape, dt, d, side, True, True) for _ in range(2))
        for u, v in zip(a, b):
            assert torch.equal(u, v), side
        ga, gb = (_run_bwd(kind, shape, dt, d, side, True, True, a[1]) for _ in range(2))
        for u, v in zip(ga, gb):
            assert torch.equal(u, v), side


# ---------------------------------------------------------------- module
def test_autograd_dual_equals_c_level_bitwise():
    """FusionConcatBN.__call__(dual=True) on the sparse map: gradients reach bev, img and all four betas (the
    two halves of beta_bv and of beta_img) and equal the C-level results bit for bit; bev's and img's are the
    sum of a pass-through gradient and a source gradient, a two-operand f32 add (commutative)."""
    from sparse_pooling_amd import fusion_bn as fb
    import sparse_pooling_amd
    assert sparse_pooling_amd.FusionConcatBN is fb.FusionConcatBN
    kind, shape, dt, cb, ci = "sparse", "small", F32, 32, 32
    smap = _smap(kind, shape)
    dbv, dim = _case(kind, shape, dt, cb, ci, "bv"), _case(kind, shape, dt, cb, ci, "img")
    mod = fb.FusionConcatBN(cb, ci, eps=EPS, decay=DECAY, dtype=torch.float32, device=DEV)
    with torch.no_grad():
        mod.beta_bv.copy_(_t(dbv.beta))
        mod.beta_img.copy_(_t(dim.beta))
    bev = _t(dbv.pass_).requires_grad_(True)
    img = _t(dbv.src).requires_grad_(True)
    bv_f, img_f = mod(bev, img, smap, dual=True, is_training=True)
    g_bv, g_img = _t(dbv.g).view_as(bv_f), _t(dim.g).view_as(img_f)
    ((bv_f * g_bv).sum() + (img_f * g_img).sum()).backward()
    # the C-level calls on the same inputs
    zeros, ones = torch.zeros(cb + ci, device=DEV), torch.ones(cb + ci, device=DEV)
    o1, s1 = fb.concat_bn_forward(smap, "bv", bev.detach(), img.detach(), None, _t(dbv.beta), zeros.clone(),
                                  ones.clone(), eps=EPS, decay=DECAY, training=True)
    o2, s2 = fb.concat_bn_forward(smap, "img", img.detach(), bev.detach(), None, _t(dim.beta), zeros.clone(),
                                  ones.clone(), eps=EPS, decay=DECAY, training=True)
    assert torch.equal(bv_f.detach(), o1) and torch.equal(img_f.detach(), o2)
    p1, r1, db1, _ = fb.concat_bn_backward(smap, "bv", bev.detach(), img.detach(), g_bv, s1, training=True)
    p2, r2, db2, _ = fb.concat_bn_backward(smap, "img", img.detach(), bev.detach(), g_img, s2, training=True)
    assert torch.equal(bev.grad, p1 + r2) and torch.equal(img.grad, p2 + r1)
    assert torch.equal(mod.beta_bv.grad, db1) and torch.equal(mod.beta_img.grad, db2)
    for side in ("bv", "img"):
        for half in mod.halves(side):
            assert half.numel() == 32
        assert mod.params[side]["beta"].grad.abs().min() > 0  # every beta of both halves got a gradient
    # the moving statistics moved (training) and the drop-in entry binds to the module
    assert not torch.equal(mod.params["bv"]["moving_mean"], zeros)
    from sparse_pooling_amd import sparse_pool_utils as spu
    m = dbv.m
    M = spu.SparseTensor(_t(m.mij), _t(m.mval), m.m_size)
    mod2 = fb.FusionConcatBN(cb, ci, eps=EPS, decay=DECAY, device=DEV)
    with torch.no_grad():
        mod2.beta_bv.copy_(_t(dbv.beta))
        mod2.beta_img.copy_(_t(dim.beta))
    b2, i2 = spu.sparse_pool_layer_bn([bev.detach(), img.detach()], [ci, cb], M, img_index_flip=_t(m.idx), bv_index=1,
                                      bn=mod2, training=True)
    assert torch.equal(b2, o1) and torch.equal(i2, o2)
    with pytest.raises(TypeError):  # the reference's own name keeps failing as the reference does
        spu.sparse_pool_layer([bev.detach(), img.detach()], [ci, cb], M, img_index_flip=_t(m.idx), use_bn=True)


def test_autograd_bf16_rounds_the_source_gradient_once():
    """bf16 maps through the module (one direction, gamma trained): the image's gradient is the C-level f32
    source gradient rounded once to bf16, bev's the C-level g_pass, beta's and gamma's the C-level sums."""
    from sparse_pooling_amd import fusion_bn as fb
    kind, shape, dt, cb, ci = "sparse", "small", BF16, 12, 12
    smap, d = _smap(kind, shape), _case(kind, shape, dt, 12, 12, "bv")
    mod = fb.FusionConcatBN(cb, ci, eps=EPS, decay=DECAY, scale=True, dtype=torch.bfloat16, device=DEV)
    with torch.no_grad():
        mod.beta_bv.copy_(_t(d.beta))
        mod.gamma_bv.copy_(_t(d.gamma))
    bev, img = _t(d.pass_, dt).requires_grad_(True), _t(d.src, dt).requires_grad_(True)
    bv_f, img_f = mod(bev, img, smap, dual=False, is_training=True)
    assert img_f is img and bv_f.dtype == torch.bfloat16
    g = _t(d.g, dt).view_as(bv_f)
    bv_f.backward(g)
    _, save = fb.concat_bn_forward(smap, "bv", bev.detach(), img.detach(), _t(d.gamma), _t(d.beta),
                                   torch.zeros(cb + ci, device=DEV), torch.ones(cb + ci, device=DEV), eps=EPS,
                                   decay=DECAY, training=True)
    p, r, db, dg = fb.concat_bn_backward(smap, "bv", bev.detach(), img.detach(), g, save, gamma=_t(d.gamma))
    assert r.dtype == torch.float32 and img.grad.dtype == torch.bfloat16
    assert torch.equal(bev.grad, p) and torch.equal(img.grad, r.to(torch.bfloat16))
    assert torch.equal(mod.beta_bv.grad, db) and torch.equal(mod.gamma_bv.grad, dg)


@pytest.mark.parametrize("dt", [F32, BF16])
def test_composition_cross_check(dt):
    """The fused training forward against the pieces the library already had, on the device: shpl_map.layer
    (the plain concat), then fusion_conv.batch_norm_train fed the host's double statistics of the oracle map.
    Each is within its forward bound of the oracle, so they are within the sum of the two bounds of each
    other. bf16: the plain concat stores the pooled half rounded to bf16, which the fused form never does;
    the composition's input is off by up to 2^-8 * |pooled| there (half an ulp of 2^-7 at the bottom of a
    binade, the rounding the 2^-8 * |y_ref| of the forward bound stands for), k = |gamma| / sqrt(var + eps)
    times that after the BatchNorm, which is added to the composition's bound. f32: the two forms do the same
    rounded operations on the same run sums."""
    from sparse_pooling_amd import fusion_conv as fc
    from sparse_pooling_amd import shpl_map as sm
    kind, shape, cb, ci = "sparse", "large", 32, 32
    smap = _smap(kind, shape)
    for side in ("bv", "img"):
        d = _case(kind, shape, dt, cb, ci, side)
        y = _run_fwd(kind, shape, dt, d, side, True, True)[0]
        bev, img = (_t(d.pass_, dt), _t(d.src, dt)) if side == "bv" else (_t(d.src, dt), _t(d.pass_, dt))
        plain = sm.layer(bev, img, smap, dual=True)[0 if side == "bv" else 1].reshape(-1, d.c)
        stats = np.stack([d.x64.sum(0), (d.x64 * d.x64).sum(0)])
        yc = fc.batch_norm_train(plain, _t(stats), d.rows, eps=EPS, gamma=_t(d.gamma), beta=_t(d.beta), relu=False,
                                 out=torch.empty_like(plain))
        ref = _ref_fwd(d, True, True)
        b = _fwd_bound(dt, d, True, True, ref.y)
        extra = 0.0
        if dt == BF16:
            k = np.abs(d.gamma.astype(np.float64)) / np.sqrt(d.x64.var(0) + EPS)
            extra = 2.0 ** -8 * np.abs(d.x64) * k
            extra[:, :d.c_pass] = 0.0
        _within(_np(y), _np(yc).astype(np.float64), 2 * b + extra, (side, dt), "composition")
