"""FusionHead.fused_dropout / FusionHead.dropout -- MV3D's 1x1 RPN heads under dropout over conv_lidar_fused
(shpl_head1x1_drop and its gradients) -- against the CPU oracle on MI355X. The maps, inputs and the float64
references without dropout are test_gpu_head.py's cases (computed once, shared).

Reference: X = the oracle's bit-exact bv_fused = [lidar || sparse_pool(M, img)] (inputs pre-rounded to bf16 for
the bf16 cases and the map rounded once, which is the MFMA operand include/shpl.h promises bit for bit), K = the
numpy restatement of the mask (dropout_mask_ref.py), s = scale, then float64:
    out   = s (K * X) W + bias
    d_X   = s K * (G W^T)                     (lidar half: d_lidar; the whole: the materialised map's gradient)
    d_img = sum over the entries (cell r, m) of a pixel of m * d_X[r, c_lidar:]     (float64 scatter-add)
    dW    = s (K * X)^T G,   dbias = sum_r G

Tolerance (derived, not tuned): a sum of n f32 terms in any order, with k further roundings on the chain,
satisfies |err| <= 1.01 (n + k) 2^-24 S, S the same expression over absolute values; a bf16 store adds
|ref| 2^-8. Per quantity, with the sums as include/shpl.h states them:
    forward   n = c_lidar + c_img (the MFMA channel sum; the pooled operand itself is exact)
              k = 3: the product's rounding, the multiply by s, the add of the bias
    d_lidar / the map's gradient
              n = c_out (fused multiply-adds), k = 1: the multiply by s
    d_img     n = c_out + L (L: the longest run of the map), k = 2: the multiplies by s and by m
    dW        n = the BEV cells (both halves run over the cells), k = 2: the multiply by s, the f64 sum's rounding
    dbias     unchanged by dropout: test_gpu_head.py's bound
At keep_prob 1 the mask is all ones, s = 1, and the outputs meet test_gpu_head.py's own bounds: in f32 fused()'s;
in bf16 __call__'s over the materialised map, because the pooled operand is rounded to bf16 here (the contract of
include/shpl.h) and fused() never rounds it, so fused()'s reference is off by up to 2^-9 per pooled element.
"""
import functools

import numpy as np
import pytest
import torch

import dropout_mask_ref as mref
import test_gpu_head as base

pytestmark = pytest.mark.gpu

DEV = base.DEV
U = 2.0 ** -24
SEED, OTHER_SEED = 20261, (977 << 32) + 5  # the second one uses the key's high word

# (case of test_gpu_head.CASES, keep_prob): 0.5 everywhere, 0.8 (an inexact scale) and 1.0 on one case each
RUNS = [
    ("grouped-5+6-4,14", 0.5),   # channel tails; the 8-channel group straddling the lidar / pooled boundary
    ("grouped-16+24-32", 0.5),   # c_out at the top of its range
    ("grouped-16+24-32", 1.0),
    ("ragged-2frames-64+128-4,14", 0.5),  # 126 cells: two workgroups, frame offsets, empty cells
    ("ragged-2frames-64+128-4,14", 0.8),
    ("k768+768-4,14", 0.5),      # the real K loop
]
PARAMS = [(c, kp, d) for c, kp in RUNS for d in ("f32", "bf16")]
IDS = [f"{c}-keep{kp}-{d}" for c, kp, d in PARAMS]

_t, _np, _within, _cat = base._t, base._np, base._within, base._cat


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from sparse_pooling_amd import _lib as L
    L.lib()
    assert torch.cuda.is_available()


def _bound(S, n, k):
    return 1.01 * (n + k) * U * S


class Ref:
    pass


@functools.lru_cache(maxsize=None)
def _ref(name, kp, dtype):
    """The float64 references and bounds of one (case, keep_prob), computed once."""
    c = base._case(name, dtype)
    d = Ref()
    ca, cb, co = c.ca, c.cb, sum(c.heads)
    rows = c.F * c.R
    K = mref.mask(rows, ca + cb, kp, SEED).astype(np.float64)
    s = mref.scale(kp)
    d.mask, d.scale = K, s
    X, W, B, G = c.fused_mat, c.W, c.B, c.G
    aX, aW, aG = np.abs(X), np.abs(W), np.abs(G)
    store = (lambda ref: np.abs(ref) * 2.0 ** -8) if c.bf else (lambda ref: 0.0)
    d.out = s * ((K * X) @ W) + B
    d.out_bound = _bound(s * ((K * aX) @ aW) + np.abs(B), ca + cb, 3) + store(d.out)
    d.d_x = s * K * (G @ W.T)
    d_x_abs = s * K * (aG @ aW.T)
    d.d_x_bound = _bound(d_x_abs, co, 1) + store(d.d_x)

    # the image half pulled back to the pixels, in float64: entry (cell, col) of frame f adds m * d_x[cell] to the
    # pixel of its column
    def to_pixels(dY, absval):
        out = np.zeros((c.F * c.Pn, dY.shape[1]))
        for f, (mij, mval, m_size, idx) in enumerate(c.refs):
            mij, idx = np.asarray(mij).reshape(-1, 2), np.asarray(idx).reshape(-1, 3)
            if not len(mij):
                continue
            mv = np.asarray(mval, dtype=np.float64)
            mv = np.abs(mv) if absval else mv
            pix = idx[mij[:, 1], 1] * c.img_hw[1] + idx[mij[:, 1], 2]
            np.add.at(out, f * c.Pn + pix, mv[:, None] * dY[f * c.R + mij[:, 0]])
        return out

    # the scatter against the oracle's transposed op (test_gpu_head's reference of the undropped gradient)
    plain = to_pixels((G @ W.T)[:, ca:], False)
    assert np.allclose(plain, c.d_img, rtol=0, atol=1e-5 * max(1.0, float(np.abs(c.d_img).max())))
    d.d_img = to_pixels(d.d_x[:, ca:], False)
    d.d_img_bound = _bound(to_pixels(d_x_abs[:, ca:], True), co + c.L, 2) + store(d.d_img)
    d.dW = s * ((K * X).T @ G)
    d.dW_bound = _bound(s * ((K * aX).T @ aG), rows, 2) + store(d.dW)
    return d


def _inputs(c):
    return _t(c.lidar).to(c.dt), _t(c.img).to(c.dt)


@pytest.mark.parametrize("name,kp,dtype", PARAMS, ids=IDS)
def test_forward(name, kp, dtype):
    """The mask against its numpy restatement, bitwise; fused_dropout, dropout over the materialised map and the
    raw shpl_head1x1_drop call within the bound; a CSR without key ranges and a second run give the same bits;
    another seed another mask."""
    from sparse_pooling_amd import _lib as L, fusion_head as fh, shpl_map as sm
    c, d = base._case(name, dtype), _ref(name, kp, dtype)
    head = base._head(c)
    tl, ti = _inputs(c)
    rows, cc = c.F * c.R, c.ca + c.cb
    mask = fh.dropout_mask(rows, cc, kp, SEED, DEV)
    other = fh.dropout_mask(rows, cc, kp, OTHER_SEED, DEV)
    outs = head.fused_dropout(tl, ti, c.smap, kp, seed=SEED)
    assert [tuple(o.shape) for o in outs] == [tuple(tl.shape[:3]) + (n,) for n in c.heads]
    assert all(o.dtype == c.dt for o in outs)
    mat = sm.pool_img_to_bev(c.smap, ti, tl.shape, bev=tl)
    outs_mat = head.dropout(mat, kp, seed=SEED)
    wcat = torch.cat([w.reshape(cc, -1) for w in head.weights], 1)
    raw = fh.head1x1_drop(tl, wcat, kp, SEED, b=ti, pool=c.smap.csr(L.BY_CELL, L.ORDER_ENTRY),
                          bias=torch.cat(head.biases))
    flat = c.rebuild()
    flat.ROW_PULLS = False  # the CSR of the flat builders: no key_range, the head builds the ranges itself
    assert flat.csr(L.BY_CELL, L.ORDER_ENTRY).key_range is None
    outs_flat = head.fused_dropout(tl, ti, flat, kp, seed=SEED)
    again = head.fused_dropout(tl, ti, c.smap, kp, seed=SEED)
    outs_other = head.fused_dropout(tl, ti, c.smap, kp, seed=OTHER_SEED)
    torch.manual_seed(31)
    drawn = head.fused_dropout(tl, ti, c.smap, kp)  # seed=None: drawn from torch's default CPU generator
    torch.manual_seed(31)
    drawn2 = head.fused_dropout(tl, ti, c.smap, kp)
    torch.cuda.synchronize()
    assert c.smap.error_bits() == 0 and flat.error_bits() == 0
    assert mask.dtype == torch.uint8 and tuple(mask.shape) == (rows, cc)
    np.testing.assert_array_equal(mask.cpu().numpy(), d.mask.astype(np.uint8))
    np.testing.assert_array_equal(other.cpu().numpy(), mref.mask(rows, cc, kp, OTHER_SEED))
    np.testing.assert_array_equal(_np(mat).reshape(-1, cc), c.fused_mat)  # the oracle's bv_fused, bitwise
    _within("fused_dropout", _np(_cat(outs)), d.out, d.out_bound)
    _within("dropout(materialised)", _np(_cat(outs_mat)), d.out, d.out_bound)
    assert torch.equal(raw.reshape(-1, sum(c.heads)), _cat(outs)), "shpl_head1x1_drop differs from fused_dropout"
    assert torch.equal(_cat(outs_flat), _cat(outs)), "the ranges built in the workspace give other sums"
    assert all(torch.equal(a, b) for a, b in zip(again, outs)), "two forward runs differ"
    assert all(torch.equal(a, b) for a, b in zip(drawn, drawn2)), "torch.manual_seed does not govern seed=None"
    if kp == 1.0:
        assert bool(mask.all()) and bool(other.all())
        if not c.bf:  # f32: the operand is the unrounded run sum, as in fused()
            _within("fused_dropout at keep 1 (fused()'s bound)", _np(_cat(outs)), c.out, c.out_bound)
        # bf16: the pooled operand is rounded to bf16 (the materialised map's element), which fused() never does,
        # so fused()'s reference does not apply; both forms are held to the heads of the rounded map instead
        _within("fused_dropout at keep 1 (__call__'s bound)", _np(_cat(outs)), c.out_mat, c.out_mat_bound)
        _within("dropout at keep 1 (__call__'s bound)", _np(_cat(outs_mat)), c.out_mat, c.out_mat_bound)
        assert all(torch.equal(a, b) for a, b in zip(outs_other, outs))
    else:
        assert not torch.equal(mask, other), "two seeds give one mask"
        assert not torch.equal(_cat(outs_other), _cat(outs))
        assert not all(torch.equal(a, b) for a, b in zip(drawn, outs))
    with pytest.raises(L.ShplLibraryError):
        head.fused_dropout(tl.cpu(), ti.cpu(), c.smap, kp, seed=SEED)
    with pytest.raises(L.ShplLibraryError):
        fh.dropout_mask(4, 8, kp, SEED, "cpu")
    with pytest.raises(ValueError):
        head.fused_dropout(tl, ti, c.smap, 0.0, seed=SEED)


def _backward(c, head, kp, smap, materialised=False):
    tl, ti = _inputs(c)
    tl.requires_grad_(True)
    ti.requires_grad_(True)
    for p in (*head.weights, *head.biases):
        p.requires_grad_(True)
        p.grad = None
    if materialised:
        from sparse_pooling_amd import shpl_map as sm
        x = sm.pool_img_to_bev(smap, ti.detach(), tl.shape, bev=tl.detach()).requires_grad_(True)
        outs = head.dropout(x, kp, seed=SEED)
        leaves = (x,)
    else:
        outs = head.fused_dropout(tl, ti, smap, kp, seed=SEED)
        leaves = (tl, ti)
    torch.autograd.backward(outs, [_t(g).to(c.dt) for g in c.g])
    return [t.grad for t in leaves], [w.grad for w in head.weights], [b.grad for b in head.biases]


@pytest.mark.parametrize("name,kp,dtype", PARAMS, ids=IDS)
def test_backward(name, kp, dtype):
    """d_lidar, d_img, every dW and dbias of fused_dropout (and of dropout over the materialised map) against
    the float64 gradients; d_lidar is exactly zero on the dropped elements and nowhere else; two runs, and a CSR
    without key ranges, give the same bits."""
    c, d = base._case(name, dtype), _ref(name, kp, dtype)
    head = base._head(c)
    cc = c.ca + c.cb
    (d_lidar, d_img), dws, dbs = _backward(c, head, kp, c.smap)
    (d_lidar2, d_img2), dws2, dbs2 = _backward(c, head, kp, c.smap)
    flat = c.rebuild()
    flat.ROW_PULLS = False
    (d_lidar3, d_img3), dws3, dbs3 = _backward(c, head, kp, flat)
    (d_map,), dws_m, dbs_m = _backward(c, head, kp, c.smap, materialised=True)
    torch.cuda.synchronize()
    assert c.smap.error_bits() == 0 and flat.error_bits() == 0
    assert d_lidar.dtype == c.dt and d_img.dtype == c.dt and d_lidar.shape[-1] == c.ca and d_img.shape[-1] == c.cb
    assert all(w.shape == p.shape and w.dtype == c.dt for w, p in zip(dws, head.weights))
    assert all(b.dtype == torch.float32 for b in dbs)
    _within("d_lidar", _np(d_lidar), d.d_x[:, :c.ca], d.d_x_bound[:, :c.ca])
    _within("d_img", _np(d_img), d.d_img, d.d_img_bound)
    _within("dW", np.concatenate([_np(w).reshape(cc, -1) for w in dws], 1), d.dW, d.dW_bound)
    _within("dbias", np.concatenate([_np(b) for b in dbs]), c.dB, c.dB_bound)
    got, kept = _np(d_lidar).reshape(-1, c.ca), d.mask[:, :c.ca] != 0
    assert not got[~kept].any(), "a dropped element of lidar has a gradient"
    assert got[kept].all(), "a kept element of lidar has none"
    for a, b in zip((d_lidar, d_img, *dws, *dbs), (d_lidar2, d_img2, *dws2, *dbs2)):
        assert torch.equal(a, b), "two backward runs differ"
    for a, b in zip((d_lidar, d_img, *dws, *dbs), (d_lidar3, d_img3, *dws3, *dbs3)):
        assert torch.equal(a, b), "the ranges built in the workspace give other gradients"
    _within("d_map (materialised)", _np(d_map), d.d_x, d.d_x_bound)
    _within("dW (materialised)", np.concatenate([_np(w).reshape(cc, -1) for w in dws_m], 1), d.dW, d.dW_bound)
    _within("dbias (materialised)", np.concatenate([_np(b) for b in dbs_m]), c.dB, c.dB_bound)
    if kp == 1.0:  # the undropped gradients' own bounds
        _within("d_lidar at keep 1", _np(d_lidar), c.d_lidar, c.d_lidar_bound)
        _within("d_img at keep 1", _np(d_img), c.d_img, c.d_img_bound)
