"""FusionHead -- MV3D's 1x1 RPN heads with the SHPL applied after the projection (shpl_head1x1 and its
gradients) -- against the CPU oracle on MI355X.

Reference: the oracle's bit-exact bv_fused = [lidar || sparse_pool(M, img)] (orc.sparse_pool_layer, inputs
pre-rounded to bf16 for the bf16 cases), then the heads in float64: einsum with the weights plus the bias.
Gradients the same way: g . W^T, its image half pulled back with the oracle's transposed op, and fused^T . g.

Tolerance (derived, not tuned): any summation order of n f32 terms satisfies |err| <= 1.01 (n + 2) 2^-24 S, S
the same expression over absolute values (the oracle on |img|, |m|, |lidar|, |W|, |g|):
    forward            n = c_lidar + c_img + L
    input gradients    n = c_out + L
    weight / bias      n = rows summed + L   (the BEV cells for the lidar rows and the bias, the pixels for the
                                              image rows: the rows each sum runs over)
L: the longest run of the map (over both keys). A bf16 store adds |ref| 2^-8. __call__ is held to the heads of
the map it is given (bf16: the oracle's bv_fused rounded once, which the materialised map equals bitwise), with
L = 0: nothing is pooled inside it.
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


# ------------------------------------------------------------------ the maps
def _small_P(im_size):
    """KITTI_P2 scaled so that the synthetic points project into an im_size (W, H) image."""
    P = synth.KITTI_P2.copy()
    P[0] *= im_size[0] / 1200.0
    P[1] *= im_size[1] / 360.0
    return P


def _frames_map(n_points, bev_hw, img_hw, seed):
    """Frames of n_points[f] points over a bev_hw BEV map and an img_hw image at stride [8, 2] (MV3D's): the
    device map of the index builder and the oracle's reference-format map of every frame."""
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

    def rebuild():
        return sm.build_index_batch(pts, vox, off, Pd, spec.im_size, spec.bv_size, spec.stride, maxp).map
    return ib.map, refs, rebuild


def _grouped_map():
    from sparse_pooling_amd import shpl_map as sm
    m = gm.make()

    def build():
        return sm.pack_map(_t(m["mij"]), _t(m["mval"]), m["m_size"], _t(m["idx"]), m["img_shape"])
    return build(), [(m["mij"], m["mval"], m["m_size"], m["idx"])], build


# name -> (map kind, c_lidar, c_img, heads)
CASES = {
    "grouped-5+6-4,14": ("grouped", 5, 6, (4, 14)),      # channel tails in both sources, scalar row loads
    "grouped-16+24-1": ("grouped", 16, 24, (1,)),        # c_out at the bottom of its range
    "grouped-16+24-32": ("grouped", 16, 24, (32,)),      # ... and at the top
    # 126 cells: no multiple of a row tile, two GEMM workgroups; frame offsets; whole 16-byte K steps in both dtypes
    "ragged-2frames-64+128-4,14": ("ragged", 64, 128, (4, 14)),
    "k768+768-4,14": ("wide", 768, 768, (4, 14)),        # the real K loop at a tiny spatial size
}
PARAMS = [(c, d) for c in CASES for d in ("f32", "bf16")]
IDS = [f"{c}-{d}" for c, d in PARAMS]


class Case:
    pass


@functools.lru_cache(maxsize=None)
def _case(name, dtype):
    """Inputs, the device map and every float64 reference of one case, computed once."""
    kind, ca, cb, heads = CASES[name]
    bf = dtype == "bf16"
    c = Case()
    c.bf, c.dt, c.ca, c.cb, c.heads = bf, torch.bfloat16 if bf else torch.float32, ca, cb, heads
    rng = np.random.default_rng(list(CASES).index(name) + 7)
    if kind == "grouped":
        c.smap, c.refs, c.rebuild = _grouped_map()
        img, lidar = gm.features(cb, ca)
        c.bev_hw, c.img_hw = gm.BEV_HW, gm.IMG_HW
    else:
        n_points, c.bev_hw, c.img_hw = ((40, 3), (7, 9), (3, 10)) if kind == "ragged" else ((60,), (5, 6), (3, 10))
        c.smap, c.refs, c.rebuild = _frames_map(n_points, c.bev_hw, c.img_hw, seed=900)
        F = len(n_points)
        lidar = rng.standard_normal((F,) + c.bev_hw + (ca,)).astype(np.float32)
        img = rng.standard_normal((F,) + c.img_hw + (cb,)).astype(np.float32)
    F = len(c.refs)
    co = sum(heads)
    w = [rng.uniform(-0.5, 0.5, (1, 1, ca + cb, n)).astype(np.float32) for n in heads]
    bias = [rng.standard_normal(n).astype(np.float32) * 0.5 for n in heads]
    g = [rng.standard_normal((F,) + c.bev_hw + (n,)).astype(np.float32) for n in heads]
    if bf:
        lidar, img, w, g = _rd(lidar), _rd(img), [_rd(v) for v in w], [_rd(v) for v in g]
    c.lidar, c.img, c.w, c.bias, c.g = lidar, img, w, bias, g
    W = np.concatenate([v.reshape(ca + cb, -1) for v in w], 1).astype(np.float64)
    B = np.concatenate(bias).astype(np.float64)
    G = np.concatenate([v.reshape(-1, v.shape[-1]) for v in g], 1).astype(np.float64)
    c.W, c.B, c.G = W, B, G
    R, Pn = int(np.prod(c.bev_hw)), int(np.prod(c.img_hw))
    c.R, c.Pn, c.F = R, Pn, F

    # the longest run of the map, over both keys
    L = 0
    for mij, mval, m_size, idx in c.refs:
        mij, idx = np.asarray(mij).reshape(-1, 2), np.asarray(idx).reshape(-1, 3)
        if len(mij):
            pix = idx[mij[:, 1], 1] * c.img_hw[1] + idx[mij[:, 1], 2]
            L = max(L, int(np.bincount(mij[:, 0]).max()), int(np.bincount(pix).max()))
    c.L = L

    def fused_of(lid, im, absval):
        out = []
        for f, (mij, mval, m_size, idx) in enumerate(c.refs):
            mv = np.abs(mval) if absval else mval
            bv, _ = orc.sparse_pool_layer(lid[f:f + 1], im[f:f + 1], mij, mv, m_size, idx)
            out.append(bv.reshape(R, ca + cb))
        return np.concatenate(out).astype(np.float64)

    def to_pixels(dY, absval):
        out = []
        for f, (mij, mval, m_size, idx) in enumerate(c.refs):
            mv = np.abs(mval) if absval else mval
            d = orc.sparse_pool_grad_img(mij, mv, m_size, dY[f * R:(f + 1) * R].astype(np.float32), idx,
                                         (1,) + tuple(c.img_hw))
            out.append(d.reshape(Pn, -1))
        return np.concatenate(out).astype(np.float64)

    c.fused_of = fused_of
    fused, fabs = fused_of(lidar, img, False), fused_of(np.abs(lidar), np.abs(img), True)
    c.fused = fused
    aW, aG = np.abs(W), np.abs(G)
    store = (lambda ref: np.abs(ref) * 2.0 ** -8) if bf else (lambda ref: 0.0)
    c.out = fused @ W + B
    c.out_bound = _bound(fabs @ aW + np.abs(B), ca + cb + L) + store(c.out)
    # __call__ reads the materialised map, whose bf16 form is the oracle's rounded once: that map is its input
    c.fused_mat = _rd(fused.astype(np.float32)).astype(np.float64) if bf else fused
    c.out_mat = c.fused_mat @ W + B
    c.out_mat_bound = _bound(np.abs(c.fused_mat) @ aW + np.abs(B), ca + cb) + store(c.out_mat)
    # input gradients
    dfused, dfabs = G @ W.T, aG @ aW.T
    c.d_fused = dfused
    c.d_fused_bound = _bound(dfabs, co) + store(dfused)
    c.d_lidar = dfused[:, :ca]
    c.d_lidar_bound = _bound(dfabs[:, :ca], co + L) + store(c.d_lidar)
    c.d_img = to_pixels(dfused[:, ca:], False)
    c.d_img_bound = _bound(to_pixels(dfabs[:, ca:], True), co + L) + store(c.d_img)
    # weight and bias gradients
    c.dW = fused.T @ G
    S = fabs.T @ aG
    n_rows = np.concatenate([np.full(ca, F * R), np.full(cb, F * Pn)]).reshape(-1, 1)
    c.dW_bound = _bound(S, n_rows + L) + store(c.dW)
    c.dW_mat = c.fused_mat.T @ G  # the one-map form sums the cells for every channel
    c.dW_mat_bound = _bound(np.abs(c.fused_mat).T @ aG, F * R) + store(c.dW_mat)
    c.dB = G.sum(0)
    c.dB_bound = _bound(aG.sum(0), F * R + L)
    return c


def _head(c):
    from sparse_pooling_amd import fusion_head as fh
    head = fh.FusionHead(c.ca, c.cb, heads=c.heads, dtype=c.dt, device=DEV, seed=5)
    assert [tuple(w.shape) for w in head.weights] == [(1, 1, c.ca + c.cb, n) for n in c.heads]
    assert all(w.dtype == c.dt for w in head.weights)
    assert all(b.dtype == torch.float32 and not bool(b.any()) for b in head.biases)  # zero-initialised
    head.weights = [_t(w).to(c.dt) for w in c.w]
    head.biases = [_t(b) for b in c.bias]
    return head


def _cat(outs):
    return torch.cat([o.reshape(-1, o.shape[-1]) for o in outs], 1)


@pytest.mark.parametrize("name,dtype", PARAMS, ids=IDS)
def test_forward(name, dtype):
    """fused, __call__ on the materialised map and the raw shpl_head1x1 call against the float64 heads of the
    oracle's bv_fused; a CSR without key ranges gives the same bits; two runs give the same bits."""
    from sparse_pooling_amd import _lib as L, fusion_head as fh, shpl_map as sm
    c = _case(name, dtype)
    head = _head(c)
    tl, ti = _t(c.lidar).to(c.dt), _t(c.img).to(c.dt)
    outs = head.fused(tl, ti, c.smap)
    assert [tuple(o.shape) for o in outs] == [tuple(tl.shape[:3]) + (n,) for n in c.heads]
    assert all(o.dtype == c.dt for o in outs)
    mat = sm.pool_img_to_bev(c.smap, ti, tl.shape, bev=tl)
    outs_mat = head(mat)
    wcat = torch.cat([w.reshape(c.ca + c.cb, -1) for w in head.weights], 1)
    raw = fh.head1x1(tl, wcat, b=ti, pool=c.smap.csr(L.BY_CELL, L.ORDER_ENTRY), bias=torch.cat(head.biases))
    flat = c.rebuild()
    flat.ROW_PULLS = False  # the CSR of the flat builders: no key_range, the head builds the ranges itself
    assert flat.csr(L.BY_CELL, L.ORDER_ENTRY).key_range is None and c.smap.csr(L.BY_CELL, L.ORDER_ENTRY).key_range is not None
    outs_flat = head.fused(tl, ti, flat)
    again = head.fused(tl, ti, c.smap)
    torch.cuda.synchronize()
    assert c.smap.error_bits() == 0 and flat.error_bits() == 0
    np.testing.assert_array_equal(_np(mat).reshape(-1, c.ca + c.cb), c.fused_mat)  # the oracle's bv_fused, bitwise
    _within("fused", _np(_cat(outs)), c.out, c.out_bound)
    _within("__call__(materialised)", _np(_cat(outs_mat)), c.out_mat, c.out_mat_bound)
    assert torch.equal(raw.reshape(-1, sum(c.heads)), _cat(outs)), "shpl_head1x1 differs from FusionHead.fused"
    assert torch.equal(_cat(outs_flat), _cat(outs)), "the ranges built in the workspace give other sums"
    assert all(torch.equal(a, b) for a, b in zip(again, outs)), "two forward runs differ"
    with pytest.raises(NotImplementedError, match="mv3d.sparse_pool"):
        head.fused(tl, ti, c.smap, keep_prob=0.5)
    with pytest.raises(L.ShplLibraryError):
        head.fused(tl.cpu(), ti.cpu(), c.smap)


def _backward(c, head, materialised):
    tl = _t(c.lidar).to(c.dt).requires_grad_(True)
    ti = _t(c.img).to(c.dt).requires_grad_(True)
    for p in (*head.weights, *head.biases):
        p.requires_grad_(True)
        p.grad = None
    if materialised:
        from sparse_pooling_amd import shpl_map as sm
        x = sm.pool_img_to_bev(c.smap, ti.detach(), tl.shape, bev=tl.detach()).requires_grad_(True)
        outs = head(x)
        leaves = (x,)
    else:
        outs = head.fused(tl, ti, c.smap)
        leaves = (tl, ti)
    torch.autograd.backward(outs, [_t(g).to(c.dt) for g in c.g])
    return [t.grad for t in leaves], [w.grad for w in head.weights], [b.grad for b in head.biases]


@pytest.mark.parametrize("name,dtype", PARAMS, ids=IDS)
def test_backward(name, dtype):
    """d_lidar, d_img, every dW and every dbias of fused (and of __call__ over the materialised map) against
    the float64 gradients; two runs give the same bits."""
    c = _case(name, dtype)
    head = _head(c)
    (d_lidar, d_img), dws, dbs = _backward(c, head, False)
    (d_lidar2, d_img2), dws2, dbs2 = _backward(c, head, False)
    (d_map,), dws_m, dbs_m = _backward(c, head, True)
    torch.cuda.synchronize()
    assert c.smap.error_bits() == 0
    assert d_lidar.dtype == c.dt and d_img.dtype == c.dt and d_lidar.shape[-1] == c.ca and d_img.shape[-1] == c.cb
    assert all(w.shape == p.shape and w.dtype == c.dt for w, p in zip(dws, head.weights))
    assert all(b.dtype == torch.float32 for b in dbs)
    _within("d_lidar", _np(d_lidar), c.d_lidar, c.d_lidar_bound)
    _within("d_img", _np(d_img), c.d_img, c.d_img_bound)
    dW = np.concatenate([_np(w).reshape(c.ca + c.cb, -1) for w in dws], 1)
    _within("dW", dW, c.dW, c.dW_bound)
    _within("dbias", np.concatenate([_np(b) for b in dbs]), c.dB, c.dB_bound)
    for a, b in zip((d_lidar, d_img, *dws, *dbs), (d_lidar2, d_img2, *dws2, *dbs2)):
        assert torch.equal(a, b), "two backward runs differ"
    _within("d_map (materialised)", _np(d_map), c.d_fused, c.d_fused_bound)
    _within("dW (materialised)", np.concatenate([_np(w).reshape(c.ca + c.cb, -1) for w in dws_m], 1), c.dW_mat,
            c.dW_mat_bound)
    _within("dbias (materialised)", np.concatenate([_np(b) for b in dbs_m]), c.dB, c.dB_bound)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_bound_sees_a_missing_planted_entry(dtype):
    """Dropping any one planted entry of the grouped map from the reference moves it outside the forward bound
    at that entry's cell: the bound can see a missing term."""
    c = _case("grouped-5+6-4,14", dtype)
    mij, mval, m_size, idx = c.refs[0]
    planted = [(r, k) for (k1, k2, k3), (ra, (rb1, rb2), rc) in zip(gm.PLANT_COLS, gm.PLANT_ROWS)
               for r, k in ((ra, k1), (rb1, k2), (rb2, k2), (rc, k3))]
    seen = 0
    for r, k in planted:
        e = int(np.flatnonzero((mij[:, 0] == r) & (mij[:, 1] == k))[0])
        keep = np.arange(len(mij)) != e
        bv, _ = orc.sparse_pool_layer(c.lidar, c.img, mij[keep], mval[keep], m_size, idx)
        out = bv.reshape(c.R, -1).astype(np.float64) @ c.W + c.B
        d = np.abs(out - c.out)
        assert not (d[np.arange(c.R) != r] > 0).any()  # only that cell moves
        assert (d[r] > c.out_bound[r]).any(), f"dropping entry ({r}, {k}) stays inside the bound"
        seen += 1
    assert seen == 12


def test_empty_map_csr_keeps_its_padding_slot_empty():
    """The CSR of an empty map (nnz_cap 0) holds one padding slot that no builder writes and that the
    torch.ops.shpl operators count as capacity: it must read as an empty slot (ent_dst -1) whatever block the
    allocator recycles for it -- here one that held a valid destination."""
    from sparse_pooling_amd import _lib as L
    for _ in range(4):
        stale = torch.zeros(1, dtype=torch.int32, device=DEV)  # destination 0, then back to the allocator
        del stale
        c = L.Csr(42, 0, DEV, with_col=False, key_range=True)
        assert c.nnz_cap == 0 and c.ent_dst.numel() == 1
        assert int(c.ent_dst[0].item()) == -1
