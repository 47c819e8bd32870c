"""The image-side post-fusion conv (pyramid_fusion_pooled_img, rpn_model.py:347-354) with the BEV->image
pooling fused into its staging -- FusionConv.fused_img / fused_img_csr, shpl_conv3x3 and its gradients over the
pixel-keyed CSR, PostFusion -- vs the CPU oracle on MI355X.

The mirror of tests/test_gpu_conv.py and tests/test_gpu_conv_grad.py with the sides swapped; their helpers and
tolerances are imported, not re-derived. What the image side adds is the summation order: a pixel's pooled
vector is TF's sum of per-column partials (shpl_pull SHPL_BY_PIXEL), which the hand-made map of
tests/grouped_map.py separates from a plain sum on its planted pixels (tests/test_grouped_map_oracle.py).
"""

import numpy as np
import pytest
import torch

import grouped_map as gm
from oracle import shpl_oracle as orc
from sparse_pooling_amd import synth
from test_gpu_conv import ACC, DEV, TOL, _assert_within, _bf16, _bound, _np, _t, _weights
from test_gpu_conv_grad import _check

pytestmark = pytest.mark.gpu


def _rd(a):
    return orc.from_bf16_bits(orc.to_bf16_bits(a))


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from sparse_pooling_amd import _lib as L
    L.lib()
    assert torch.cuda.is_available()


def _oracle_frame(fr, spec):
    gen = orc.gen_sparse_pooling_input_avod(fr.points, fr.voxel_indices, fr.P, list(spec.im_size),
                                            tuple(spec.bv_size))
    return orc.produce_sparse_pooling_input(gen, stride=spec.stride)


def _conv_for(ci, cb, cout, dt, bn=True):
    """A FusionConv over [img (ci) || pooled bev (cb)] with seeded weights and epilogue (BatchNorm inference, or
    bias + ReLU as RetinaNet's)."""
    from sparse_pooling_amd import fusion_conv as fc
    conv = fc.FusionConv(ci + cb, cout, batch_norm=bn, bias=not bn, dtype=dt, device=DEV, seed=3)
    w = _weights(ci + cb, cout, 13)
    if dt == torch.bfloat16:
        w = _rd(w)
    conv.weights = _t(w).to(dt)
    if bn:
        conv.moving_mean = _t(np.random.default_rng(1).standard_normal(cout).astype(np.float32) * 0.1)
        conv.beta = _t(np.random.default_rng(2).standard_normal(cout).astype(np.float32) * 0.1)
    else:
        conv.bias = _t(np.random.default_rng(4).standard_normal(cout).astype(np.float32) * 0.5)
    return conv, w


# ------------------------------------------------------------------ 1. the grouped map, every forward form
GROUPED_FORMS = [  # dtype, c_img, c_bev, c_out, BatchNorm
    ("f32", 5, 6, 7, True),        # tiled f32, channel tails in both sources (scalar staging)
    ("f32", 16, 24, 32, True),     # tiled f32, whole staging chunks
    ("bf16", 16, 16, 32, True),    # k_conv_rows over rows::k_pool_runs' compact rows
    ("bf16", 64, 64, 256, False),  # k_conv_wide over wide::k_pool_runs_wide_k's compact rows
]


@pytest.mark.parametrize("form", GROUPED_FORMS, ids=[f"{f[0]}-{f[1]}+{f[2]}-{f[3]}" for f in GROUPED_FORMS])
def test_grouped_map_fused_img_is_the_conv_of_img_fused(form):
    """fused_img == the conv of the materialised img_fused = [img || shpl_pull(BY_PIXEL)], bitwise; that map ==
    the oracle's img_fused, bitwise (bf16: rounded once); the output within the conv bound of the oracle's conv
    of it; and the raw shpl_conv3x3 call over the pixel-keyed CSR gives the same bits. On the planted pixels
    the pooled channels are 2 * scale, which a plain sum in entry order makes 0: both comparisons fail for a
    kernel that sums a pixel's run without the per-column partials.
    5 + 6 channels: c_img is no multiple of the staging chunk, so (include/shpl.h) the one-map conv sums K in
    another order; the bitwise reference is the two-source conv over the map's two halves, as
    test_fused_conv_noncanonical_map takes it, and the one-map conv is held to the oracle bound."""
    from sparse_pooling_amd import _lib as L, fusion_conv as fc, shpl_map as sm
    dtype, ci, cb, cout, bn = form
    bf = dtype == "bf16"
    dt = torch.bfloat16 if bf else torch.float32
    m = gm.make()
    img, bev = gm.features(ci, cb)
    ti, tb = _t(img).to(dt), _t(bev).to(dt)
    smap = sm.pack_map(_t(m["mij"]), _t(m["mval"]), m["m_size"], _t(m["idx"]), img.shape)
    conv, w = _conv_for(ci, cb, cout, dt, bn)
    center, scale, shift = (None if v is None else _np(v) for v in conv._inference_epilogue())
    pool = smap.csr(L.BY_PIXEL, L.ORDER_COL_ROW)
    assert pool.ent_col is not None
    rows = fc.rows_form(ti, conv.weights, b=tb, pool=pool, frame_off=smap.frame_off, relu=True)
    assert rows == (form[:4] == ("bf16", 16, 16, 32))
    y = conv.fused_img(ti, tb, smap)
    mat = sm.pool_bev_to_img(smap, tb, ti.shape, img=ti)
    if ci % (16 if bf else 8) == 0:
        y_unf = conv(mat)
    else:
        y_unf = fc.conv3x3(mat[..., :ci].contiguous(), conv.weights, b=mat[..., ci:].contiguous(),
                           center=conv.moving_mean, scale=conv._scale, shift=conv.beta, relu=True)
    y_raw = fc.conv3x3(ti, conv.weights, b=tb, pool=pool, frame_off=smap.frame_off,
                       center=None if center is None else _t(center), scale=None if scale is None else _t(scale),
                       shift=None if shift is None else _t(shift), relu=True)
    torch.cuda.synchronize()
    assert smap.error_bits() == 0
    _, ei = orc.sparse_pool_layer(bev, img, m["mij"], m["mval"], m["m_size"], m["idx"], dual=True)
    if bf:
        ei = _rd(ei)
    for py, px in m["planted"]:  # the planted pixels carry the per-column sums
        np.testing.assert_array_equal(ei[0, py, px, ci:], 2.0 * gm.channel_scale(cb))
    np.testing.assert_array_equal(_np(mat.float()), ei)
    assert torch.equal(y, y_unf), "fused_img differs from the conv of the materialised img_fused"
    assert torch.equal(y_raw, y), "shpl_conv3x3 over the pixel-keyed CSR differs from fused_img"
    ref = orc.conv3x3(ei, w, center, scale, shift, True)
    bound = _bound(ei, w, scale)
    if bf:
        bound = bound + np.abs(ref) * 2.0 ** -8
    _assert_within(y.float(), ref, bound)
    _assert_within(conv(mat).float(), ref, bound)


def test_grouped_wide_fused_img_materialised_map():
    """The pooled wide forward past the occupancy table on the image side (image 18433 x 3: h * words per row
    = 18433 > 18432, as test_bf16_wide_fused_materialised_map's BEV grid): shpl_conv3x3 materialises the pooled
    map in its workspace with shpl_pull -- SHPL_BY_PIXEL for a pixel-keyed pool -- and reads it as a dense
    second source. Fused == the conv of [img || shpl_pull(BY_PIXEL)], bitwise; a planted cancellation triple on
    the last pixel holds 2 * scale (a cell-keyed pull of this CSR would leave 0 there)."""
    from sparse_pooling_amd import _lib as L, fusion_conv as fc, shpl_map as sm
    rng = np.random.default_rng(95)
    n, h, w, hb, wb, ci, cb, cout = 300, 18433, 3, 15, 17, 64, 64, 256
    R = hb * wb
    idx = np.stack([np.zeros(n, np.int64), rng.integers(0, h - 1, n), rng.integers(0, w, n)], 1)
    idx[:6, 1:] = [[0, 0], [0, 1], [0, 2], [h - 2, 0], [h - 2, 1], [h - 2, 2]]
    k1, k2, k3 = 50, 120, 290  # the triple's columns, alone on pixel (h - 1, 2)
    idx[[k1, k2, k3], 1:] = [h - 1, 2]
    rows = rng.integers(3, R, n)  # BEV rows 0, 1, 2 are the triple's
    extra = np.stack([rng.integers(3, R, 200), rng.integers(0, n, 200)], 1)
    extra = extra[~np.isin(extra[:, 1], [k1, k2, k3])]
    keep = ~np.isin(np.arange(n), [k1, k2, k3])
    mij = np.concatenate([np.stack([rows, np.arange(n)], 1)[keep], extra,
                          [[0, k1], [1, k2], [1, k2], [2, k3]]]).astype(np.int64)
    mval = np.concatenate([rng.uniform(0.25, 2.0, len(mij) - 4), [4096.0, 1.0, 1.0, 4096.0]]).astype(np.float32)
    perm = rng.permutation(len(mij))
    mij, mval = np.ascontiguousarray(mij[perm]), mval[perm]
    bev = _rd(rng.standard_normal((1, hb, wb, cb)).astype(np.float32))
    s = gm.channel_scale(cb)
    bev.reshape(-1, cb)[:3] = [4096.0 * s, s, -4096.0 * s]
    img = _bf16(rng.standard_normal((1, h, w, ci)).astype(np.float32))
    tb = _bf16(bev)
    smap = sm.pack_map(_t(mij), _t(mval), [R, n], _t(idx), img.shape)
    pool = smap.csr(L.BY_PIXEL, L.ORDER_COL_ROW)
    assert (fc.conv_ws_bytes(L.BF16, 1, h, w, ci, cb, cout, pool.nnz_cap, False) -
            fc.conv_ws_bytes(L.BF16, 1, h, w, ci, cb, cout, None, False)) >= h * w * cb * 2
    wts = _bf16(_weights(ci + cb, cout, 92))
    bias = _t(np.random.default_rng(93).standard_normal(cout).astype(np.float32) * 0.5)
    fused = fc.conv3x3(img, wts, b=tb, pool=pool, frame_off=smap.frame_off, shift=bias, relu=True)
    mat = sm.pool_bev_to_img(smap, tb, img.shape, img=img)
    unf = fc.conv3x3(mat[..., :ci].contiguous(), wts, b=mat[..., ci:].contiguous(), shift=bias, relu=True)
    torch.cuda.synchronize()
    assert smap.error_bits() == 0
    np.testing.assert_array_equal(_np(mat[0, h - 1, 2, ci:].float()), 2.0 * s)
    assert torch.equal(fused, unf)


# ------------------------------------------------------------------ 2. batched index-builder maps
@pytest.fixture(scope="module")
def batch3():
    """Config 1's geometry, 3 frames: a full one, an empty one, one of a single point."""
    from sparse_pooling_amd import pipeline
    spec = synth.CONFIGS[1]
    small = lambda n: synth.FrameSpec(n, spec.im_size, spec.bv_size, spec.stride, spec.c_bev, spec.c_img)  # noqa: E731
    frames = [synth.make_frame(spec, seed=520, n_outside=20), synth.make_frame(small(0), seed=521),
              synth.make_frame(small(1), seed=522)]
    Hb, Wb = spec.bev_feat_hw
    Hi, Wi = spec.img_feat_hw
    bev = synth.make_features((3, Hb, Wb, spec.c_bev), 11)
    img = synth.make_features((3, Hi, Wi, spec.c_img), 12)
    return spec, frames, pipeline.stack_frames(frames, DEV), bev, img


def test_fused_img_is_the_conv_of_img_fused_batched(batch3):
    """The mirror of test_fused_pool_conv_is_the_conv_of_bv_fused[1-3] over build_index_batch's map (identity
    columns, carried as ent_col): fused == unfused bitwise, the per-frame oracle img_fused bitwise, the conv
    within bound; frame 1 is empty, frame 2 holds one point."""
    from sparse_pooling_amd import shpl_map as sm
    spec, frames, (pts, vox, off, P, maxp, N), bev, img = batch3
    ib = sm.build_index_batch(pts, vox, off, P, spec.im_size, spec.bv_size, spec.stride, maxp)
    Ci, Cb = spec.c_img, spec.c_bev
    tb, ti = _t(bev), _t(img)
    conv, w = _conv_for(Ci, Cb, Cb, torch.float32)
    img_fused = sm.pool_bev_to_img(ib.map, tb, ti.shape, img=ti)
    y_unf = conv(img_fused)
    y_fus = conv.fused_img(ti, tb, ib.map)
    torch.cuda.synchronize()
    assert ib.map.error_bits() == 0
    assert [int(v) for v in _np(ib.frame_nnz)[1:]] == [0, 1]
    np.testing.assert_array_equal(_np(y_fus), _np(y_unf))
    center, scale, shift = (_np(v) for v in conv._inference_epilogue())
    for f, fr in enumerate(frames):
        ref = _oracle_frame(fr, spec)
        _, ei = orc.sparse_pool_layer(bev[f:f + 1], img[f:f + 1], ref["Mij_pool"], ref["M_val"], ref["M_size"],
                                      ref["img_index_flip_pool"], dual=True)
        np.testing.assert_array_equal(_np(img_fused[f:f + 1]), ei)
        _assert_within(y_fus[f:f + 1], orc.conv3x3(ei, w, center, scale, shift, True), _bound(ei, w, scale))


def test_fused_img_csr_over_bucket_built_csr_in_a_graph(batch3):
    """fused_img_csr over a FusedPipeline's bucket-built pixel CSR (identity columns flagged, no ent_col: the
    plain form, as in the pulls): bitwise the conv of the pipeline's img_fused and the ent_col form over the
    same frames; captured once in a HIP graph on one stream and replayed twice, bitwise the eager call."""
    from sparse_pooling_amd import _lib as L, pipeline, shpl_map as sm
    spec, frames, (pts, vox, off, P, maxp, N), bev, img = batch3
    Ci, Cb = spec.c_img, spec.c_bev
    tb, ti = _t(bev), _t(img)
    pl = pipeline.FusedPipeline(3, maxp, N, spec.im_size, spec.bv_size, spec.stride, Cb, Ci, dual=True)
    assert pl.buckets and pl.pcsr.ent_col is None and pl.pcsr.struct.flags == L.CSR_IDENTITY_COLS
    pl.step(pts, vox, off, P, tb, ti)
    conv, _ = _conv_for(Ci, Cb, Cb, torch.float32)
    y_eager = conv.fused_img_csr(ti, tb, pl.pcsr, pl.frame_off)
    y_map = conv(pl.img_fused)
    ib = sm.build_index_batch(pts, vox, off, P, spec.im_size, spec.bv_size, spec.stride, maxp)
    y_cols = conv.fused_img(ti, tb, ib.map)
    torch.cuda.synchronize()
    assert int(pl.err.item()) == 0
    assert torch.equal(y_eager, y_map) and torch.equal(y_eager, y_cols)
    y_graph = torch.empty_like(y_eager)
    gs = torch.cuda.Stream()
    gs.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=gs):
        conv.fused_img_csr(ti, tb, pl.pcsr, pl.frame_off, out=y_graph)
    for _ in range(2):
        y_graph.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(y_graph, y_eager)


# ------------------------------------------------------------------ 3. autograd against the oracle chain
@pytest.mark.parametrize("train", [True, False])
def test_fused_img_autograd_vs_oracle(train):
    """d(img), d(bev), d(weights), d(beta) of FusionConv.fused_img against the oracle chain: img_fused -> conv
    -> BatchNorm -> ReLU forward, and its TF gradients (BN / conv backward, then the gradient of
    _sparse_pool_trans_op for the BEV map). The mirror of test_fused_conv_autograd_vs_oracle, the roles of
    d_bev and d_img swapped in the bounds."""
    from sparse_pooling_amd import shpl_map as sm, fusion_conv as fc
    spec = synth.CONFIGS[1]
    fr = synth.make_frame(spec, seed=900, n_outside=10)
    ref = _oracle_frame(fr, spec)
    Hb, Wb = spec.bev_feat_hw
    Hi, Wi = spec.img_feat_hw
    Cb, Ci = spec.c_bev, spec.c_img
    bev = synth.make_features((1, Hb, Wb, Cb), 11)
    img = synth.make_features((1, Hi, Wi, Ci), 12)
    w = _weights(Ci + Cb, Cb, 13)
    rng = np.random.default_rng(14)
    beta = (0.1 * rng.standard_normal(Cb)).astype(np.float32)
    mm = (0.1 * rng.standard_normal(Cb)).astype(np.float32)
    mv = rng.uniform(0.5, 2.0, Cb).astype(np.float32)
    g = rng.standard_normal((1, Hi, Wi, Cb)).astype(np.float32)
    smap = sm.pack_map(_t(ref["Mij_pool"]), _t(ref["M_val"].astype(np.float32)), ref["M_size"],
                       _t(ref["img_index_flip_pool"]), img.shape)
    conv = fc.FusionConv(Ci + Cb, Cb, device=DEV)
    conv.weights = _t(w).requires_grad_(True)
    conv.beta = _t(beta).requires_grad_(True)
    conv.moving_mean, conv.moving_var = _t(mm), _t(mv)
    tb, ti = _t(bev).requires_grad_(True), _t(img).requires_grad_(True)
    y = conv.fused_img(ti, tb, smap, is_training=train)
    y.backward(_t(g))
    # oracle chain
    _, ei = orc.sparse_pool_layer(bev, img, ref["Mij_pool"], ref["M_val"], ref["M_size"],
                                  ref["img_index_flip_pool"], dual=True)
    _, raw = orc.conv3x3(ei, w, raw=True)
    mean = None if train else mm.astype(np.float64)
    var = None if train else mv.astype(np.float64)
    if train:
        ey, _, _, _, _ = orc.batch_norm_train(raw, 1e-3, None, beta, True)
        scale = 1.0 / np.sqrt(raw.reshape(-1, Cb).var(0) + 1e-3)
    else:
        scale = 1.0 / np.sqrt(mv.astype(np.float64) + 1e-3)
        ey = np.maximum((raw - mm) * scale + beta, 0.0)
    g_raw, e_db, _ = orc.batch_norm_backward(raw, g, train, mean, var, 1e-3, None, beta, True)
    g_raw32 = g_raw.astype(np.float32)
    d_if = orc.conv3x3_dgrad(g_raw32, w).astype(np.float64)
    d_bev = orc.sparse_pool_trans_grad_bev(ref["Mij_pool"], ref["M_val"], ref["M_size"],
                                           np.ascontiguousarray(d_if[..., Ci:].astype(np.float32)),
                                           ref["img_index_flip_pool"]).reshape(1, Hb, Wb, Cb)
    d_w = orc.conv3x3_wgrad(ei, g_raw32)
    _, ab_y = orc.conv3x3(np.abs(ei), np.abs(w), raw=True)
    _check(y, ey, TOL + ACC * ab_y * np.abs(scale) + 1e-5 * np.abs(ey), "y")
    gr_mag = np.abs(g_raw) + 1e-3
    wt = np.ascontiguousarray(w[::-1, ::-1].transpose(0, 1, 3, 2))
    _, ab_dx = orc.conv3x3(gr_mag.astype(np.float32), np.abs(wt), raw=True)
    _check(ti.grad, d_if[..., :Ci], TOL + 2e-5 * ab_dx[..., :Ci], "d_img")
    _check(tb.grad, d_bev, 1e-4 + 1e-4 * np.abs(d_bev), "d_bev")
    ab_w = orc.conv3x3_wgrad(np.abs(ei), gr_mag.astype(np.float32))
    _check(conv.weights.grad, d_w, TOL + 2e-5 * ab_w, "d_w")
    _check(conv.beta.grad, e_db, 1e-4 + 1e-6 * np.abs(g).reshape(-1, Cb).sum(0), "d_beta")


# ------------------------------------------------------------------ 4. bf16 training, the row-streaming form
def _train_pair(smap, bev, img, w, g, beta):
    """(fused, unfused): y, d_img, d_bev, d_w, d_beta, moving mean / variance of one bf16 training step through
    fused_img, and through the autograd graph over the materialised img_fused (sm.layer(..., dual=True)[1])."""
    from sparse_pooling_amd import fusion_conv as fc, shpl_map as sm

    def run(fused):
        conv = fc.FusionConv(int(w.shape[2]), int(w.shape[3]), dtype=torch.bfloat16, device=DEV)
        conv.weights = w.clone().requires_grad_(True)
        conv.beta = beta.clone().requires_grad_(True)
        tb, ti = bev.clone().requires_grad_(True), img.clone().requires_grad_(True)
        if fused:
            y = conv.fused_img(ti, tb, smap, is_training=True)
        else:
            y = conv(sm.layer(tb, ti, smap, dual=True)[1], is_training=True)
        y.backward(g)
        return y, ti.grad, tb.grad, conv.weights.grad, conv.beta.grad, conv.moving_mean, conv.moving_var

    return run(True), run(False)


NAMES = ("y", "d_img", "d_bev", "d_w", "d_beta", "moving_mean", "moving_var")


def _oracle_train_y(ei, w, beta):
    _, raw = orc.conv3x3(_rd(ei), w.float().cpu().numpy(), raw=True)
    return orc.batch_norm_train(raw, 1e-3, None, beta.cpu().numpy(), True)[0]


def test_fused_img_training_bf16_rows():
    """bf16 fused_img in training at config-1 geometry, 32 + 32 -> 32 channels (k_conv_rows with the statistics
    epilogue over the compact pooled rows, the weight gradient reading them back, the BEV channels' gradient
    stored at occupied pixels only and pulled back to the BEV map): output, every gradient and the moving
    statistics bitwise those of the autograd graph over the materialised img_fused; the output within the bf16
    bound of the oracle chain. The mirror of test_fused_conv_training_bf16_rows."""
    from sparse_pooling_amd import _lib as L, fusion_conv as fc, shpl_map as sm
    spec = synth.CONFIGS[1]
    fr = synth.make_frame(spec, seed=910, n_outside=10)
    ref = _oracle_frame(fr, spec)
    Hb, Wb = spec.bev_feat_hw
    Hi, Wi = spec.img_feat_hw
    Cb = Ci = 32
    bf = lambda a: torch.from_numpy(a).to(torch.bfloat16)  # noqa: E731
    bev = bf(synth.make_features((1, Hb, Wb, Cb), 21)).to(DEV)
    img = bf(synth.make_features((1, Hi, Wi, Ci), 22)).to(DEV)
    w = bf(_weights(Ci + Cb, Cb, 23)).to(DEV)
    g = bf(np.random.default_rng(24).standard_normal((1, Hi, Wi, Cb)).astype(np.float32)).to(DEV)
    smap = sm.pack_map(_t(ref["Mij_pool"]), _t(ref["M_val"].astype(np.float32)), ref["M_size"],
                       _t(ref["img_index_flip_pool"]), tuple(img.shape))
    beta = _t((0.1 * np.random.default_rng(25).standard_normal(Cb)).astype(np.float32))
    assert fc.rows_form(img, w, b=bev, pool=smap.csr(L.BY_PIXEL, L.ORDER_COL_ROW), frame_off=smap.frame_off,
                        relu=False, stats=True)
    got, want = _train_pair(smap, bev, img, w, g, beta)
    for name, u, v in zip(NAMES, got, want):
        assert torch.equal(u, v), name
    _, ei = orc.sparse_pool_layer(bev.float().cpu().numpy(), img.float().cpu().numpy(), ref["Mij_pool"],
                                  ref["M_val"], ref["M_size"], ref["img_index_flip_pool"], dual=True)
    ey = _oracle_train_y(ei, w, beta)
    _check(got[0].float(), ey, 1e-2 + 2.0 ** -7 * np.abs(ey), "y bf16")


def test_fused_img_training_bf16_rows_grouped_map():
    """The same on the grouped map (columns of several entries, several columns per pixel, the planted
    cancellation triples): the compact pooled rows the forward and the weight gradient gather are the
    per-column sums."""
    from sparse_pooling_amd import _lib as L, fusion_conv as fc, shpl_map as sm
    m = gm.make()
    img_f, bev_f = gm.features(32, 32)
    bf = lambda a: torch.from_numpy(a).to(torch.bfloat16).to(DEV)  # noqa: E731
    img, bev = bf(img_f), bf(bev_f)
    w = bf(_weights(64, 32, 23))
    g = bf(np.random.default_rng(24).standard_normal((1,) + gm.IMG_HW + (32,)).astype(np.float32))
    beta = _t((0.1 * np.random.default_rng(25).standard_normal(32)).astype(np.float32))
    smap = sm.pack_map(_t(m["mij"]), _t(m["mval"]), m["m_size"], _t(m["idx"]), img_f.shape)
    assert fc.rows_form(img, w, b=bev, pool=smap.csr(L.BY_PIXEL, L.ORDER_COL_ROW), frame_off=smap.frame_off,
                        relu=False, stats=True)
    got, want = _train_pair(smap, bev, img, w, g, beta)
    for name, u, v in zip(NAMES, got, want):
        assert torch.equal(u, v), name
    _, ei = orc.sparse_pool_layer(bev_f, img_f, m["mij"], m["mval"], m["m_size"], m["idx"], dual=True)
    for py, px in m["planted"]:
        np.testing.assert_array_equal(ei[0, py, px, 32:], 2.0 * gm.channel_scale(32))
    ey = _oracle_train_y(ei, w, beta)
    _check(got[0].float(), ey, 1e-2 + 2.0 ** -7 * np.abs(ey), "y bf16 grouped")


@pytest.mark.parametrize("stats,frames", [(True, 2), (False, 1)])
def test_dgrad_reuse_writes_occupied_pixels_only(stats, frames):
    """shpl_conv3x3_dgrad_reuse after a forward over the pixel-keyed CSR: the first map and, at every occupied
    pixel, the second map are bitwise shpl_conv3x3_dgrad's; every other pixel of the second map keeps what it
    held (a NaN fill). The mirror of test_dgrad_reuse_writes_occupied_cells_only."""
    from sparse_pooling_amd import _lib as L, fusion_conv as fc, pipeline, shpl_map as sm
    spec = synth.CONFIGS[1]
    frs = [synth.make_frame(spec, seed=931 + f, n_outside=20 * f) for f in range(frames)]
    pts, vox, off, P, maxp, N = pipeline.stack_frames(frs, DEV)
    ib = sm.build_index_batch(pts, vox, off, P, spec.im_size, spec.bv_size, spec.stride, maxp)
    smap = ib.map
    Hb, Wb = spec.bev_feat_hw
    Hi, Wi = spec.img_feat_hw
    bev = _t(synth.make_features((frames, Hb, Wb, 32), 61)).to(torch.bfloat16)
    img = _t(synth.make_features((frames, Hi, Wi, 32), 62)).to(torch.bfloat16)
    pool = smap.csr(L.BY_PIXEL, L.ORDER_COL_ROW)
    w = _t(np.random.default_rng(63).uniform(-0.1, 0.1, (3, 3, 64, 32)).astype(np.float32)).to(torch.bfloat16)
    assert fc.rows_form(img, w, b=bev, pool=pool, frame_off=smap.frame_off, relu=False, stats=stats)
    fws = L.workspace(fc.conv_ws_bytes(L.BF16, frames, Hi, Wi, 32, 32, 32, pool.nnz_cap, stats), DEV)
    st = torch.empty((2, 32), dtype=torch.float64, device=DEV) if stats else None
    fc.conv3x3(img, w, b=bev, pool=pool, frame_off=smap.frame_off, relu=False, stats=st, ws=fws)
    gy = _t(np.random.default_rng(64).standard_normal((frames, Hi, Wi, 32)).astype(np.float32)).to(torch.bfloat16)
    da, db = fc.conv3x3_dgrad(gy, w, 64, split=32)
    ws = L.workspace(fc.conv_ws_bytes(L.BF16, frames, Hi, Wi, 32, 0, 64, None, False), DEV)
    ra = torch.empty_like(da)
    rb = torch.full_like(db, float("nan"))
    L.check(L.lib().shpl_conv3x3_dgrad_reuse(L.BF16, frames, Hi, Wi, L.ptr(gy), 32, 32, L.ptr(w), 64, L.ptr(ra), 32,
                                             32, L.ptr(rb), 32, L.ptr(ws), ws.numel(), pool.ref(), L.ptr(fws),
                                             fws.numel(), int(stats), L.stream_of(DEV)), "shpl_conv3x3_dgrad_reuse")
    torch.cuda.synchronize()
    assert torch.equal(ra, da)
    dst, fo, fn = (_np(t) for t in (pool.ent_dst, smap.frame_off, ib.frame_nnz))
    occ = np.zeros(frames * Hi * Wi, dtype=bool)
    for f in range(frames):
        d = dst[fo[f]:fo[f] + fn[f]]
        occ[d[d >= 0]] = True
    occ = torch.from_numpy(occ).to(DEV)
    assert 0 < int(occ.sum()) < occ.numel()
    flat_b, flat_r = db.reshape(-1, 32), rb.reshape(-1, 32)
    assert torch.equal(flat_r[occ], flat_b[occ])
    assert bool(torch.isnan(flat_r[~occ].float()).all())


# ------------------------------------------------------------------ 5. PostFusion
@pytest.mark.parametrize("dual", [True, False])
def test_post_fusion_is_the_two_convs(dual):
    """PostFusion (both scopes of rpn_model.py:338-354, the two convs on two streams): its outputs equal the
    two convs called on their own, bev.grad and img.grad the sum of the two branches' gradients computed
    separately; dual=False (bv_index=None) convolves img itself and builds no BEV->image CSR."""
    from sparse_pooling_amd import _lib as L, fusion_conv as fc, shpl_map as sm
    spec = synth.CONFIGS[1]
    fr = synth.make_frame(spec, seed=940, n_outside=10)
    ref = _oracle_frame(fr, spec)
    Hb, Wb = spec.bev_feat_hw
    Hi, Wi = spec.img_feat_hw
    Cb, Ci = spec.c_bev, spec.c_img
    bev = _t(synth.make_features((1, Hb, Wb, Cb), 71))
    img = _t(synth.make_features((1, Hi, Wi, Ci), 72))

    def new_map():
        return sm.pack_map(_t(ref["Mij_pool"]), _t(ref["M_val"].astype(np.float32)), ref["M_size"],
                           _t(ref["img_index_flip_pool"]), tuple(img.shape))

    pf = fc.PostFusion(Cb, Ci, dual=dual, device=DEV, seed=7)
    assert pf.bev.c_out == Ci and pf.img.c_out == Cb  # feature_depths = [img depth, bev depth]
    assert pf.img.c_in == Ci + (Cb if dual else 0)
    with pytest.raises(ValueError):
        pf(bev, img, new_map(), dual=not dual)
    smap = new_map()
    bo, io = pf(bev, img, smap, dual=dual)
    torch.cuda.synchronize()
    assert ((L.BY_PIXEL, L.ORDER_COL_ROW) in smap._csr) == dual
    if not dual:
        assert all(k[0] != L.BY_PIXEL for k in smap._csr)  # no pixel-keyed CSR was built
    assert torch.equal(bo, pf.bev.fused(bev, img, smap))
    assert torch.equal(io, pf.img.fused_img(img, bev, smap) if dual else pf.img(img))
    # gradients: the two branches' add through autograd
    g_b = _t(np.random.default_rng(73).standard_normal(tuple(bo.shape)).astype(np.float32))
    g_i = _t(np.random.default_rng(74).standard_normal(tuple(io.shape)).astype(np.float32))
    tb, ti = bev.clone().requires_grad_(True), img.clone().requires_grad_(True)
    bo2, io2 = pf(tb, ti, smap, dual=dual, is_training=False)
    assert torch.equal(bo2, bo) and torch.equal(io2, io)
    torch.autograd.backward([bo2, io2], [g_b, g_i])
    torch.cuda.synchronize()
    b1, i1 = bev.clone().requires_grad_(True), img.clone().requires_grad_(True)
    pf.bev.fused(b1, i1, smap).backward(g_b)
    b2, i2 = bev.clone().requires_grad_(True), img.clone().requires_grad_(True)
    (pf.img.fused_img(i2, b2, smap) if dual else pf.img(i2)).backward(g_i)
    torch.cuda.synchronize()
    assert torch.equal(ti.grad, i1.grad + i2.grad)
    assert torch.equal(tb.grad, b1.grad + b2.grad if dual else b1.grad)
    assert ((L.BY_PIXEL, L.ORDER_COL_ROW) in smap._csr) == dual


# ------------------------------------------------------------------ 6. errors
def test_fused_img_argument_errors():
    from sparse_pooling_amd import _lib as L, fusion_conv as fc, shpl_map as sm
    m = gm.make()
    img, bev = gm.features(8, 8)
    smap = sm.pack_map(_t(m["mij"]), _t(m["mval"]), m["m_size"], _t(m["idx"]), img.shape)
    pool = smap.csr(L.BY_PIXEL, L.ORDER_COL_ROW)
    ti, tb = _t(img), _t(bev)
    w = _t(_weights(16, 8, 1))
    H, W = gm.IMG_HW
    out = torch.empty((1, H - 1, W, 8), device=DEV)
    ws = L.workspace(fc.conv_ws_bytes(L.F32, 1, H, W, 8, 8, 8, pool.nnz_cap, False), DEV)
    # a pixel pool whose n_keys is not n_frames * h * w (one image row short)
    rc = L.lib().shpl_conv3x3(L.F32, 1, H - 1, W, L.ptr(ti), 8, 0, 8, L.ptr(tb), 8, 0, 8, pool.ref(),
                              L.ptr(smap.frame_off), L.ptr(w), 8, None, None, None, L.ACT_RELU, L.ptr(out), 8, None,
                              L.ptr(ws), ws.numel(), L.stream_of(DEV))
    assert rc == L.ERR_BAD_SHAPE
    conv = fc.FusionConv(16, 8, device=DEV)
    with pytest.raises(ValueError):  # a BEV map whose rows are not the map's cells
        conv.fused_img(ti, tb[:, :-1].contiguous(), smap)
