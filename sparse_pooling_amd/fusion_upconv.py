"""After-VGG fusion: the SHPL over conv4, fused into upconv3 (a 3x3 stride-2 transposed conv), over libshpl.

With ``rpn_sparse_pooling_after_vgg`` (and ``rpn_dual_sparse_pooling_after_vgg``) the reference fuses the two
stride-8 maps right after VGG's conv4 and hands each fused map to the pyramid's first upconv
(avod/avod/core/feature_extractors/fusion_vgg_pyramid.py:53-60, :198-206):

    conv4_bev, conv4_img = sparse_pool_layer([conv4_bev, conv4_img], ...)
    upconv3 = slim.conv2d_transpose(conv4, vgg_conv3[1], [3, 3], stride=2,
                                    normalizer_fn=slim.batch_norm,
                                    normalizer_params={'is_training': is_training})

slim defaults, as for ``FusionConv``: SAME padding, ReLU, no bias under the normalizer; slim.batch_norm with beta,
no gamma, epsilon 1e-3, decay 0.999. The variable is ``[3, 3, c_out, c_in]`` ("HWOI"). TF evaluates
conv2d_transpose as conv2d_backprop_input of the SAME stride-2 conv over the 2h x 2w output (pad_before =
pad_total // 2 = 0, pad_after = 1):

    out[f, oy, ox, co] = sum over (i, ky): 2i + ky = oy, (j, kx): 2j + kx = ox, ci of x[f, i, j, ci] W[ky, kx, co, ci]

``FusionUpconv.fused(bev, img, smap)`` computes upconv3 of [bev || pool(img)] straight from the img->BEV CSR
(shpl_upconv3x3): the fused conv4 never reaches HBM, and the result is bitwise that of the materialised map.
``fused_img`` is the image side from the BEV->img CSR. ``AfterVggFusion`` holds both upconv3 scopes.

The backward (``FusionUpconv(backward=...)``), after BatchNorm/ReLU backward over the 2h x 2w rows:

``"direct"`` (the default): the transposed conv's own gradient kernels on the raw output's gradient --
``upconv3x3_dgrad`` (shpl_upconv3x3_dgrad: the nine taps over the four parity planes of gy, one staged chunk
feeding up to four blocks of 32 input channels; the pooled half written to a dense map and carried back to the
pooled source by the side's pull) and ``upconv3x3_wgrad`` (shpl_upconv3x3_wgrad: the pooled channels recomputed
from the CSR in the staging, never stored). 9 c_in c_out multiply-adds per input pixel each.

``"phases"``: the four output parities (oy & 1, ox & 1) are four stride-1 convs over the 2 x 2 window
x[i-1..i, j-1..j]; ``phase_weights`` writes them as ONE stride-1 3x3 SAME conv to 4 c_out channels whose taps are
9 of 36 nonzero, and the gradients go through ``space_to_depth``, shpl_conv3x3_dgrad and shpl_conv3x3_wgrad with
``phase_weights(W)``, the weight gradient gathered back to HWOI by ``phase_weight_grad``. 4x the MFMA work (the
zero taps are multiplied too); kept as the comparator of the direct route (scripts/time_upconv.py, DESIGN.md §8
item 6). ``FusionUpconv.forward_phases`` is the forward by the same route, in the same spirit.
One stream, plain calls; neither route stores the fused map.
"""
from __future__ import annotations

import torch

from . import _lib as L
from .fusion_conv import (FusionConv, _beta_bias_grads, _bn_relu_backward, _Call, _fused_call, _pull_back,
                          _split_outputs, _TwoScopes, _wgrad_call, batch_norm_train, conv3x3, conv3x3_dgrad,
                          conv3x3_wgrad)

_UPCONV = _Call("shpl_upconv3x3", 2, 3, 2, "transposed conv", " (HWOI)")  # HWOI weights, 2H x 2W out

# Per axis: tap k' of the stride-1 phase conv (it reads x[i + k' - 1]) -> tap k of the transposed conv, by
# output parity. Parity 0 (o = 2i): k = 0 from x[i] (k' = 1), k = 2 from x[i-1] (k' = 0); parity 1 (o = 2i + 1):
# k = 1 from x[i] (k' = 1). Everything else is zero.
_KMAP = ({1: 0, 0: 2}, {1: 1})


def _phase_taps():
    """(ky', kx', parity block 2 py + px, ky, kx) of the 9 nonzero taps."""
    return [(kyp, kxp, 2 * py + px, ky, kx)
            for py in (0, 1) for px in (0, 1)
            for kyp, ky in _KMAP[py].items() for kxp, kx in _KMAP[px].items()]


def phase_weights(weights):
    """HWOI [3,3,c_out,c_in] -> the HWIO [3,3,c_in,4*c_out] weights of the stride-1 3x3 SAME conv that computes
    the four output parities as channel blocks (2*py + px)*c_out + co."""
    c_out, c_in = int(weights.shape[2]), int(weights.shape[3])
    out = weights.new_zeros((3, 3, c_in, 4 * c_out))
    for kyp, kxp, blk, ky, kx in _phase_taps():
        out[kyp, kxp, :, blk * c_out:(blk + 1) * c_out] = weights[ky, kx].transpose(0, 1)
    return out


def phase_weight_grad(dw_phase):
    """The adjoint of ``phase_weights``: HWIO [3,3,c_in,4*c_out] -> HWOI [3,3,c_out,c_in] (every HWOI element
    is read from the one phase tap that holds it)."""
    c_in, c_out = int(dw_phase.shape[2]), int(dw_phase.shape[3]) // 4
    out = dw_phase.new_empty((3, 3, c_out, c_in))
    for kyp, kxp, blk, ky, kx in _phase_taps():
        out[ky, kx] = dw_phase[kyp, kxp, :, blk * c_out:(blk + 1) * c_out].transpose(0, 1)
    return out


def depth_to_space(y):
    """[B,h,w,4c] (channel blocks (2*py + px)*c + co) -> [B,2h,2w,c]."""
    B, h, w, c4 = (int(s) for s in y.shape)
    c = c4 // 4
    return y.reshape(B, h, w, 2, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * h, 2 * w, c)


def space_to_depth(y):
    """[B,2h,2w,c] -> [B,h,w,4c], the inverse of ``depth_to_space``."""
    B, h2, w2, c = (int(s) for s in y.shape)
    return y.reshape(B, h2 // 2, 2, w2 // 2, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(B, h2 // 2, w2 // 2, 4 * c)


def upconv_ws_bytes(dtype, n_frames, h, w, c_a, c_b, c_out, pool_cap, stats):
    """Workspace of shpl_upconv3x3; pool_cap: the pooling CSR's entry capacity, or None without a pool."""
    return L.ws_bytes("shpl_upconv3x3", dtype, n_frames, h, w, c_a, c_b, c_out, pool_cap, bool(stats))


def upconv3x3(a, weights, b=None, pool=None, frame_off=None, center=None, scale=None, shift=None, relu=True,
              stats=None, out=None, ws=None):
    """act((conv2d_transpose_SAME_stride2([a || b], weights) - center) * scale + shift) -> [B,2H,2W,Cout].

    a: [B,H,W,Ca] NHWC (f32 or bf16); weights: HWOI [3,3,Cout,Ca+Cb]; b, pool, frame_off: the second source
    exactly as ``fusion_conv.conv3x3`` takes it (dense, pooled through the cell-keyed or the pixel-keyed CSR,
    or absent); stats: optional [2,Cout] float64 tensor receiving per-channel sum / sum of squares of the
    pre-epilogue output over the B*2H*2W rows."""
    return _fused_call(_UPCONV, a, weights, b, pool, frame_off, center, scale, shift, relu, stats, out, ws)


def upconv_grad_ws_bytes(which, dtype, n_frames, h, w, c_a, c_b, c_out, pool_cap=None):
    """Workspace of shpl_upconv3x3_dgrad (which = "dgrad": c_a = c_gy, c_out = c_dx, c_b and pool_cap unused) or
    of shpl_upconv3x3_wgrad (which = "wgrad"; pool_cap: the pooling CSR's entry capacity, or None without a pool).
    h, w: the INPUT map's size."""
    if which == "dgrad":
        return L.ws_bytes("shpl_upconv3x3_dgrad", dtype, n_frames, h, w, c_a, c_out)
    if which == "wgrad":
        return L.ws_bytes("shpl_upconv3x3_wgrad", dtype, n_frames, h, w, c_a, c_b, c_out, pool_cap)
    raise ValueError(f"which = {which!r}: 'dgrad' or 'wgrad'")


def upconv3x3_dgrad(gy, weights, c_dx, split=None, ws=None):
    """Input gradient [B,H,W,c_dx] of ``upconv3x3`` with its HWOI ``weights`` [3,3,Cout,c_dx]: gy is the gradient
    of the raw output, [B,2H,2W,Cout] (its last dimension dense; rows may be a view into a wider buffer). With
    ``split`` = c, the pair (channels [0, c), channels [c, c_dx)) as two dense maps written by the kernel's
    epilogue (shpl_upconv3x3_dgrad)."""
    if gy.stride(-1) != 1 or gy.stride(2) < gy.shape[3] or gy.stride(1) != gy.stride(2) * gy.shape[2] \
            or gy.stride(0) != gy.stride(1) * gy.shape[1]:
        gy = gy.contiguous()
    B, H2, W2, Cg = (int(s) for s in gy.shape)
    if H2 % 2 or W2 % 2:
        raise ValueError(f"the output gradient {tuple(gy.shape)} is not 2H x 2W")
    H, W = H2 // 2, W2 // 2
    weights = weights.to(gy.dtype).contiguous()
    c_dx = int(c_dx)
    if tuple(weights.shape) != (3, 3, Cg, c_dx):
        raise ValueError(f"weights {tuple(weights.shape)} (HWOI) do not match {Cg} -> {c_dx} channels")
    dt = L.dtype_code(gy)
    dx, dx_b, outs = _split_outputs(gy, (B, H, W), c_dx, split)
    if ws is None:
        ws = L.workspace(upconv_grad_ws_bytes("dgrad", dt, B, H, W, Cg, 0, c_dx), gy.device)
    L.check(L.lib().shpl_upconv3x3_dgrad(dt, B, H, W, L.ptr(gy), int(gy.stride(2)), Cg, L.ptr(weights), c_dx, *outs,
                                         L.ptr(ws), ws.numel(), L.stream_of(gy.device)), "shpl_upconv3x3_dgrad")
    return dx if split is None else (dx, dx_b)


def upconv3x3_wgrad(a, gy, b=None, pool=None, frame_off=None, ws=None):
    """Weight gradient (f32 HWOI [3,3,Cout,Ca+Cb]) of ``upconv3x3`` of [a || b]: b dense, pooled through ``pool``
    (recomputed in the staging, never stored) or absent, as ``upconv3x3`` takes it; gy the gradient of the raw
    output, [B,2H,2W,Cout] (shpl_upconv3x3_wgrad)."""
    B, H, W = (int(s) for s in a.shape[:3])
    if tuple(gy.shape[:3]) != (B, 2 * H, 2 * W) or gy.dtype != a.dtype:
        raise ValueError(f"the output gradient {tuple(gy.shape)} {gy.dtype} does not match the input {tuple(a.shape)}")
    return _wgrad_call(_UPCONV, "shpl_upconv3x3_wgrad", a, gy, b, pool, frame_off, ws)


class _FusionUpconvFn(torch.autograd.Function):
    """FusionUpconv forward + the TF-autodiff backward of the same graph, by the module's route (``up.backward``,
    module docstring).
    Inputs: a [B,H,W,Ca]; b: None, or -- with side -- the other map, pooled through smap; the HWOI weights; beta."""

    @staticmethod
    def forward(ctx, a, b, weights, beta, up, smap, side, is_training, out):
        pooled = side is not None
        a = a.contiguous()
        b = None if b is None else b.contiguous()
        pool = smap.csr(*side.fwd) if pooled else None
        frame_off = smap.frame_off if pooled else None
        train_bn = up.batch_norm and is_training
        y, raw, mean, scale = up._forward(a, b, pool, frame_off, is_training, out, keep=True)
        ctx.up, ctx.smap, ctx.side, ctx.train_bn = up, smap, side, train_bn
        ctx.save_for_backward(a, b, weights, None if train_bn else y, raw, mean, scale, beta if train_bn else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        a, b, weights, y, raw, mean, scale, beta = ctx.saved_tensors
        up, smap, side = ctx.up, ctx.smap, ctx.side
        pooled = side is not None
        Ca = int(a.shape[-1])
        Cb = 0 if b is None else int(b.shape[-1])
        g_raw, dbeta = _bn_relu_backward(up, ctx.train_bn, gy.contiguous().to(a.dtype), y, raw, mean, scale, beta)
        pool = smap.csr(*side.fwd) if pooled else None
        frame_off = smap.frame_off if pooled else None
        direct = up.backward == "direct"
        g_ph = None if direct else space_to_depth(g_raw).contiguous()
        B, H, W = (int(s) for s in a.shape[:3])
        dt = L.dtype_code(a)
        d_a = d_b = dw = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            split = None if b is None else Ca
            if direct:
                ws = up._ws_for(("up_dgrad", dt, B, H, W, Cb),
                                upconv_grad_ws_bytes("dgrad", dt, B, H, W, up.c_out, 0, Ca + Cb))
                dx = upconv3x3_dgrad(g_raw, weights, Ca + Cb, split=split, ws=ws)
            else:
                dx = conv3x3_dgrad(g_ph, phase_weights(weights.to(a.dtype)), Ca + Cb, split=split)
            if b is None:
                d_a = dx
            else:
                d_a, dx_b = dx
                if ctx.needs_input_grad[1]:
                    d_b = _pull_back(smap, side, dx_b, b)
            if not ctx.needs_input_grad[0]:
                d_a = None
        if ctx.needs_input_grad[2]:
            if direct:
                cap = None if pool is None else pool.nnz_cap
                ws = up._ws_for(("up_wgrad", dt, B, H, W, Cb, cap),
                                upconv_grad_ws_bytes("wgrad", dt, B, H, W, Ca, Cb, up.c_out, cap))
                dw = upconv3x3_wgrad(a, g_raw, b=b, pool=pool, frame_off=frame_off, ws=ws).to(weights.dtype)
            else:
                dw = phase_weight_grad(conv3x3_wgrad(a, g_ph, b=b, pool=pool, frame_off=frame_off)).to(weights.dtype)
        d_beta, _ = _beta_bias_grads(up, dbeta, ctx.needs_input_grad[3], False)
        return d_a, d_b, dw, d_beta, None, None, None, None, None


class FusionUpconv(FusionConv):
    """slim.conv2d_transpose(x, c_out, [3,3], stride=2) with slim.batch_norm and ReLU: the variables of one
    ``upconv3`` scope and its forward. ``weights`` is slim's HWOI variable [3,3,c_out,c_in] (xavier-uniform);
    beta, the moving statistics and the device-resident inference scale are kept as ``FusionConv`` keeps them.
    The entry points are ``FusionConv``'s, with upconv3 for the conv: ``__call__`` on a materialised fused map or
    on plain conv4 (the image side of a non-dual layer), ``fused`` / ``fused_img`` (``smap`` at conv4's stride)
    without writing the concat, ``fused_csr`` / ``fused_img_csr`` over an already built CSR, forward only."""

    DEFAULT_BACKWARD = "direct"
    BACKWARDS = ("direct", "phases")
    _CALL, _WS_KEY = _UPCONV, ("up",)

    def __init__(self, c_in, c_out, batch_norm=True, relu=True, eps=1e-3, decay=0.999, dtype=torch.float32,
                 device="cuda", seed=0, backward=None):
        """backward: "direct" -- shpl_upconv3x3_dgrad / shpl_upconv3x3_wgrad on the raw output's gradient -- or
        "phases", the stride-1 phase conv's gradients (module docstring); None: DEFAULT_BACKWARD."""
        backward = self.DEFAULT_BACKWARD if backward is None else backward
        if backward not in self.BACKWARDS:
            raise ValueError(f"backward = {backward!r}: one of {self.BACKWARDS}")
        self.backward = backward
        super().__init__(c_in, c_out, batch_norm=batch_norm, bias=False, relu=relu, eps=eps, decay=decay,
                         dtype=dtype, device=device, seed=seed)

    def _apply(self, a, b, smap, side, is_training, out):
        return _FusionUpconvFn.apply(a, b, self.weights, self.beta, self, smap, side, is_training, out)

    def forward_phases(self, a, b=None, pool=None, frame_off=None, is_training=False):
        """The forward by the phase route: ``conv3x3`` with ``phase_weights`` to 4*c_out channels, then
        ``depth_to_space`` -- the same sums in another order (and 4x the MFMA work). b / pool / frame_off as
        ``upconv3x3`` takes them. Training mode normalises with the batch moments but leaves the moving
        statistics alone: this is a cross-check and a timing comparator, not a second forward."""
        w_ph = phase_weights(self.weights)
        B, H, W = (int(s) for s in a.shape[:3])
        if not (self.batch_norm and is_training):
            center, scale, shift = self._inference_epilogue()
            rep = [None if v is None else v.repeat(4) for v in (center, scale, shift)]
            y = conv3x3(a, w_ph, b=b, pool=pool, frame_off=frame_off, center=rep[0], scale=rep[1], shift=rep[2],
                        relu=self.relu)
            return depth_to_space(y).contiguous()
        st4 = torch.empty((2, 4 * self.c_out), dtype=torch.float64, device=a.device)
        raw = depth_to_space(conv3x3(a, w_ph, b=b, pool=pool, frame_off=frame_off, relu=False, stats=st4))
        raw = raw.contiguous()
        stats = st4.reshape(2, 4, self.c_out).sum(1).contiguous()
        return batch_norm_train(raw, stats, B * 4 * H * W, eps=self.eps, beta=self.beta, relu=self.relu,
                                moving_mean=self.moving_mean.clone(), moving_var=self.moving_var.clone(),
                                decay=self.decay)


class AfterVggFusion(_TwoScopes):
    """Both ``upconv3`` scopes that follow the SHPL under rpn_sparse_pooling_after_vgg
    (fusion_vgg_pyramid.py:53-60, :198-206, one feature extractor per side): the BEV one over
    [conv4_bev || pool(conv4_img)], the image one over [conv4_img || trans(conv4_bev)] for a dual layer
    (rpn_dual_sparse_pooling_after_vgg) and over conv4_img itself otherwise (bv_index=None). ``dual`` fixes the
    image scope's input channels, as it fixes the graph in the reference."""

    def __init__(self, c_bev=256, c_img=256, c_out=128, dual=True, dtype=torch.float32, device="cuda", seed=0, **kw):
        super().__init__(c_bev, c_img, dual,
                         FusionUpconv(c_bev + c_img, c_out, dtype=dtype, device=device, seed=seed, **kw),
                         FusionUpconv(c_img + (c_bev if dual else 0), c_out, dtype=dtype, device=device,
                                      seed=seed + 1, **kw))

    def __call__(self, conv4_bev, conv4_img, smap, is_training=False):
        """(upconv3_bev, upconv3_img): the BEV scope on the current stream, the image scope on the module's side
        stream, which the current stream then waits for (as ``PostFusion`` issues its two convs)."""
        return super().__call__(conv4_bev, conv4_img, smap, is_training)
