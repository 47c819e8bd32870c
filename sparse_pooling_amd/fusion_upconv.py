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

import ctypes

import numpy as np
import torch

from . import _lib as L
from . import shpl_map as sm
from .fusion_conv import (SIDE_BEV, SIDE_IMG, FusionConv, batch_norm_backward, batch_norm_train, conv3x3,
                          conv3x3_dgrad, conv3x3_wgrad)

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
    out = ctypes.c_size_t()
    L.check(L.lib().shpl_upconv3x3_workspace_bytes(dtype, int(n_frames), int(h), int(w), int(c_a), int(c_b),
                                                   int(c_out), -1 if pool_cap is None else int(pool_cap),
                                                   int(bool(stats)), ctypes.byref(out)),
            "shpl_upconv3x3_workspace_bytes")
    return out.value


def upconv3x3(a, weights, b=None, pool=None, frame_off=None, center=None, scale=None, shift=None, relu=True,
              stats=None, out=None, ws=None):
    """act((conv2d_transpose_SAME_stride2([a || b], weights) - center) * scale + shift) -> [B,2H,2W,Cout].

    a: [B,H,W,Ca] NHWC (f32 or bf16); weights: HWOI [3,3,Cout,Ca+Cb]; b, pool, frame_off: the second source
    exactly as ``fusion_conv.conv3x3`` takes it (dense, pooled through the cell-keyed or the pixel-keyed CSR,
    or absent); stats: optional [2,Cout] float64 tensor receiving per-channel sum / sum of squares of the
    pre-epilogue output over the B*2H*2W rows."""
    dt = L.dtype_code(a)
    a = a if a.is_contiguous() else a.contiguous()
    B, H, W, Ca = (int(s) for s in a.shape)
    Cb = 0
    if b is not None:
        b = b if b.is_contiguous() else b.contiguous()
        if b.dtype != a.dtype:
            raise TypeError("both inputs of the transposed conv must share one dtype")
        Cb = int(b.shape[-1])
        if pool is None and tuple(b.shape[:3]) != (B, H, W):
            raise ValueError(f"dense second input {tuple(b.shape)} does not match {tuple(a.shape)}")
    if weights.dtype != a.dtype:
        weights = weights.to(a.dtype)
    weights = weights.contiguous()
    Cout = int(weights.shape[2])
    if tuple(weights.shape[:2]) != (3, 3) or int(weights.shape[3]) != Ca + Cb:
        raise ValueError(f"weights {tuple(weights.shape)} (HWOI) do not match {Ca}+{Cb} input channels")
    if out is None:
        out = torch.empty((B, 2 * H, 2 * W, Cout), dtype=a.dtype, device=a.device)
    if ws is None:
        ws = L.workspace(upconv_ws_bytes(dt, B, H, W, Ca, Cb, Cout, None if pool is None else pool.nnz_cap,
                                         stats is not None), a.device)
    f32 = [None if v is None else v.to(device=a.device, dtype=torch.float32).contiguous()
           for v in (center, scale, shift)]
    L.check(L.lib().shpl_upconv3x3(dt, B, H, W, L.ptr(a), Ca, 0, Ca, L.ptr(b), Cb, 0, Cb,
                                   None if pool is None else pool.ref(), L.ptr(frame_off), L.ptr(weights), Cout,
                                   *[L.ptr(v) for v in f32], L.ACT_RELU if relu else L.ACT_NONE, L.ptr(out),
                                   int(out.stride(2)), L.ptr(stats), L.ptr(ws), ws.numel(),
                                   L.stream_of(a.device)), "shpl_upconv3x3")
    return out


def upconv_grad_ws_bytes(which, dtype, n_frames, h, w, c_a, c_b, c_out, pool_cap=None):
    """Workspace of shpl_upconv3x3_dgrad (which = "dgrad": c_a = c_gy, c_out = c_dx, c_b and pool_cap unused) or
    of shpl_upconv3x3_wgrad (which = "wgrad"; pool_cap: the pooling CSR's entry capacity, or None without a pool).
    h, w: the INPUT map's size."""
    out = ctypes.c_size_t()
    if which == "dgrad":
        L.check(L.lib().shpl_upconv3x3_dgrad_workspace_bytes(dtype, int(n_frames), int(h), int(w), int(c_a),
                                                             int(c_out), ctypes.byref(out)),
                "shpl_upconv3x3_dgrad_workspace_bytes")
    elif which == "wgrad":
        L.check(L.lib().shpl_upconv3x3_wgrad_workspace_bytes(dtype, int(n_frames), int(h), int(w), int(c_a),
                                                             int(c_b), int(c_out),
                                                             -1 if pool_cap is None else int(pool_cap),
                                                             ctypes.byref(out)),
                "shpl_upconv3x3_wgrad_workspace_bytes")
    else:
        raise ValueError(f"which = {which!r}: 'dgrad' or 'wgrad'")
    return out.value


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
    c0 = c_dx if split is None else int(split)
    dx = torch.empty((B, H, W, c0), dtype=gy.dtype, device=gy.device)
    dx_b = None if split is None else torch.empty((B, H, W, c_dx - c0), dtype=gy.dtype, device=gy.device)
    if ws is None:
        ws = L.workspace(upconv_grad_ws_bytes("dgrad", dt, B, H, W, Cg, 0, c_dx), gy.device)
    L.check(L.lib().shpl_upconv3x3_dgrad(dt, B, H, W, L.ptr(gy), int(gy.stride(2)), Cg, L.ptr(weights), c_dx,
                                         L.ptr(dx), max(c0, 1), c0, L.ptr(dx_b), max(c_dx - c0, 1), L.ptr(ws),
                                         ws.numel(), L.stream_of(gy.device)), "shpl_upconv3x3_dgrad")
    return dx if split is None else (dx, dx_b)


def upconv3x3_wgrad(a, gy, b=None, pool=None, frame_off=None, ws=None):
    """Weight gradient (f32 HWOI [3,3,Cout,Ca+Cb]) of ``upconv3x3`` of [a || b]: b dense, pooled through ``pool``
    (recomputed in the staging, never stored) or absent, as ``upconv3x3`` takes it; gy the gradient of the raw
    output, [B,2H,2W,Cout] (shpl_upconv3x3_wgrad)."""
    a = a.contiguous()
    gy = gy.contiguous()
    dt = L.dtype_code(a)
    B, H, W, Ca = (int(s) for s in a.shape)
    Cb = 0 if b is None else int(b.shape[-1])
    if b is not None:
        b = b.contiguous()
    Cout = int(gy.shape[-1])
    if tuple(gy.shape[:3]) != (B, 2 * H, 2 * W) or gy.dtype != a.dtype:
        raise ValueError(f"the output gradient {tuple(gy.shape)} {gy.dtype} does not match the input {tuple(a.shape)}")
    dw = torch.empty((3, 3, Cout, Ca + Cb), dtype=torch.float32, device=a.device)
    if ws is None:
        ws = L.workspace(upconv_grad_ws_bytes("wgrad", dt, B, H, W, Ca, Cb, Cout,
                                              None if pool is None else pool.nnz_cap), a.device)
    L.check(L.lib().shpl_upconv3x3_wgrad(dt, B, H, W, L.ptr(a), Ca, 0, Ca, L.ptr(b), Cb, 0, Cb,
                                         None if pool is None else pool.ref(), L.ptr(frame_off), L.ptr(gy), Cout,
                                         Cout, L.ptr(dw), L.ptr(ws), ws.numel(), L.stream_of(a.device)),
            "shpl_upconv3x3_wgrad")
    return dw


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
        gy = gy.contiguous().to(a.dtype)
        if up.batch_norm or up.relu:
            g_raw, dbeta, _ = batch_norm_backward(gy, y=y, raw=raw, mean=mean if up.batch_norm else None,
                                                  scale=scale if up.batch_norm else None, relu=up.relu,
                                                  training=ctx.train_bn, beta=beta)
        else:
            g_raw, dbeta = gy, None
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
                    # the pooled channels' gradient back to the pooled source (_Side.grad), as FusionConv's
                    d_b = torch.empty(b.shape, dtype=dx_b.dtype, device=dx_b.device)
                    sm.pull(smap, *side.grad, dx_b, Cb, 0, Cb, d_b, Cb)
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
        d_beta = dbeta if (up.batch_norm and ctx.needs_input_grad[3]) else None
        return d_a, d_b, dw, d_beta, None, None, None, None, None


class FusionUpconv(FusionConv):
    """slim.conv2d_transpose(x, c_out, [3,3], stride=2) with slim.batch_norm and ReLU: the variables of one
    ``upconv3`` scope and its forward. ``weights`` is slim's HWOI variable [3,3,c_out,c_in] (xavier-uniform);
    beta, the moving statistics and the device-resident inference scale are kept as ``FusionConv`` keeps them."""

    DEFAULT_BACKWARD = "direct"
    BACKWARDS = ("direct", "phases")

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
        g = np.random.default_rng(seed)
        # xavier_initializer (uniform) over the variable's shape [3,3,c_out,c_in]: fans 9*c_out and 9*c_in
        lim = float(np.sqrt(6.0 / (9 * c_in + 9 * c_out)))
        w = g.uniform(-lim, lim, size=(3, 3, c_out, c_in)).astype(np.float32)
        self.weights = torch.from_numpy(w).to(self.device, dtype)

    def _forward(self, a, b, pool, frame_off, is_training, out, keep=False):
        """The forward; keep: also what the backward needs -- (y, raw, mean, scale)."""
        B, H, W, Ca = (int(s) for s in a.shape)
        Cb = 0 if b is None else int(b.shape[-1])
        dt = L.dtype_code(a)
        train_bn = self.batch_norm and is_training
        cap = None if pool is None else pool.nnz_cap
        ws = self._ws_for(("up", dt, B, H, W, Cb, cap, train_bn),
                          upconv_ws_bytes(dt, B, H, W, Ca, Cb, self.c_out, cap, train_bn))
        if not train_bn:
            center, scale, shift = self._inference_epilogue()
            if keep and scale is not None:  # saved for the backward: a copy, not the buffer a training step rewrites
                scale = scale.clone()
            y = upconv3x3(a, self.weights, b=b, pool=pool, frame_off=frame_off, center=center, scale=scale,
                          shift=shift, relu=self.relu, out=out, ws=ws)
            return (y, None, center, scale) if keep else y
        stats = torch.empty((2, self.c_out), dtype=torch.float64, device=a.device)
        raw = upconv3x3(a, self.weights, b=b, pool=pool, frame_off=frame_off, relu=False, stats=stats,
                        out=None if keep else out, ws=ws)
        bn_ws = torch.empty(2 * self.c_out, dtype=torch.float32, device=a.device)
        y = (out if out is not None else torch.empty_like(raw)) if keep else None
        y = batch_norm_train(raw, stats, B * 4 * H * W, eps=self.eps, beta=self.beta, relu=self.relu,
                             moving_mean=self.moving_mean, moving_var=self.moving_var, decay=self.decay, out=y,
                             ws=bn_ws)
        self._refresh_scale()  # batch_norm_train updated the moving statistics through their device pointers
        return (y, raw, bn_ws[:self.c_out], bn_ws[self.c_out:]) if keep else y

    def _run(self, a, b, pool, frame_off, is_training, out):
        return self._forward(a, b, pool, frame_off, is_training, out)

    def _apply(self, a, b, smap, side, is_training, out):
        return _FusionUpconvFn.apply(a, b, self.weights, self.beta, self, smap, side, is_training, out)

    def __call__(self, x, is_training=False, out=None):
        """upconv3 of a materialised fused map, or of plain conv4 (the image side of a non-dual layer)."""
        if self._grad_wanted(x):
            return self._apply(x, None, None, None, is_training, out)
        return self._run(x, None, None, None, is_training, out)

    def fused(self, bev, img, smap, is_training=False, out=None):
        """upconv3 of [bev || _sparse_pool_op(M, img)] without writing the concat: ``smap`` is the ShplMap of the
        frames of ``bev`` (at conv4's stride). Differentiable in bev, img, the weights and beta."""
        if self._grad_wanted(bev, img):
            return self._apply(bev, img, smap, SIDE_BEV, is_training, out)
        return self.fused_csr(bev, img, smap.csr(*SIDE_BEV.fwd), smap.frame_off, is_training, out)

    def fused_img(self, img, bev, smap, is_training=False, out=None):
        """upconv3 of [img || _sparse_pool_trans_op(M, bev)] (the dual layer's image side) without writing the
        concat. Differentiable in img, bev, the weights and beta."""
        if int(bev.numel()) // max(int(bev.shape[-1]), 1) != smap.n_cells:
            raise ValueError(f"BEV map {tuple(bev.shape)} has {int(bev.numel()) // max(int(bev.shape[-1]), 1)} rows, "
                             f"the map {smap.n_cells} cells")
        if self._grad_wanted(img, bev):
            return self._apply(img, bev, smap, SIDE_IMG, is_training, out)
        return self.fused_img_csr(img, bev, smap.csr(*SIDE_IMG.fwd), smap.frame_off, is_training, out)

    # fused_csr / fused_img_csr: FusionConv's (forward only, over an already built CSR), through _run above

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


class AfterVggFusion:
    """Both ``upconv3`` scopes that follow the SHPL under rpn_sparse_pooling_after_vgg
    (fusion_vgg_pyramid.py:53-60, :198-206, one feature extractor per side): the BEV one over
    [conv4_bev || pool(conv4_img)], the image one over [conv4_img || trans(conv4_bev)] for a dual layer
    (rpn_dual_sparse_pooling_after_vgg) and over conv4_img itself otherwise (bv_index=None). ``dual`` fixes the
    image scope's input channels, as it fixes the graph in the reference."""

    def __init__(self, c_bev=256, c_img=256, c_out=128, dual=True, dtype=torch.float32, device="cuda", seed=0, **kw):
        self.c_bev, self.c_img, self.dual = int(c_bev), int(c_img), bool(dual)
        self.bev = FusionUpconv(c_bev + c_img, c_out, dtype=dtype, device=device, seed=seed, **kw)
        self.img = FusionUpconv(c_img + (c_bev if dual else 0), c_out, dtype=dtype, device=device, seed=seed + 1,
                                **kw)
        self._side = None

    def __call__(self, conv4_bev, conv4_img, smap, is_training=False):
        """(upconv3_bev, upconv3_img): the BEV scope on the current stream, the image scope on the module's side
        stream, which the current stream then waits for (as ``PostFusion`` issues its two convs)."""
        cur = torch.cuda.current_stream(conv4_bev.device)
        if self._side is None:
            self._side = torch.cuda.Stream(device=conv4_bev.device)
        side = self._side
        if self.dual:  # both CSRs on the current stream, before the fork: the map builds each once, stream-ordered
            smap.csr(*SIDE_IMG.fwd)
        smap.csr(*SIDE_BEV.fwd)
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            if self.dual:
                img_out = self.img.fused_img(conv4_img, conv4_bev, smap, is_training)
            else:
                img_out = self.img(conv4_img, is_training)
        bev_out = self.bev.fused(conv4_bev, conv4_img, smap, is_training)
        for t in (conv4_bev, conv4_img, self.img.weights):
            t.record_stream(side)
        cur.wait_stream(side)
        img_out.record_stream(cur)
        return bev_out, img_out
