"""Post-fusion 3x3 convolution over the libshpl C ABI.

The reference follows the SHPL with a 3x3 conv on each fused map when
``rpn_sparse_pooling_conv_after_fusion`` is set (default true,
avod/avod/protos/model.proto:88):

    bev = slim.conv2d(bv_fused, feature_depths[0], [3, 3],
                      normalizer_fn=slim.batch_norm,
                      normalizer_params={'is_training': is_training},
                      scope='pyramid_fusion_pooled_bev')        # rpn_model.py:338-346
    img = slim.conv2d(img_fused, feature_depths[1], [3, 3], ...,
                      scope='pyramid_fusion_pooled_img')        # rpn_model.py:347-354

(RetinaNet: ``slim.conv2d(bev_fused, 256, [3, 3])`` with a bias and no BN,
retinanet_model.py:343-348). slim defaults: SAME padding, stride 1, ReLU,
no bias under a normalizer; slim.batch_norm: center (beta), no scale,
epsilon 1e-3, decay 0.999, fused kernel (batch moments when training, moving
averages with the Bessel-corrected variance).

``FusionConv.fused(bev, img, smap)`` computes the BEV conv of
[bev || pool(img)] straight from the img->BEV CSR (shpl_conv3x3 with a
pool CSR): bv_fused never reaches HBM, and the result is bitwise the conv of
the materialised map. The backward (TF autodiff of the same graph) runs on
the device too: BatchNorm/ReLU backward, the input gradient (the same conv
kernel on transposed weights) and the weight gradient (an MFMA reduction over
pixels that recomputes the pooled channels from the CSR), then the SHPL pull
that carries the pooled channels' gradient back to the image map.

``FusionConv.fused_img(img, bev, smap)`` is the image side's conv of
[img || _sparse_pool_trans_op(M, bev)] (the dual path of sparse_pool_layer,
sparse_pool_utils.py:79-87) the same way, from the BEV->img (pixel-keyed) CSR:
the same kernels with the sides swapped, the pooled sums taken per column of M
first (TF's ScatterNd order, as shpl_pull SHPL_BY_PIXEL), and the pooled
channels' gradient pulled back to the BEV map. ``PostFusion`` holds both
scopes of rpn_model.py:338-354 and issues the two convs side by side.
"""
from __future__ import annotations

import collections
import ctypes

import numpy as np
import torch

from . import _lib as L
from . import shpl_map as sm


# The directions of a fused conv: the CSR (direction, order) its forward pools through, the pull that carries the
# pooled channels' gradient back to the pooled source (the TF gradient of the forward's op), and the pull that
# materialises the pooled channels (f32 weight gradient).
_Side = collections.namedtuple("_Side", "fwd grad pool")
# pyramid_fusion_pooled_bev: [bev || _sparse_pool_op(M, img)]; the gradient returns to the image (a8's TF gradient)
SIDE_BEV = _Side((L.BY_CELL, L.ORDER_ENTRY), (L.BY_PIXEL, L.ORDER_COL_ENTRY), sm.pool_img_to_bev)
# pyramid_fusion_pooled_img: [img || _sparse_pool_trans_op(M, bev)]; the gradient returns to the BEV map (the pull
# of _DualFn.backward)
SIDE_IMG = _Side((L.BY_PIXEL, L.ORDER_COL_ROW), (L.BY_CELL, L.ORDER_COL_ENTRY), sm.pool_bev_to_img)


def conv_ws_bytes(dtype, n_frames, h, w, c_a, c_b, c_out, pool_cap, stats):
    """Workspace of shpl_conv3x3; pool_cap: the pooling CSR's entry capacity
    (``Csr.nnz_cap``), or None without a pool."""
    return L.ws_bytes("shpl_conv3x3", dtype, n_frames, h, w, c_a, c_b, c_out, pool_cap, bool(stats))


def _form(symbol, a, weights, b, pool, frame_off, relu, stats, out, c_out):
    """The answer of a dispatch query of conv3x3 (shpl_conv3x3_rows_form, shpl_conv3x3_wide_form)."""
    B, H, W, Ca = (int(s) for s in a.shape)
    Cb = 0 if b is None else int(b.shape[-1])
    Cout = int(weights.shape[3]) if c_out is None else int(c_out)
    flag = ctypes.c_int(0)
    out_ptr = L.ptr(out) if out is not None else ctypes.c_void_p(256)  # a stand-in aligned address
    L.check(getattr(L.lib(), symbol)(L.dtype_code(a), B, H, W, L.ptr(a), Ca, 0, Ca, L.ptr(b), Cb, 0, Cb,
                                     None if pool is None else pool.ref(), L.ptr(frame_off), L.ptr(weights),
                                     Cout, L.ACT_RELU if relu else L.ACT_NONE, out_ptr,
                                     Cout if out is None else int(out.stride(2)), int(bool(stats)),
                                     ctypes.byref(flag)), symbol)
    return flag.value


def rows_form(a, weights, b=None, pool=None, frame_off=None, relu=True, stats=False, out=None, c_out=None):
    """Whether conv3x3 with these arguments runs the row-streaming form (shpl_conv3x3_rows_form): only then
    does its workspace hold the pooled operand shpl_conv3x3_wgrad_reuse reads. ``out`` None: a fresh
    contiguous output (16-byte aligned, as torch allocates)."""
    return bool(_form("shpl_conv3x3_rows_form", a, weights, b, pool, frame_off, relu, stats, out, c_out))


def wide_form(a, weights, b=None, pool=None, frame_off=None, relu=True, stats=False, out=None, c_out=None):
    """Which form of the wide bf16 kernel conv3x3 with these arguments runs (shpl_conv3x3_wide_form): 0 none,
    1 with b dense or absent, 2 over the compact pooled runs, 3 over the materialised pooled map."""
    return _form("shpl_conv3x3_wide_form", a, weights, b, pool, frame_off, relu, stats, out, c_out)


# A forward of the library over [a || b]: its symbol (the workspace query is <symbol>_workspace_bytes), the output's
# size per input pixel and axis, the weight axes that hold c_in and c_out, and the wording of its errors.
_Call = collections.namedtuple("_Call", "symbol up w_in w_out noun layout")
_CONV = _Call("shpl_conv3x3", 1, 2, 3, "conv", "")  # HWIO weights


def _fused_call(call, a, weights, b, pool, frame_off, center, scale, shift, relu, stats, out, ws):
    """conv3x3 (_CONV) or fusion_upconv.upconv3x3 (its _UPCONV): the checks, the output, the workspace, the call."""
    dt = L.dtype_code(a)
    a = a if a.is_contiguous() else a.contiguous()
    B, H, W, Ca = (int(s) for s in a.shape)
    Cb = 0
    if b is not None:
        b = b if b.is_contiguous() else b.contiguous()
        if b.dtype != a.dtype:
            raise TypeError(f"both inputs of the {call.noun} must share one dtype")
        Cb = int(b.shape[-1])
        if pool is None and tuple(b.shape[:3]) != (B, H, W):
            raise ValueError(f"dense second input {tuple(b.shape)} does not match {tuple(a.shape)}")
    if weights.dtype != a.dtype:
        weights = weights.to(a.dtype)
    weights = weights.contiguous()
    Cout = int(weights.shape[call.w_out])
    if tuple(weights.shape[:2]) != (3, 3) or int(weights.shape[call.w_in]) != Ca + Cb:
        raise ValueError(f"weights {tuple(weights.shape)}{call.layout} do not match {Ca}+{Cb} input channels")
    if out is None:
        out = torch.empty((B, call.up * H, call.up * W, Cout), dtype=a.dtype, device=a.device)
    if ws is None:
        ws = L.workspace(L.ws_bytes(call.symbol, dt, B, H, W, Ca, Cb, Cout, None if pool is None else pool.nnz_cap,
                                    stats is not None), a.device)
    f32 = [None if v is None else v.to(device=a.device, dtype=torch.float32).contiguous()
           for v in (center, scale, shift)]
    L.check(getattr(L.lib(), call.symbol)(dt, B, H, W, L.ptr(a), Ca, 0, Ca, L.ptr(b), Cb, 0, Cb,
                                          None if pool is None else pool.ref(), L.ptr(frame_off), L.ptr(weights),
                                          Cout, *[L.ptr(v) for v in f32], L.ACT_RELU if relu else L.ACT_NONE,
                                          L.ptr(out), int(out.stride(2)), L.ptr(stats), L.ptr(ws), ws.numel(),
                                          L.stream_of(a.device)), call.symbol)
    return out


def conv3x3(a, weights, b=None, pool=None, frame_off=None, center=None, scale=None, shift=None, relu=True,
            stats=None, out=None, ws=None):
    """act((conv3x3_SAME([a || b], weights) - center) * scale + shift).

    a: [B,H,W,Ca] NHWC (f32 or bf16); weights: HWIO [3,3,Ca+Cb,Cout] of the
    same dtype; b: a second dense map [B,H,W,Cb], or -- with ``pool`` (the
    cell-keyed ``_lib.Csr`` of an img->BEV map) and ``frame_off`` -- the image
    map [Bi,Hi,Wi,Cb] that is pooled on the fly (a the BEV map); with the
    pixel-keyed CSR (BY_PIXEL, ORDER_COL_ROW) a is the image map and b the BEV
    map [Bb,Hb,Wb,Cb] pooled to the image; stats: optional [2,Cout]
    float64 tensor receiving per-channel sum / sum of squares of the
    pre-epilogue output."""
    return _fused_call(_CONV, a, weights, b, pool, frame_off, center, scale, shift, relu, stats, out, ws)


def batch_norm_train(x, stats, count, eps=1e-3, gamma=None, beta=None, relu=True, moving_mean=None,
                     moving_var=None, decay=0.999, batch_mean=None, batch_var=None, out=None, ws=None):
    """FusedBatchNorm (is_training) of x [..., C] from conv3x3's stats into
    ``out`` (None: in place). ``ws`` (2*C floats) receives the batch mean and
    scale the backward needs."""
    C = int(x.shape[-1])
    rows = x.numel() // C
    if ws is None:
        ws = torch.empty(2 * C, dtype=torch.float32, device=x.device)
    L.check(L.lib().shpl_batch_norm(L.dtype_code(x), rows, L.ptr(x), L.ptr(out), C, C, L.ptr(stats), float(count),
                                    float(eps), L.ptr(gamma), L.ptr(beta), L.ACT_RELU if relu else L.ACT_NONE,
                                    L.ptr(moving_mean), L.ptr(moving_var), float(decay), L.ptr(batch_mean),
                                    L.ptr(batch_var), L.ptr(ws), L.stream_of(x.device)), "shpl_batch_norm")
    return x if out is None else out


def batch_norm_backward(gy, y=None, raw=None, mean=None, scale=None, gamma=None, relu=True, training=True,
                        beta=None):
    """(g_raw, dbeta, dgamma) of BatchNorm (+ ReLU) over [..., C]; mean / scale
    None -> 0 / 1 (a conv bias: dbeta is the bias gradient). With y None the
    ReLU mask is recomputed from raw (and beta), bitwise the forward's."""
    C = int(gy.shape[-1])
    rows = gy.numel() // C
    out = torch.empty_like(gy)
    dbeta = torch.empty(C, dtype=torch.float32, device=gy.device)
    dgamma = torch.empty(C, dtype=torch.float32, device=gy.device)
    ws = L.workspace(L.ws_bytes("shpl_batch_norm_backward", rows, C), gy.device)
    L.check(L.lib().shpl_batch_norm_backward(L.dtype_code(gy), rows, L.ptr(y), L.ptr(raw), L.ptr(gy), C, C,
                                             L.ptr(mean), L.ptr(scale), L.ptr(gamma), L.ptr(beta),
                                             L.ACT_RELU if relu else L.ACT_NONE, int(bool(training)), L.ptr(out),
                                             L.ptr(dbeta), L.ptr(dgamma), L.ptr(ws), ws.numel(),
                                             L.stream_of(gy.device)), "shpl_batch_norm_backward")
    return out, dbeta, dgamma


def _split_outputs(gy, shape, c_dx, split):
    """An input gradient's outputs over the [B,H,W] ``shape``, of gy's type: (dx, dx_b, their arguments in the C
    ABI: dx, its row stride, the split channel, dx_b, its row stride). split None: dx is whole and dx_b None."""
    c0 = c_dx if split is None else int(split)
    dx = torch.empty(shape + (c0,), dtype=gy.dtype, device=gy.device)
    dx_b = None if split is None else torch.empty(shape + (c_dx - c0,), dtype=gy.dtype, device=gy.device)
    return dx, dx_b, (L.ptr(dx), max(c0, 1), c0, L.ptr(dx_b), max(c_dx - c0, 1))


def _wgrad_call(call, symbol, a, gy, b, pool, frame_off, ws, *tail):
    """The f32 weight gradient, in ``call``'s weight layout, of ``call`` over [a || b] by the library's ``symbol``
    (the arguments after the workspace: ``tail``); ws None: a fresh workspace."""
    a = a.contiguous()
    gy = gy.contiguous()
    dt = L.dtype_code(a)
    B, H, W, Ca = (int(s) for s in a.shape)
    Cb = 0 if b is None else int(b.shape[-1])
    if b is not None:
        b = b.contiguous()
    Cout = int(gy.shape[-1])
    shape = [3, 3, 0, 0]
    shape[call.w_in], shape[call.w_out] = Ca + Cb, Cout
    dw = torch.empty(shape, dtype=torch.float32, device=a.device)
    if ws is None:
        ws = L.workspace(L.ws_bytes(call.symbol + "_wgrad", dt, B, H, W, Ca, Cb, Cout,
                                    None if pool is None else pool.nnz_cap), a.device)
    L.check(getattr(L.lib(), symbol)(dt, B, H, W, L.ptr(a), Ca, 0, Ca, L.ptr(b), Cb, 0, Cb,
                                     None if pool is None else pool.ref(), L.ptr(frame_off), L.ptr(gy), Cout, Cout,
                                     L.ptr(dw), L.ptr(ws), ws.numel(), *tail, L.stream_of(a.device)), symbol)
    return dw


def conv3x3_dgrad(gy, weights, c_dx, split=None, pool=None, fwd_ws=None, fwd_stats=False):
    """Input gradient [B,H,W,c_dx] of the SAME 3x3 conv with HWIO ``weights``;
    with ``split`` = c, the pair (channels [0, c), channels [c, c_dx)) as two
    dense maps written by the kernel's epilogue (no slicing copies). ``fwd_ws`` (with ``pool``, the pooled bf16
    forward's CSR, and ``split``): the workspace of that forward conv3x3 (taken with statistics: fwd_stats),
    whose occupancy words limit the second map to the occupied cells (pixels, for a pixel-keyed pool) -- the
    only rows the pull back to the pooled source reads; its other rows are left unwritten
    (shpl_conv3x3_dgrad_reuse)."""
    gy = gy.contiguous()
    B, H, W, Cg = (int(s) for s in gy.shape)
    weights = weights.to(gy.dtype).contiguous()
    c_dx = int(c_dx)
    dx, dx_b, outs = _split_outputs(gy, (B, H, W), c_dx, split)
    ws = L.workspace(conv_ws_bytes(L.dtype_code(gy), B, H, W, Cg, 0, c_dx, None, False), gy.device)
    args = (L.dtype_code(gy), B, H, W, L.ptr(gy), Cg, Cg, L.ptr(weights), c_dx, *outs, L.ptr(ws), ws.numel())
    if fwd_ws is not None:
        L.check(L.lib().shpl_conv3x3_dgrad_reuse(*args, pool.ref(), L.ptr(fwd_ws), fwd_ws.numel(),
                                                 int(bool(fwd_stats)), L.stream_of(gy.device)),
                "shpl_conv3x3_dgrad_reuse")
    else:
        L.check(L.lib().shpl_conv3x3_dgrad(*args, L.stream_of(gy.device)), "shpl_conv3x3_dgrad")
    return dx if split is None else (dx, dx_b)


def conv3x3_wgrad(a, gy, b=None, pool=None, frame_off=None, fwd_ws=None, fwd_stats=False):
    """Weight gradient (f32 HWIO [3,3,Ca+Cb,Cout]) of the SAME 3x3 conv of
    [a || b] (b dense, or the image map pooled through ``pool``). fwd_ws (pooled bf16): the workspace of
    the forward conv3x3 over the same inputs (taken with statistics: fwd_stats), whose pooled operand is
    read instead of prepared again (shpl_conv3x3_wgrad_reuse)."""
    if fwd_ws is not None:
        return _wgrad_call(_CONV, "shpl_conv3x3_wgrad_reuse", a, gy, b, pool, frame_off, None, L.ptr(fwd_ws),
                          fwd_ws.numel(), int(bool(fwd_stats)))
    return _wgrad_call(_CONV, "shpl_conv3x3_wgrad", a, gy, b, pool, frame_off, None)


# ------------------------------------------------------------------ what the modules' backwards share
def _bn_relu_backward(mod, train_bn, gy, y, raw, mean, scale, beta):
    """The backward's prologue: (g_raw, dbeta) of the module's BatchNorm (batch or frozen moments) or bias, and
    ReLU; gy itself where the module has none of them."""
    if not (mod.batch_norm or mod.bias is not None or mod.relu):
        return gy, None
    g_raw, dbeta, _ = batch_norm_backward(gy, y=y, raw=raw, mean=mean if mod.batch_norm else None,
                                          scale=scale if mod.batch_norm else None, relu=mod.relu, training=train_bn,
                                          beta=beta)
    return g_raw, dbeta


def _pull_back(smap, side, dx_b, b):
    """The pooled channels' gradient dx_b back to the pooled source b's map (_Side.grad): a fresh d_b."""
    Cb = int(b.shape[-1])
    d_b = torch.empty(b.shape, dtype=dx_b.dtype, device=dx_b.device)
    return sm.pull(smap, *side.grad, dx_b, Cb, 0, Cb, d_b, Cb)


def _beta_bias_grads(mod, dbeta, need_beta, need_bias):
    """(d_beta, d_bias): the prologue's dbeta is BatchNorm's beta gradient, or the conv bias's without one."""
    return (dbeta if (mod.batch_norm and need_beta) else None,
            dbeta if (not mod.batch_norm and need_bias) else None)


class _FusionConvFn(torch.autograd.Function):
    """FusionConv forward + its TF-autodiff backward, all on the device.
    Inputs: a [B,H,W,Ca]; b: a dense [B,H,W,Cb], or None, or -- with side (SIDE_BEV: a the BEV map, SIDE_IMG:
    a the image map) -- the other map, pooled through smap; the conv weights; beta / bias."""

    @staticmethod
    def forward(ctx, a, b, weights, beta, bias, conv, smap, side, is_training, out):
        pooled = side is not None
        a = a.contiguous()
        b = None if b is None else b.contiguous()
        B, H, W, Ca = (int(s) for s in a.shape)
        Cb = 0 if b is None else int(b.shape[-1])
        pool = smap.csr(*side.fwd) if pooled else None
        frame_off = smap.frame_off if pooled else None
        train_bn = conv.batch_norm and is_training
        want_dw = ctx.needs_input_grad[2]
        if pooled and ctx.needs_input_grad[1]:  # the pooled source's gradient's CSR sorts beside the forward
            smap.prefetch_csr(*side.grad)
        src, xb, ws = (b, pool, frame_off), None, None
        if pooled and train_bn and want_dw and a.dtype != torch.bfloat16:
            # f32: the weight gradient needs the pooled channels in HBM (see _wgrad): pooled here, once, the
            # forward is the dense two-source conv (bf16 pools inside both convs: k_conv_rows / k_wgrad_rows)
            xb = side.pool(smap, b, (B, H, W, Cb))
            src = (xb, None, None)
        elif (pooled and conv.WGRAD_REUSE and a.dtype == torch.bfloat16 and want_dw and
              rows_form(a, weights.to(a.dtype), b=b, pool=pool, frame_off=frame_off,
                        relu=conv.relu if not train_bn else False, stats=train_bn,
                        out=out if not train_bn else None, c_out=conv.c_out)):
            # bf16 pooled with a weight gradient to come: a workspace of this call's own, kept for the backward,
            # whose weight gradient reads the pooled operand the forward prepared in it (shpl_conv3x3_wgrad_reuse)
            # -- only when the forward runs the row-streaming form, which is what leaves that operand there
            ws = L.workspace(conv_ws_bytes(L.dtype_code(a), B, H, W, Ca, Cb, conv.c_out, pool.nnz_cap, train_bn),
                             a.device)
        y, raw, mean, scale = conv._forward(a, *src, is_training, out, keep=True, ws=ws)
        ctx.conv, ctx.smap, ctx.pooled, ctx.side, ctx.train_bn = conv, smap, pooled, side, train_bn
        ctx.shapes, ctx.xb, ctx.fwd_ws = (Ca, Cb), xb, ws
        # training BN: the backward recomputes the ReLU mask from raw and beta (bitwise y's), so y is not kept
        ctx.save_for_backward(a, b, weights, None if train_bn else y, raw, mean, scale,
                              beta if train_bn else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        a, b, weights, y, raw, mean, scale, beta = ctx.saved_tensors
        conv, smap, pooled, dirs = ctx.conv, ctx.smap, ctx.pooled, ctx.side
        Ca, Cb = ctx.shapes
        need_a, need_b, need_w, need_beta, need_bias = ctx.needs_input_grad[:5]
        need_x = need_a or need_b
        g_raw, dbeta = _bn_relu_backward(conv, ctx.train_bn, gy.contiguous().to(a.dtype), y, raw, mean, scale, beta)
        # The form, decided once. The pooled source's gradient d_b is the pull of the input gradient's pooled half
        # dx_b; its zero rows need no index and no input gradient, so they may be written early.
        #   zeros_early: the zero rows on the side stream beside the input gradient, the sparse rows on the main
        #                stream after it (IMG_ZERO_SIDE)
        #   img_late:    zero rows, then sparse rows, on the side stream after the input gradient, beside the
        #                weight gradient on the main stream (IMG_BESIDE_WGRAD)
        #   wgrad_side:  the weight gradient on the side stream beside the input gradient -- it reads the same
        #                g_raw and writes a disjoint output (WGRAD_SIDE); otherwise on the main stream, last
        # none of them (or no device): input gradient, whole pull, weight gradient, one after the other.
        cuda = g_raw.is_cuda
        wgrad_side = cuda and need_x and need_w and conv.WGRAD_SIDE
        zero_side = cuda and pooled and b is not None and need_b and conv.IMG_ZERO_SIDE
        img_late = zero_side and conv.IMG_BESIDE_WGRAD and need_w and not wgrad_side
        zeros_early = zero_side and not img_late
        fork = zeros_early or img_late or wgrad_side
        if fork:
            cur, side = torch.cuda.current_stream(g_raw.device), _side_stream(g_raw.device)
        d_a = d_b = dx_b = dw = None

        def zero_rows():  # (the dense half reads no source rows: any aligned map stands in for dx_b)
            sm.pull(smap, *dirs.grad, d_b, Cb, 0, Cb, d_b, Cb, part="dense")

        def pull_sparse():
            sm.pull(smap, *dirs.grad, dx_b, Cb, 0, Cb, d_b, Cb, part="sparse")

        def wgrad():
            return _FusionConvFn._wgrad(ctx, a, b, weights, g_raw)

        if zeros_early or wgrad_side:  # beside the input gradient
            side.wait_stream(cur)
            if zeros_early:
                d_b = torch.empty(b.shape, dtype=a.dtype, device=a.device)
            with torch.cuda.stream(side):
                if zeros_early:
                    zero_rows()
                    zeros_done = torch.cuda.Event()
                    zeros_done.record(side)
                if wgrad_side:
                    dw = wgrad()
            for t in (a, b, g_raw, ctx.fwd_ws, ctx.xb, d_b):
                if t is not None:
                    t.record_stream(side)
        if need_x and b is None:
            d_a = conv3x3_dgrad(g_raw, weights, Ca)
        elif need_x:  # the epilogue writes the two sources' gradients as separate dense maps
            occ = pooled and ctx.fwd_ws is not None and conv.DGRAD_OCC and need_b
            d_a, dx_b = conv3x3_dgrad(g_raw, weights, Ca + Cb, split=Ca, pool=smap.csr(*dirs.fwd) if occ else None,
                                      fwd_ws=ctx.fwd_ws if occ else None, fwd_stats=ctx.train_bn)
            if img_late:
                side.wait_stream(cur)
                d_b = torch.empty(b.shape, dtype=a.dtype, device=a.device)
                with torch.cuda.stream(side):
                    zero_rows()
                    pull_sparse()
                for t in (dx_b, d_b):
                    t.record_stream(side)
            elif zeros_early:  # its zero rows are on the side stream already
                cur.wait_event(zeros_done)
                pull_sparse()
            elif need_b:
                d_b = _pull_back(smap, dirs, dx_b, b) if pooled else dx_b
        if not need_a:
            d_a = None
        if img_late:  # on the main stream, beside the side's image gradient
            dw = wgrad()
        if fork:
            cur.wait_stream(side)
            if wgrad_side:
                dw.record_stream(cur)
        if dw is None and need_w:
            dw = wgrad()
        return (d_a, d_b, dw, *_beta_bias_grads(conv, dbeta, need_beta, need_bias), None, None, None, None, None)

    @staticmethod
    def _wgrad(ctx, a, b, weights, g_raw):
        smap, pooled = ctx.smap, ctx.pooled
        if pooled and a.dtype == torch.bfloat16:
            # k_wgrad_rows gathers the pooled rows from a compact per-run buffer: bv_fused never stored
            dw = conv3x3_wgrad(a, g_raw, b=b, pool=smap.csr(*ctx.side.fwd), frame_off=smap.frame_off,
                               fwd_ws=ctx.fwd_ws, fwd_stats=ctx.train_bn)
        elif pooled:
            # f32: the pooled channels once into HBM (shpl_pull): the dense two-source weight gradient
            # runs at twice the waves per SIMD of the one that recomputes them per tile (257 vs
            # 214 registers); conv3x3_wgrad(..., pool=...) stays the memory-lean form
            xb = ctx.xb if ctx.xb is not None else ctx.side.pool(smap, b, tuple(a.shape[:3]) + (ctx.shapes[1],))
            dw = conv3x3_wgrad(a, g_raw, b=xb)
        else:
            dw = conv3x3_wgrad(a, g_raw, b=b)
        return dw.to(weights.dtype)


_SIDE = {}


def _side_stream(dev):
    """One side stream per device for the weight gradient (created once: stream creation is not free)."""
    s = _SIDE.get(dev)
    if s is None:
        s = _SIDE[dev] = torch.cuda.Stream(device=dev)
    return s


class FusionConv:
    """slim.conv2d(x, c_out, [3,3]) with slim.batch_norm (or a bias) and ReLU:
    the variables of one ``pyramid_fusion_pooled_*`` scope and its forward."""

    # bf16 fused(): the weight gradient reads the pooled operand its forward prepared (False: prepares its own)
    WGRAD_REUSE = True
    # backward, beside the input gradient on a side stream: the image gradient's zero rows (IMG_ZERO_SIDE) and
    # the weight gradient (WGRAD_SIDE; False: after the input gradient on one stream -- the two convs side by
    # side measured slower: 7.34-7.35 vs 7.14-7.20 ms per bf16 training step, profiles/r05_wside_ab.log)
    IMG_ZERO_SIDE = True
    WGRAD_SIDE = False
    # bf16 fused() backward: the input gradient's pooled channels stored at the occupied cells only, by the
    # forward's occupancy words (shpl_conv3x3_dgrad_reuse; False: the whole map, shpl_conv3x3_dgrad)
    DGRAD_OCC = True
    # the image gradient (zero rows, then the pull of the pooled channels' gradient) on the side stream after the
    # input gradient, beside the weight gradient (False: only its zero rows, beside the input gradient): 6.93-7.00
    # against 6.98-7.04 ms per bf16 training step, interleaved (profiles/r06_ab/beside_*)
    IMG_BESIDE_WGRAD = True
    # what FusionUpconv overrides: the library call (its weight layout, its output rows per input pixel) and the
    # prefix of the cached workspaces' keys
    _CALL, _WS_KEY = _CONV, ()

    def __init__(self, c_in, c_out, batch_norm=True, bias=False, relu=True, eps=1e-3, decay=0.999,
                 dtype=torch.float32, device="cuda", seed=0):
        g = np.random.default_rng(seed)
        # xavier_initializer (uniform), slim's default weights_initializer, over the variable's shape: fans 9 c_in
        # and 9 c_out in either layout
        lim = float(np.sqrt(6.0 / (9 * c_in + 9 * c_out)))
        shape = [3, 3, 0, 0]
        shape[self._CALL.w_in], shape[self._CALL.w_out] = c_in, c_out
        w = g.uniform(-lim, lim, size=shape).astype(np.float32)
        self.c_in, self.c_out = int(c_in), int(c_out)
        self.device, self.dtype = torch.device(device), dtype
        self.weights = torch.from_numpy(w).to(self.device, dtype)
        self.batch_norm, self.relu, self.eps, self.decay = batch_norm, relu, float(eps), float(decay)
        f32 = dict(dtype=torch.float32, device=self.device)
        self.beta = torch.zeros(c_out, **f32) if batch_norm else None
        self.moving_mean = torch.zeros(c_out, **f32) if batch_norm else None
        self.moving_var = torch.ones(c_out, **f32) if batch_norm else None
        self.bias = torch.zeros(c_out, **f32) if (bias and not batch_norm) else None
        self._ws = {}
        self._scale = torch.empty(c_out, **f32) if batch_norm else None
        if batch_norm:
            self._refresh_scale()

    def _inference_epilogue(self):
        if not self.batch_norm:
            return None, None, self.bias
        # FusedBatchNorm inference: (x - moving_mean) * rsqrt(moving_var + eps) + beta. The scale lives in one
        # tensor, rewritten ON THE DEVICE right after every batch_norm_train (which updates moving_var through
        # its device pointer, bumping no tensor version), so a training step replayed from a captured graph
        # refreshes it too, and an inference graph reads the current one; an eager in-place update of moving_var
        # (its version) refreshes it here. An inference step launches nothing for it.
        if self._scale_key != (self.moving_var.data_ptr(), self.moving_var._version, self.eps):
            self._refresh_scale()
        return self.moving_mean, self._scale, self.beta

    def _refresh_scale(self):
        """self._scale = 1 / sqrt(moving_var + eps), in place (three launches, stream-ordered, capturable)."""
        torch.add(self.moving_var, self.eps, out=self._scale)
        self._scale.sqrt_().reciprocal_()
        self._scale_key = (self.moving_var.data_ptr(), self.moving_var._version, self.eps)

    def _ws_for(self, key, nbytes):
        t = self._ws.get(key)
        if t is None or t.numel() < nbytes:
            t = L.workspace(nbytes, self.device)
            self._ws[key] = t
        return t

    def _forward(self, a, b, pool, frame_off, is_training, out, keep=False, ws=None):
        """The forward of [a || b] (b dense, pooled through ``pool``, or None). keep: also what the backward needs
        -- (y, raw, mean, scale): raw kept apart from y, the inference scale a copy. ws None: the module's cached
        workspace for these sizes."""
        B, H, W, Ca = (int(s) for s in a.shape)
        Cb = 0 if b is None else int(b.shape[-1])
        dt = L.dtype_code(a)
        train_bn = self.batch_norm and is_training
        if ws is None:
            cap = None if pool is None else pool.nnz_cap
            ws = self._ws_for(self._WS_KEY + (dt, B, H, W, Cb, cap, train_bn),
                              L.ws_bytes(self._CALL.symbol, dt, B, H, W, Ca, Cb, self.c_out, cap, train_bn))
        if not train_bn:
            center, scale, shift = self._inference_epilogue()
            if keep and scale is not None:  # saved for the backward: a copy, not the buffer a training step rewrites
                scale = scale.clone()
            y = _fused_call(self._CALL, a, self.weights, b, pool, frame_off, center, scale, shift, self.relu, None, out,
                           ws)
            return (y, None, center, scale) if keep else y
        stats = torch.empty((2, self.c_out), dtype=torch.float64, device=a.device)
        raw = _fused_call(self._CALL, a, self.weights, b, pool, frame_off, None, None, None, False, stats,
                         None if keep else out, ws)
        bn_ws = torch.empty(2 * self.c_out, dtype=torch.float32, device=a.device)
        y = (out if out is not None else torch.empty_like(raw)) if keep else None  # None: normalised in place
        y = batch_norm_train(raw, stats, B * self._CALL.up ** 2 * H * W, eps=self.eps, beta=self.beta, relu=self.relu,
                             moving_mean=self.moving_mean, moving_var=self.moving_var, decay=self.decay, out=y,
                             ws=bn_ws)
        self._refresh_scale()  # batch_norm_train updated the moving statistics through their device pointers
        return (y, raw, bn_ws[:self.c_out], bn_ws[self.c_out:]) if keep else y

    def _apply(self, a, b, smap, side, is_training, out):
        """The forward under autograd: the module's Function."""
        return _FusionConvFn.apply(a, b, self.weights, self.beta, self.bias, self, smap, side, is_training, out)

    def _grad_wanted(self, *tensors):
        return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in
                                               (*tensors, self.weights, self.beta, self.bias))

    def __call__(self, x, is_training=False, out=None):
        """The conv of a materialised map (bv_fused, img_fused, or img)."""
        if self._grad_wanted(x):
            return self._apply(x, None, None, None, is_training, out)
        return self._forward(x, None, None, None, is_training, out)

    def fused(self, bev, img, smap, is_training=False, out=None):
        """The conv of [bev || _sparse_pool_op(M, img)] without writing the
        concat: ``smap`` is the ShplMap of the frames of ``bev``. Differentiable
        in bev, img, the weights and beta / bias."""
        if self._grad_wanted(bev, img):
            return self._apply(bev, img, smap, SIDE_BEV, is_training, out)
        return self.fused_csr(bev, img, smap.csr(*SIDE_BEV.fwd), smap.frame_off, is_training, out)

    def fused_csr(self, bev, img, csr, frame_off, is_training=False, out=None):
        """fused() over an already built cell-keyed CSR (``_lib.Csr``) and the
        per-frame entry slots ``frame_off`` (FusedPipeline.csr / .frame_off);
        forward only."""
        return self._forward(bev, img, csr, frame_off, is_training, out)

    def fused_img(self, img, bev, smap, is_training=False, out=None):
        """The conv of [img || _sparse_pool_trans_op(M, bev)] (img_fused of the dual
        sparse_pool_layer) without writing the concat: ``smap`` is the ShplMap of the
        frames of ``img``. Differentiable in img, bev, the weights and beta / bias."""
        if int(bev.numel()) // max(int(bev.shape[-1]), 1) != smap.n_cells:
            raise ValueError(f"BEV map {tuple(bev.shape)} has {int(bev.numel()) // max(int(bev.shape[-1]), 1)} rows, "
                             f"the map {smap.n_cells} cells")
        if self._grad_wanted(img, bev):
            return self._apply(img, bev, smap, SIDE_IMG, is_training, out)
        return self.fused_img_csr(img, bev, smap.csr(*SIDE_IMG.fwd), smap.frame_off, is_training, out)

    def fused_img_csr(self, img, bev, csr, frame_off, is_training=False, out=None):
        """fused_img() over an already built pixel-keyed CSR (``_lib.Csr``: BY_PIXEL, ORDER_COL_ROW, with ent_col
        or flagged identity columns) and the per-frame entry slots ``frame_off`` (FusedPipeline.pcsr /
        .frame_off); forward only."""
        return self._forward(img, bev, csr, frame_off, is_training, out)


class _TwoScopes:
    """A BEV scope over [bev || pool(img)] and an image scope over [img || trans(bev)] (dual) or img itself, with
    the module's own side stream: what PostFusion and fusion_upconv.AfterVggFusion share."""

    def __init__(self, c_bev, c_img, dual, bev, img):
        self.c_bev, self.c_img, self.dual = int(c_bev), int(c_img), bool(dual)
        self.bev, self.img = bev, img
        self._side = None

    def __call__(self, bev, img, smap, is_training=False):
        """(bev_out, img_out): the BEV scope on the current stream, the image scope on the module's side stream,
        which the current stream then waits for. Gradients into bev and img from the two scopes add in autograd."""
        cur = torch.cuda.current_stream(bev.device)
        if self._side is None:
            self._side = torch.cuda.Stream(device=bev.device)
        side = self._side
        if self.dual:  # both CSRs on the current stream, before the fork: the map builds each once, stream-ordered
            smap.csr(*SIDE_IMG.fwd)
        smap.csr(*SIDE_BEV.fwd)
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            if self.dual:
                img_out = self.img.fused_img(img, bev, smap, is_training)
            else:
                img_out = self.img(img, is_training)
        bev_out = self.bev.fused(bev, img, smap, is_training)
        for t in (bev, img, self.img.weights):
            t.record_stream(side)
        cur.wait_stream(side)
        img_out.record_stream(cur)
        return bev_out, img_out


class PostFusion(_TwoScopes):
    """Both convs that follow the SHPL under rpn_sparse_pooling_conv_after_fusion (rpn_model.py:338-354):
    ``pyramid_fusion_pooled_bev`` over bv_fused = [bev || pool(img)] and ``pyramid_fusion_pooled_img`` over
    img_fused -- [img || trans(bev)] for a dual layer, img itself otherwise (bv_index=None, the RPN's own call).
    ``dual`` fixes the image conv's input channels, as it fixes the graph in the reference. depths: the output
    channels (bev conv, img conv); default the reference's feature_depths = (c_img, c_bev)."""

    def __init__(self, c_bev, c_img, depths=None, dual=True, dtype=torch.float32, device="cuda", seed=0, **kw):
        d_bev, d_img = (c_img, c_bev) if depths is None else depths
        super().__init__(c_bev, c_img, dual,
                         FusionConv(c_bev + c_img, d_bev, dtype=dtype, device=device, seed=seed, **kw),
                         FusionConv(c_img + (c_bev if dual else 0), d_img, dtype=dtype, device=device, seed=seed + 1,
                                    **kw))

    def __call__(self, bev, img, smap, dual=None, is_training=False):
        """(bev_out, img_out): the BEV conv on the current stream, the image conv on the module's side stream,
        which the current stream then waits for (_TwoScopes)."""
        dual = self.dual if dual is None else bool(dual)
        if dual != self.dual:
            raise ValueError(f"this PostFusion's image conv was built for dual={self.dual}")
        return super().__call__(bev, img, smap, is_training)
