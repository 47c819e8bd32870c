"""MV3D's 1x1 RPN heads over the fused map, with the SHPL applied after the projection.

The reference's second caller pools the image features to the BEV grid, concatenates them with the lidar
features and runs two 1x1 convs over the 1536-channel map
(MV3D_TF_release/lib/networks/MV3D_voxel_train.py:144-178):

    img_features_pooled = sparse_pool(M, img_features, idx)            # network.py:243-246
    conv_lidar_fused    = concat(lidar_features, img_features_pooled)  # (-> dropout when use_dropout)
    rpn_cls_score       = conv(1, 1, 4, 1, 1, padding='VALID', relu=False)
    rpn_bbox_pred       = conv(1, 1, 14, 1, 1, padding='VALID', relu=False)

A 1x1 conv and the SHPL are both linear, so ``FusionHead.fused(lidar, img, smap)`` applies the heads to the
image map first (Z = img . W_img, 18 channels per pixel) and pools Z instead of the 768 image channels
(shpl_head1x1 with a pool CSR): neither the pooled map nor the concat reaches HBM, and every head shares one
pass over the two feature maps. The backward is the TF autodiff of the same graph on the device: the incoming
gradients of all heads joined into one map, pulled back to the pixels at 18 channels through the pixel-keyed
CSR, then the input gradients (shpl_head1x1_dgrad) and the weight / bias gradients (shpl_head1x1_wgrad, two
stages, no atomics). ``FusionHead.__call__(fused_map)`` is the same heads over a materialised
conv_lidar_fused.

The result equals the heads of [lidar || shpl_pull(BY_CELL)] up to summation order, not bitwise
(include/shpl.h states the order).

MV3D trains with dropout(keep_prob = 0.5) over conv_lidar_fused (MV3D_voxel_train.py:148-150;
train_voxelnet_fusion.py:42, train_mv_voxel.py:335). A mask between the pooling and the heads rules out projecting
first, so ``FusionHead.fused_dropout`` pools inside the GEMM's operand staging instead (shpl_head1x1_drop and its
gradients): still no pooled map, concat or mask in memory. The mask is a pure function of (seed, row, channel,
keep_prob) -- Philox4x32-10, stated in include/shpl.h -- that the backward computes again; ``FusionHead.dropout``
applies the same mask over a materialised map and ``dropout_mask`` returns it as an array.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib as L
from .fusion_conv import SIDE_BEV


def _rows(t):
    return int(t.numel()) // max(int(t.shape[-1]), 1)


def _on_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise L.ShplLibraryError("FusionHead runs on the GPU only: got a CPU tensor (there is no CPU path)")


def head_ws_bytes(dtype, rows, c_a, rows_b, c_b, c_out, pooled, wgrad=False):
    """Workspace of shpl_head1x1 / shpl_head1x1_dgrad (wgrad: of shpl_head1x1_wgrad)."""
    out = ctypes.c_size_t()
    fn, name = ((L.lib().shpl_head1x1_wgrad_workspace_bytes, "shpl_head1x1_wgrad_workspace_bytes") if wgrad else
                (L.lib().shpl_head1x1_workspace_bytes, "shpl_head1x1_workspace_bytes"))
    L.check(fn(dtype, int(rows), int(c_a), int(rows_b), int(c_b), int(c_out), int(bool(pooled)), ctypes.byref(out)),
            name)
    return out.value


def head1x1(a, weights, b=None, pool=None, bias=None, out=None):
    """[a || b] . weights + bias over the rows of a [..., Ca] (shpl_head1x1). weights [Ca+Cb, Cout] of a's dtype;
    b: a second dense map [..., Cb] of as many rows, or -- with ``pool``, the cell-keyed ``_lib.Csr`` of the
    map -- the image map [..., Cb] whose pooling is applied after the projection; bias: [Cout] f32."""
    _on_gpu(a, b, weights, bias)
    dt = L.dtype_code(a)
    a = a.contiguous()
    Ca, rows = int(a.shape[-1]), _rows(a)
    Cb, rows_b = 0, 0
    if b is not None:
        if b.dtype != a.dtype:
            raise TypeError("both inputs of the head must share one dtype")
        b = b.contiguous()
        Cb, rows_b = int(b.shape[-1]), _rows(b)
    weights = weights.to(a.dtype).contiguous()
    Cout = int(weights.shape[-1])
    if weights.numel() != (Ca + Cb) * Cout:
        raise ValueError(f"weights {tuple(weights.shape)} do not match {Ca}+{Cb} input channels")
    if bias is not None:
        bias = bias.to(torch.float32).contiguous()
    if out is None:
        out = torch.empty(tuple(a.shape[:-1]) + (Cout,), dtype=a.dtype, device=a.device)
    ws = L.workspace(head_ws_bytes(dt, rows, Ca, rows_b, Cb, Cout, pool is not None), a.device)
    L.check(L.lib().shpl_head1x1(dt, rows, L.ptr(a), Ca, 0, Ca, L.ptr(b), Cb, 0, Cb, rows_b,
                                 None if pool is None else pool.ref(), L.ptr(weights), Cout, L.ptr(bias),
                                 L.ptr(out), int(out.stride(-2)), L.ptr(ws), ws.numel(), L.stream_of(a.device)),
            "shpl_head1x1")
    return out


def head1x1_dgrad(gy, weights, c_a, a_shape=None, b_shape=None, pool_grad=None):
    """(d_a, d_b) of head1x1: gy [..., Cout]; weights [Ca+Cb, Cout]; a_shape / b_shape: the shapes of the wanted
    gradients (None: not computed); pool_grad: the pixel-keyed gradient CSR of the pooled form."""
    gy = gy.contiguous()
    dt = L.dtype_code(gy)
    weights = weights.to(gy.dtype).contiguous()
    Cout, rows = int(gy.shape[-1]), _rows(gy)
    Ca = int(c_a)
    Cb = weights.numel() // Cout - Ca
    d_a = None if a_shape is None else torch.empty(tuple(a_shape), dtype=gy.dtype, device=gy.device)
    d_b = None if b_shape is None else torch.empty(tuple(b_shape), dtype=gy.dtype, device=gy.device)
    rows_b = rows if pool_grad is None else pool_grad.n_keys
    ws = L.workspace(head_ws_bytes(dt, rows, Ca, rows_b, Cb, Cout, pool_grad is not None), gy.device)
    L.check(L.lib().shpl_head1x1_dgrad(dt, rows, L.ptr(gy), Cout, Cout, L.ptr(weights), Ca, Cb, L.ptr(d_a), Ca,
                                       L.ptr(d_b), max(Cb, 1), rows_b,
                                       None if pool_grad is None else pool_grad.ref(), L.ptr(ws), ws.numel(),
                                       L.stream_of(gy.device)), "shpl_head1x1_dgrad")
    return d_a, d_b


def head1x1_wgrad(a, gy, b=None, pool_grad=None, bias=True):
    """(dw f32 [Ca+Cb, Cout], dbias f32 [Cout] or None) of head1x1 over the same inputs."""
    a = a.contiguous()
    gy = gy.to(a.dtype).contiguous()
    dt = L.dtype_code(a)
    Ca, rows, Cout = int(a.shape[-1]), _rows(a), int(gy.shape[-1])
    Cb, rows_b = 0, 0
    if b is not None:
        b = b.contiguous()
        Cb, rows_b = int(b.shape[-1]), _rows(b)
    dw = torch.empty((Ca + Cb, Cout), dtype=torch.float32, device=a.device)
    db = torch.empty(Cout, dtype=torch.float32, device=a.device) if bias else None
    ws = L.workspace(head_ws_bytes(dt, rows, Ca, rows_b, Cb, Cout, pool_grad is not None, wgrad=True), a.device)
    L.check(L.lib().shpl_head1x1_wgrad(dt, rows, L.ptr(a), Ca, 0, Ca, L.ptr(b), Cb, 0, Cb, rows_b,
                                       None if pool_grad is None else pool_grad.ref(), L.ptr(gy), Cout,
                                       Cout, L.ptr(dw), L.ptr(db), L.ptr(ws), ws.numel(), L.stream_of(a.device)),
            "shpl_head1x1_wgrad")
    return dw, db


def _u64(seed):
    return ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)


def dropout_mask(rows, channels, keep_prob, seed, device):
    """The dropout mask of the heads as an array (shpl_dropout_mask): uint8 [rows, channels], 1 kept, 0 dropped --
    the pure function of (seed, row, channel, keep_prob) that include/shpl.h states. The head calls never read
    one; this is for checks and for callers that need the mask elsewhere."""
    device = torch.device(device)
    if device.type != "cuda":
        raise L.ShplLibraryError("dropout_mask runs on the GPU only (there is no CPU path)")
    out = torch.empty((int(rows), int(channels)), dtype=torch.uint8, device=device)
    L.check(L.lib().shpl_dropout_mask(int(rows), int(channels), float(keep_prob), _u64(seed), L.ptr(out),
                                      L.stream_of(device)), "shpl_dropout_mask")
    return out


def head_drop_ws_bytes(dtype, rows, c_a, rows_b, c_b, c_out, pooled, wgrad=False):
    """Workspace of shpl_head1x1_drop / shpl_head1x1_drop_dgrad (wgrad: of shpl_head1x1_drop_wgrad)."""
    out = ctypes.c_size_t()
    name = "shpl_head1x1_drop_wgrad_workspace_bytes" if wgrad else "shpl_head1x1_drop_workspace_bytes"
    L.check(getattr(L.lib(), name)(dtype, int(rows), int(c_a), int(rows_b), int(c_b), int(c_out), int(bool(pooled)),
                                   ctypes.byref(out)), name)
    return out.value


def head1x1_drop(a, weights, keep_prob, seed, b=None, pool=None, bias=None):
    """scale * (mask * [a || b]) . weights + bias (shpl_head1x1_drop): head1x1's arguments, the pooling of ``b``
    through ``pool`` done inside the GEMM's operand staging, the mask computed from (seed, row, channel)."""
    _on_gpu(a, b, weights, bias)
    dt = L.dtype_code(a)
    a = a.contiguous()
    Ca, rows = int(a.shape[-1]), _rows(a)
    Cb, rows_b = 0, 0
    if b is not None:
        if b.dtype != a.dtype:
            raise TypeError("both inputs of the head must share one dtype")
        b = b.contiguous()
        Cb, rows_b = int(b.shape[-1]), _rows(b)
    weights = weights.to(a.dtype).contiguous()
    Cout = int(weights.shape[-1])
    if weights.numel() != (Ca + Cb) * Cout:
        raise ValueError(f"weights {tuple(weights.shape)} do not match {Ca}+{Cb} input channels")
    if bias is not None:
        bias = bias.to(torch.float32).contiguous()
    out = torch.empty(tuple(a.shape[:-1]) + (Cout,), dtype=a.dtype, device=a.device)
    ws = L.workspace(head_drop_ws_bytes(dt, rows, Ca, rows_b, Cb, Cout, pool is not None), a.device)
    L.check(L.lib().shpl_head1x1_drop(dt, rows, L.ptr(a), Ca, 0, Ca, L.ptr(b), Cb, 0, Cb, rows_b,
                                      None if pool is None else pool.ref(), L.ptr(weights), Cout, L.ptr(bias),
                                      L.ptr(out), Cout, float(keep_prob), _u64(seed), L.ptr(ws), ws.numel(),
                                      L.stream_of(a.device)), "shpl_head1x1_drop")
    return out


def head1x1_drop_dgrad(gy, weights, c_a, keep_prob, seed, a_shape=None, b_shape=None, pool_grad=None):
    """(d_a, d_b) of head1x1_drop with the mask computed again; arguments as head1x1_dgrad."""
    gy = gy.contiguous()
    dt = L.dtype_code(gy)
    weights = weights.to(gy.dtype).contiguous()
    Cout, rows = int(gy.shape[-1]), _rows(gy)
    Ca = int(c_a)
    Cb = weights.numel() // Cout - Ca
    d_a = None if a_shape is None else torch.empty(tuple(a_shape), dtype=gy.dtype, device=gy.device)
    d_b = None if b_shape is None else torch.empty(tuple(b_shape), dtype=gy.dtype, device=gy.device)
    rows_b = rows if pool_grad is None else pool_grad.n_keys
    ws = L.workspace(head_drop_ws_bytes(dt, rows, Ca, rows_b, Cb, Cout, pool_grad is not None), gy.device)
    L.check(L.lib().shpl_head1x1_drop_dgrad(dt, rows, L.ptr(gy), Cout, Cout, L.ptr(weights), Ca, Cb, L.ptr(d_a), Ca,
                                            L.ptr(d_b), max(Cb, 1), rows_b,
                                            None if pool_grad is None else pool_grad.ref(), float(keep_prob),
                                            _u64(seed), L.ptr(ws), ws.numel(), L.stream_of(gy.device)),
            "shpl_head1x1_drop_dgrad")
    return d_a, d_b


def head1x1_drop_wgrad(a, gy, keep_prob, seed, b=None, pool=None, bias=True):
    """(dw f32 [Ca+Cb, Cout], dbias f32 [Cout] or None) of head1x1_drop; ``pool`` is the forward's cell-keyed CSR."""
    a = a.contiguous()
    gy = gy.to(a.dtype).contiguous()
    dt = L.dtype_code(a)
    Ca, rows, Cout = int(a.shape[-1]), _rows(a), int(gy.shape[-1])
    Cb, rows_b = 0, 0
    if b is not None:
        b = b.contiguous()
        Cb, rows_b = int(b.shape[-1]), _rows(b)
    dw = torch.empty((Ca + Cb, Cout), dtype=torch.float32, device=a.device)
    db = torch.empty(Cout, dtype=torch.float32, device=a.device) if bias else None
    ws = L.workspace(head_drop_ws_bytes(dt, rows, Ca, rows_b, Cb, Cout, pool is not None, wgrad=True), a.device)
    L.check(L.lib().shpl_head1x1_drop_wgrad(dt, rows, L.ptr(a), Ca, 0, Ca, L.ptr(b), Cb, 0, Cb, rows_b,
                                            None if pool is None else pool.ref(), L.ptr(gy), Cout, Cout, L.ptr(dw),
                                            L.ptr(db), float(keep_prob), _u64(seed), L.ptr(ws), ws.numel(),
                                            L.stream_of(a.device)), "shpl_head1x1_drop_wgrad")
    return dw, db


class _FusionHeadDropFn(torch.autograd.Function):
    """_FusionHeadFn under dropout over [a || pooled b]: the same inputs, then keep_prob and the seed, which the
    context keeps for the backward -- the mask is computed again there, never stored."""

    @staticmethod
    def forward(ctx, a, b, smap, sizes, keep_prob, seed, *params):
        n = len(sizes)
        ws_, bs_ = params[:n], params[n:]
        a = a.contiguous()
        b = None if b is None else b.contiguous()
        Ca = int(a.shape[-1])
        Cb = 0 if b is None else int(b.shape[-1])
        w = torch.cat([p.reshape(Ca + Cb, k) for p, k in zip(ws_, sizes)], dim=1).to(a.dtype)
        bias = torch.cat([p.to(torch.float32) for p in bs_])
        pool = None if b is None else smap.csr(*SIDE_BEV.fwd)
        if b is not None and ctx.needs_input_grad[1]:  # the gradient's CSR sorts beside the forward
            smap.prefetch_csr(*SIDE_BEV.grad)
        out = head1x1_drop(a, w, keep_prob, seed, b=b, pool=pool, bias=bias)
        ctx.smap, ctx.sizes, ctx.Ca, ctx.keep_prob, ctx.seed = smap, sizes, Ca, keep_prob, seed
        ctx.shapes = [tuple(p.shape) for p in ws_]
        ctx.save_for_backward(a, b, w)
        return tuple(t.contiguous() for t in out.split(list(sizes), dim=-1))

    @staticmethod
    def backward(ctx, *gs):
        a, b, w = ctx.saved_tensors
        sizes, n, Ca = ctx.sizes, len(ctx.sizes), ctx.Ca
        lead = tuple(a.shape[:-1])
        gy = torch.cat([torch.zeros(lead + (k,), dtype=a.dtype, device=a.device) if g is None else g.to(a.dtype)
                        for g, k in zip(gs, sizes)], dim=-1)
        need = ctx.needs_input_grad
        d_a = d_b = None
        if need[0] or (b is not None and need[1]):
            want_b = b is not None and need[1]
            d_a, d_b = head1x1_drop_dgrad(gy, w, Ca, ctx.keep_prob, ctx.seed, a_shape=a.shape if need[0] else None,
                                          b_shape=b.shape if want_b else None,
                                          pool_grad=ctx.smap.csr(*SIDE_BEV.grad) if want_b else None)
        dws, dbs = [None] * n, [None] * n
        if any(need[6:]):
            dw, db = head1x1_drop_wgrad(a, gy, ctx.keep_prob, ctx.seed, b=b,
                                        pool=None if b is None else ctx.smap.csr(*SIDE_BEV.fwd),
                                        bias=any(need[6 + n:]))
            for i, (part, shape) in enumerate(zip(dw.split(list(sizes), dim=1), ctx.shapes)):
                if need[6 + i]:
                    dws[i] = part.reshape(shape).to(w.dtype)
            if db is not None:
                for i, part in enumerate(db.split(list(sizes))):
                    if need[6 + n + i]:
                        dbs[i] = part.contiguous()
        return (d_a, d_b, None, None, None, None, *dws, *dbs)


class _FusionHeadFn(torch.autograd.Function):
    """All heads in one pass, forward and backward. Inputs: a [B,H,W,Ca]; b: None (a is the materialised map) or
    the image map pooled through smap; then every head's weights, then every head's bias."""

    @staticmethod
    def forward(ctx, a, b, smap, sizes, *params):
        n = len(sizes)
        ws_, bs_ = params[:n], params[n:]
        a = a.contiguous()
        b = None if b is None else b.contiguous()
        Ca = int(a.shape[-1])
        Cb = 0 if b is None else int(b.shape[-1])
        w = torch.cat([p.reshape(Ca + Cb, k) for p, k in zip(ws_, sizes)], dim=1).to(a.dtype)
        bias = torch.cat([p.to(torch.float32) for p in bs_])
        pool = None if b is None else smap.csr(*SIDE_BEV.fwd)
        need = ctx.needs_input_grad
        if b is not None and (need[1] or any(need[4:4 + n])):  # the gradient's CSR sorts beside the forward
            smap.prefetch_csr(*SIDE_BEV.grad)
        out = head1x1(a, w, b=b, pool=pool, bias=bias)
        ctx.smap, ctx.sizes, ctx.Ca = smap, sizes, Ca
        ctx.shapes = [tuple(p.shape) for p in ws_]
        ctx.save_for_backward(a, b, w)
        return tuple(t.contiguous() for t in out.split(list(sizes), dim=-1))

    @staticmethod
    def backward(ctx, *gs):
        a, b, w = ctx.saved_tensors
        sizes, n, Ca = ctx.sizes, len(ctx.sizes), ctx.Ca
        lead = tuple(a.shape[:-1])
        # the heads' gradients joined into one [., sum n] map: one pass for all of them
        gy = torch.cat([torch.zeros(lead + (k,), dtype=a.dtype, device=a.device) if g is None else g.to(a.dtype)
                        for g, k in zip(gs, sizes)], dim=-1)
        need = ctx.needs_input_grad
        pool_grad = None if b is None else ctx.smap.csr(*SIDE_BEV.grad)
        d_a = d_b = None
        if need[0] or (b is not None and need[1]):
            d_a, d_b = head1x1_dgrad(gy, w, Ca, a_shape=a.shape if need[0] else None,
                                     b_shape=b.shape if (b is not None and need[1]) else None, pool_grad=pool_grad)
        dws, dbs = [None] * n, [None] * n
        if any(need[4:]):
            dw, db = head1x1_wgrad(a, gy, b=b, pool_grad=pool_grad, bias=any(need[4 + n:]))
            for i, (part, shape) in enumerate(zip(dw.split(list(sizes), dim=1), ctx.shapes)):
                if need[4 + i]:
                    dws[i] = part.reshape(shape).to(w.dtype)
            if db is not None:
                for i, part in enumerate(db.split(list(sizes))):
                    if need[4 + n + i]:
                        dbs[i] = part.contiguous()
        return (d_a, d_b, None, None, *dws, *dbs)


class FusionHead:
    """The 1x1 heads that follow conv_lidar_fused in MV3D (rpn_cls_score: 4 channels, rpn_bbox_pred: 14): one
    weight [1, 1, c_lidar + c_img, n] and one zero-initialised bias [n] (f32) per head, as Network.conv makes them
    (network.py:131-148: xavier_initializer_conv2d, constant 0), VALID, stride 1, no ReLU."""

    def __init__(self, c_lidar, c_img, heads=(4, 14), dtype=torch.float32, device="cuda", seed=0):
        self.c_lidar, self.c_img = int(c_lidar), int(c_img)
        self.heads = tuple(int(n) for n in heads)
        if not self.heads or min(self.heads) < 1 or sum(self.heads) > 32:
            raise ValueError(f"heads {heads}: between 1 and 32 output channels in all")
        self.device, self.dtype = torch.device(device), dtype
        g = np.random.default_rng(seed)
        c_in = self.c_lidar + self.c_img
        self.weights, self.biases = [], []
        for n in self.heads:
            lim = float(np.sqrt(6.0 / (c_in + n)))  # xavier (uniform) over a 1x1 kernel: fan_in c_in, fan_out n
            w = g.uniform(-lim, lim, size=(1, 1, c_in, n)).astype(np.float32)
            self.weights.append(torch.from_numpy(w).to(self.device, dtype))
            self.biases.append(torch.zeros(n, dtype=torch.float32, device=self.device))

    def _apply(self, a, b, smap):
        _on_gpu(a, b)
        outs = _FusionHeadFn.apply(a, b, smap, self.heads, *self.weights, *self.biases)
        return tuple(outs)

    def __call__(self, fused_map):
        """The heads of a materialised conv_lidar_fused [B, H, W, c_lidar + c_img]: one tensor per head."""
        if int(fused_map.shape[-1]) != self.c_lidar + self.c_img:
            raise ValueError(f"fused map {tuple(fused_map.shape)} does not hold {self.c_lidar}+{self.c_img} channels")
        return self._apply(fused_map, None, None)

    def fused(self, lidar, img, smap, keep_prob=1.0):
        """(rpn_cls_score, rpn_bbox_pred, ...) of [lidar || sparse_pool(M, img)] without writing the pooled map
        or the concat; ``smap`` is the ShplMap of the frames of ``lidar``. Differentiable in lidar, img, every
        weight and every bias."""
        if keep_prob != 1.0:
            raise NotImplementedError(
                "FusionHead.fused applies the heads before the pooling, which needs the heads to be linear in the "
                "pooled map; a dropout mask over the concat (keep_prob < 1) is not. Materialise the map instead: "
                "mv3d.sparse_pool, then the concat, dropout and 1x1 convs in torch")
        if int(lidar.shape[-1]) != self.c_lidar or int(img.shape[-1]) != self.c_img:
            raise ValueError(f"maps {tuple(lidar.shape)}, {tuple(img.shape)} do not hold {self.c_lidar} and "
                             f"{self.c_img} channels")
        if _rows(lidar) != smap.n_cells or _rows(img) != smap.n_pix:
            raise ValueError(f"maps of {_rows(lidar)} cells and {_rows(img)} pixels, the map {smap.n_cells} and "
                             f"{smap.n_pix}")
        return self._apply(lidar, img, smap)

    def _apply_dropout(self, a, b, smap, keep_prob, seed):
        _on_gpu(a, b)
        keep_prob = float(keep_prob)
        if not 0.0 < keep_prob <= 1.0:
            raise ValueError(f"keep_prob {keep_prob}: a probability in (0, 1]")
        if seed is None:  # torch's default CPU generator: torch.manual_seed governs it
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
        outs = _FusionHeadDropFn.apply(a, b, smap, self.heads, keep_prob, int(seed), *self.weights, *self.biases)
        return tuple(outs)

    def dropout(self, fused_map, keep_prob, seed=None):
        """The heads of dropout(conv_lidar_fused, keep_prob) over a materialised map [B, H, W, c_lidar + c_img], as
        MV3D trains them (MV3D_voxel_train.py:148-178 with use_dropout): the mask of include/shpl.h over
        (row, channel), computed in the kernels and again in the backward, never stored. seed: an integer, or
        None to draw one from torch's default CPU generator. Differentiable in the map, every weight and bias."""
        if int(fused_map.shape[-1]) != self.c_lidar + self.c_img:
            raise ValueError(f"fused map {tuple(fused_map.shape)} does not hold {self.c_lidar}+{self.c_img} channels")
        return self._apply_dropout(fused_map, None, None, keep_prob, seed)

    def fused_dropout(self, lidar, img, smap, keep_prob, seed=None):
        """The heads of dropout([lidar || sparse_pool(M, img)], keep_prob) without writing the pooled map, the
        concat or a mask: the pooling runs inside the GEMM's operand staging and the mask is computed from
        (seed, row, channel). The same mask as ``dropout`` over the materialised map with the same seed.
        Differentiable in lidar, img, every weight and every bias."""
        if int(lidar.shape[-1]) != self.c_lidar or int(img.shape[-1]) != self.c_img:
            raise ValueError(f"maps {tuple(lidar.shape)}, {tuple(img.shape)} do not hold {self.c_lidar} and "
                             f"{self.c_img} channels")
        if _rows(lidar) != smap.n_cells or _rows(img) != smap.n_pix:
            raise ValueError(f"maps of {_rows(lidar)} cells and {_rows(img)} pixels, the map {smap.n_cells} and "
                             f"{smap.n_pix}")
        return self._apply_dropout(lidar, img, smap, keep_prob, seed)
