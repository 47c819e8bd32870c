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


def _inputs(a, b, weights=None, bias=None):
    """The operands as the calls take them: contiguous maps of one dtype, the weights in that dtype, the bias f32."""
    a = a.contiguous()
    if b is not None:
        if b.dtype != a.dtype:
            raise TypeError("both inputs of the head must share one dtype")
        b = b.contiguous()
    if weights is not None:
        weights = weights.to(a.dtype).contiguous()
    if bias is not None:
        bias = bias.to(torch.float32).contiguous()
    return a, b, weights, bias


def _dims(a, b):
    """(Ca, rows, Cb, rows_b); no second source: 0, 0."""
    return (int(a.shape[-1]), _rows(a)) + ((0, 0) if b is None else (int(b.shape[-1]), _rows(b)))


def _u64(seed):
    return ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)


# mask: None for the plain heads, (keep_prob, seed) for the heads under dropout -- the shpl_head1x1_drop* symbols,
# which take the two after the plain call's arguments and before the workspace
def _symbol(drop, kind=""):
    return "shpl_head1x1" + ("_drop" if drop else "") + kind


def _mask_args(mask):
    return () if mask is None else (float(mask[0]), _u64(mask[1]))


def _csr_ref(csr):
    return None if csr is None else csr.ref()


def _workspace(mask, kind, device, *shape):
    return L.workspace(L.ws_bytes(_symbol(mask is not None, kind), *shape), device)


def head_ws_bytes(dtype, rows, c_a, rows_b, c_b, c_out, pooled, wgrad=False):
    """Workspace of shpl_head1x1 / shpl_head1x1_dgrad (wgrad: of shpl_head1x1_wgrad)."""
    return L.ws_bytes(_symbol(False, "_wgrad" if wgrad else ""), dtype, rows, c_a, rows_b, c_b, c_out, bool(pooled))


def head_drop_ws_bytes(dtype, rows, c_a, rows_b, c_b, c_out, pooled, wgrad=False):
    """Workspace of shpl_head1x1_drop / shpl_head1x1_drop_dgrad (wgrad: of shpl_head1x1_drop_wgrad)."""
    return L.ws_bytes(_symbol(True, "_wgrad" if wgrad else ""), dtype, rows, c_a, rows_b, c_b, c_out, bool(pooled))


def _forward(a, weights, b, pool, bias, out, mask):
    _on_gpu(a, b, weights, bias)
    dt = L.dtype_code(a)
    a, b, weights, bias = _inputs(a, b, weights, bias)
    Ca, rows, Cb, rows_b = _dims(a, b)
    Cout = int(weights.shape[-1])
    if weights.numel() != (Ca + Cb) * Cout:
        raise ValueError(f"weights {tuple(weights.shape)} do not match {Ca}+{Cb} input channels")
    if out is None:
        out = torch.empty(tuple(a.shape[:-1]) + (Cout,), dtype=a.dtype, device=a.device)
    ws = _workspace(mask, "", a.device, dt, rows, Ca, rows_b, Cb, Cout, pool is not None)
    name = _symbol(mask is not None)
    L.check(getattr(L.lib(), name)(dt, rows, L.ptr(a), Ca, 0, Ca, L.ptr(b), Cb, 0, Cb, rows_b, _csr_ref(pool),
                                   L.ptr(weights), Cout, L.ptr(bias), L.ptr(out), int(out.stride(-2)),
                                   *_mask_args(mask), L.ptr(ws), ws.numel(), L.stream_of(a.device)), name)
    return out


def _dgrad(gy, weights, c_a, a_shape, b_shape, pool_grad, mask):
    gy = gy.contiguous()
    dt = L.dtype_code(gy)
    weights = weights.to(gy.dtype).contiguous()
    Cout, rows = int(gy.shape[-1]), _rows(gy)
    Ca = int(c_a)
    Cb = weights.numel() // Cout - Ca
    d_a = None if a_shape is None else torch.empty(tuple(a_shape), dtype=gy.dtype, device=gy.device)
    d_b = None if b_shape is None else torch.empty(tuple(b_shape), dtype=gy.dtype, device=gy.device)
    rows_b = rows if pool_grad is None else pool_grad.n_keys
    ws = _workspace(mask, "", gy.device, dt, rows, Ca, rows_b, Cb, Cout, pool_grad is not None)
    name = _symbol(mask is not None, "_dgrad")
    L.check(getattr(L.lib(), name)(dt, rows, L.ptr(gy), Cout, Cout, L.ptr(weights), Ca, Cb, L.ptr(d_a), Ca, L.ptr(d_b),
                                   max(Cb, 1), rows_b, _csr_ref(pool_grad), *_mask_args(mask), L.ptr(ws), ws.numel(),
                                   L.stream_of(gy.device)), name)
    return d_a, d_b


def _wgrad(a, gy, b, pool, bias, mask):
    a, b, _, _ = _inputs(a, b)
    gy = gy.to(a.dtype).contiguous()
    dt = L.dtype_code(a)
    Ca, rows, Cb, rows_b = _dims(a, b)
    Cout = int(gy.shape[-1])
    dw = torch.empty((Ca + Cb, Cout), dtype=torch.float32, device=a.device)
    db = torch.empty(Cout, dtype=torch.float32, device=a.device) if bias else None
    ws = _workspace(mask, "_wgrad", a.device, dt, rows, Ca, rows_b, Cb, Cout, pool is not None)
    name = _symbol(mask is not None, "_wgrad")
    L.check(getattr(L.lib(), name)(dt, rows, L.ptr(a), Ca, 0, Ca, L.ptr(b), Cb, 0, Cb, rows_b, _csr_ref(pool), L.ptr(gy),
                                   Cout, Cout, L.ptr(dw), L.ptr(db), *_mask_args(mask), L.ptr(ws), ws.numel(),
                                   L.stream_of(a.device)), name)
    return dw, db


def head1x1(a, weights, b=None, pool=None, bias=None, out=None):
    """[a || b] . weights + bias over the rows of a [..., Ca] (shpl_head1x1). weights [Ca+Cb, Cout] of a's dtype;
    b: a second dense map [..., Cb] of as many rows, or -- with ``pool``, the cell-keyed ``_lib.Csr`` of the
    map -- the image map [..., Cb] whose pooling is applied after the projection; bias: [Cout] f32."""
    return _forward(a, weights, b, pool, bias, out, None)


def head1x1_dgrad(gy, weights, c_a, a_shape=None, b_shape=None, pool_grad=None):
    """(d_a, d_b) of head1x1: gy [..., Cout]; weights [Ca+Cb, Cout]; a_shape / b_shape: the shapes of the wanted
    gradients (None: not computed); pool_grad: the pixel-keyed gradient CSR of the pooled form."""
    return _dgrad(gy, weights, c_a, a_shape, b_shape, pool_grad, None)


def head1x1_wgrad(a, gy, b=None, pool_grad=None, bias=True):
    """(dw f32 [Ca+Cb, Cout], dbias f32 [Cout] or None) of head1x1 over the same inputs."""
    return _wgrad(a, gy, b, pool_grad, bias, None)


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


def head1x1_drop(a, weights, keep_prob, seed, b=None, pool=None, bias=None):
    """scale * (mask * [a || b]) . weights + bias (shpl_head1x1_drop): head1x1's arguments, the pooling of ``b``
    through ``pool`` done inside the GEMM's operand staging, the mask computed from (seed, row, channel)."""
    return _forward(a, weights, b, pool, bias, None, (keep_prob, seed))


def head1x1_drop_dgrad(gy, weights, c_a, keep_prob, seed, a_shape=None, b_shape=None, pool_grad=None):
    """(d_a, d_b) of head1x1_drop with the mask computed again; arguments as head1x1_dgrad."""
    return _dgrad(gy, weights, c_a, a_shape, b_shape, pool_grad, (keep_prob, seed))


def head1x1_drop_wgrad(a, gy, keep_prob, seed, b=None, pool=None, bias=True):
    """(dw f32 [Ca+Cb, Cout], dbias f32 [Cout] or None) of head1x1_drop; ``pool`` is the forward's cell-keyed CSR."""
    return _wgrad(a, gy, b, pool, bias, (keep_prob, seed))


_PARAMS = 6  # the inputs of _FusionHeadFn before every head's weights and biases


class _FusionHeadFn(torch.autograd.Function):
    """All heads in one pass, forward and backward. Inputs: a [B,H,W,Ca]; b: None (a is the materialised map) or
    the image map pooled through smap; the heads' widths; keep_prob and the seed of the heads under dropout over
    [a || pooled b] (None, None: the plain heads) -- the context keeps them for the backward, where the mask is
    computed again, never stored; then every head's weights, then every head's bias."""

    @staticmethod
    def forward(ctx, a, b, smap, sizes, keep_prob, seed, *params):
        n = len(sizes)
        ws_, bs_ = params[:n], params[n:]
        a, b, _, _ = _inputs(a, b)
        Ca, _, Cb, _ = _dims(a, b)
        w = torch.cat([p.reshape(Ca + Cb, k) for p, k in zip(ws_, sizes)], dim=1).to(a.dtype)
        bias = torch.cat([p.to(torch.float32) for p in bs_])
        mask = None if keep_prob is None else (keep_prob, seed)
        pool = None if b is None else smap.csr(*SIDE_BEV.fwd)
        # the gradient's CSR sorts beside the forward: the image gradient takes it, and so does the weight gradient
        # of the plain heads
        need = ctx.needs_input_grad
        if b is not None and (need[1] or (mask is None and any(need[_PARAMS:_PARAMS + n]))):
            smap.prefetch_csr(*SIDE_BEV.grad)
        out = _forward(a, w, b, pool, bias, None, mask)
        ctx.smap, ctx.sizes, ctx.Ca, ctx.mask = smap, sizes, Ca, mask
        ctx.shapes = [tuple(p.shape) for p in ws_]
        ctx.save_for_backward(a, b, w)
        return tuple(t.contiguous() for t in out.split(list(sizes), dim=-1))

    @staticmethod
    def backward(ctx, *gs):
        a, b, w = ctx.saved_tensors
        sizes, n, Ca, mask = ctx.sizes, len(ctx.sizes), ctx.Ca, ctx.mask
        lead = tuple(a.shape[:-1])
        # the heads' gradients joined into one [., sum n] map: one pass for all of them
        gy = torch.cat([torch.zeros(lead + (k,), dtype=a.dtype, device=a.device) if g is None else g.to(a.dtype)
                        for g, k in zip(gs, sizes)], dim=-1)
        need = ctx.needs_input_grad
        want_b = b is not None and need[1]
        d_a = d_b = None
        if need[0] or want_b:
            d_a, d_b = _dgrad(gy, w, Ca, a.shape if need[0] else None, b.shape if want_b else None,
                              ctx.smap.csr(*SIDE_BEV.grad) if want_b else None, mask)
        dws, dbs = [None] * n, [None] * n
        if any(need[_PARAMS:]):
            # the plain heads pull gy back to the pixels: the pixel-keyed gradient CSR; under dropout the weight
            # gradient pools b again as the forward did: its cell-keyed CSR
            pool = None if b is None else ctx.smap.csr(*(SIDE_BEV.grad if mask is None else SIDE_BEV.fwd))
            dw, db = _wgrad(a, gy, b, pool, any(need[_PARAMS + n:]), mask)
            for i, (part, shape) in enumerate(zip(dw.split(list(sizes), dim=1), ctx.shapes)):
                if need[_PARAMS + i]:
                    dws[i] = part.reshape(shape).to(w.dtype)
            if db is not None:
                for i, part in enumerate(db.split(list(sizes))):
                    if need[_PARAMS + n + i]:
                        dbs[i] = part.contiguous()
        return (d_a, d_b) + (None,) * (_PARAMS - 2) + (*dws, *dbs)


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

    def _apply(self, a, b, smap, keep_prob=None, seed=None):
        """keep_prob None: the plain heads; else the heads under dropout, seed None drawing one."""
        _on_gpu(a, b)
        if keep_prob is not None:
            keep_prob = float(keep_prob)
            if not 0.0 < keep_prob <= 1.0:
                raise ValueError(f"keep_prob {keep_prob}: a probability in (0, 1]")
            if seed is None:  # torch's default CPU generator: torch.manual_seed governs it
                seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
            seed = int(seed)
        return tuple(_FusionHeadFn.apply(a, b, smap, self.heads, keep_prob, seed, *self.weights, *self.biases))

    def _check_map(self, fused_map):
        if int(fused_map.shape[-1]) != self.c_lidar + self.c_img:
            raise ValueError(f"fused map {tuple(fused_map.shape)} does not hold {self.c_lidar}+{self.c_img} channels")

    def _check_maps(self, lidar, img, smap):
        if int(lidar.shape[-1]) != self.c_lidar or int(img.shape[-1]) != self.c_img:
            raise ValueError(f"maps {tuple(lidar.shape)}, {tuple(img.shape)} do not hold {self.c_lidar} and "
                             f"{self.c_img} channels")
        if _rows(lidar) != smap.n_cells or _rows(img) != smap.n_pix:
            raise ValueError(f"maps of {_rows(lidar)} cells and {_rows(img)} pixels, the map {smap.n_cells} and "
                             f"{smap.n_pix}")

    def __call__(self, fused_map):
        """The heads of a materialised conv_lidar_fused [B, H, W, c_lidar + c_img]: one tensor per head."""
        self._check_map(fused_map)
        return self._apply(fused_map, None, None)

    def fused(self, lidar, img, smap, keep_prob=1.0):
        """(rpn_cls_score, rpn_bbox_pred, ...) of [lidar || sparse_pool(M, img)] without writing the pooled map
        or the concat; ``smap`` is the ShplMap of the frames of ``lidar``. Differentiable in lidar, img, every
        weight and every bias."""
        if keep_prob != 1.0:
            raise NotImplementedError(
                "FusionHead.fused applies the heads before the pooling, which needs the heads to be linear in the "
                "pooled map; a dropout mask over the concat (keep_prob < 1) is not. Use fused_dropout, or materialise "
                "the map: mv3d.sparse_pool, then the concat, dropout and 1x1 convs in torch")
        self._check_maps(lidar, img, smap)
        return self._apply(lidar, img, smap)

    def dropout(self, fused_map, keep_prob, seed=None):
        """The heads of dropout(conv_lidar_fused, keep_prob) over a materialised map [B, H, W, c_lidar + c_img], as
        MV3D trains them (MV3D_voxel_train.py:148-178 with use_dropout): the mask of include/shpl.h over
        (row, channel), computed in the kernels and again in the backward, never stored. seed: an integer, or
        None to draw one from torch's default CPU generator. Differentiable in the map, every weight and bias."""
        self._check_map(fused_map)
        return self._apply(fused_map, None, None, keep_prob, seed)

    def fused_dropout(self, lidar, img, smap, keep_prob, seed=None):
        """The heads of dropout([lidar || sparse_pool(M, img)], keep_prob) without writing the pooled map, the
        concat or a mask: the pooling runs inside the GEMM's operand staging and the mask is computed from
        (seed, row, channel). The same mask as ``dropout`` over the materialised map with the same seed.
        Differentiable in lidar, img, every weight and every bias."""
        self._check_maps(lidar, img, smap)
        return self._apply(lidar, img, smap, keep_prob, seed)
