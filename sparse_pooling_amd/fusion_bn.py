"""SHPL concat with BatchNorm on both halves, fused (shpl_concat_bn of include/shpl.h).

What ``sparse_pool_layer(..., use_bn=True)`` was meant to do (avod/avod/utils/sparse_pool_utils.py:69-70,
:84-85 through ``concat_bn_op`` :120-124): BatchNorm each half on its own -- slim defaults ``center=True``,
``scale=False``, ``eps`` 1e-3, ``decay`` 0.999, no activation -- then concatenate:

    bv_fused  = [BN(bev) || BN(img_pooled)]
    img_fused = [BN(img) || BN(bv_pooled)]        (dual)

The reference's own code dies there with ``TypeError`` (``slim.batch_norm`` has no ``training`` keyword), and
``sparse_pool_utils.sparse_pool_layer(use_bn=True)`` keeps reproducing that; the capability lives under the new
names of this module. The pooled map is never stored, forward or backward: its statistics are sums over the
occupied rows, every empty row's normalised pooled half is one per-channel constant, and its gradient is
written at the occupied rows only and pulled back by the existing pull of the other direction.
"""
from __future__ import annotations

import torch

from . import _lib as L

SIDES = ("bv", "img")  # bv: [BN(bev) || BN(pool(img))], cell-keyed; img: [BN(img) || BN(trans(bev))], pixel-keyed
_FWD = {"bv": (L.BY_CELL, L.ORDER_ENTRY), "img": (L.BY_PIXEL, L.ORDER_COL_ROW)}
_GRAD = {"bv": (L.BY_PIXEL, L.ORDER_COL_ENTRY), "img": (L.BY_CELL, L.ORDER_COL_ENTRY)}


def rows_csr(smap, direction, order):
    """smap's CSR of (direction, order) WITH key ranges, which the row-keyed kernels here need
    (ShplMap.csr(key_range=True): maps of fewer than 2^24 entries)."""
    return smap.csr(direction, order, key_range=True)


def _rows2d(t):
    """[.., C] contiguous -> (tensor, row stride)."""
    t = t if t.is_contiguous() else t.contiguous()
    return t, int(t.shape[-1])


def concat_bn_forward(smap, side, pass_, src, gamma, beta, moving_mean, moving_var, eps=1e-3, decay=0.999,
                      training=True, batch_mean=None, batch_var=None, save=None, ws=None, out=None):
    """shpl_concat_bn over smap: out [.., c_pass + c_pool] = [BN(pass_) || BN(pooled src)], side "bv" (pass_ the
    BEV map, src the image map) or "img" (the other way). gamma (None: 1), beta (None: 0), moving_mean,
    moving_var, batch_mean, batch_var: f32 [c_pass + c_pool], the pass-through half's first. Training updates
    the moving statistics in place. Returns (out, save): save [2, C] holds the mean and scale the backward
    takes."""
    direction, order = _FWD[side]
    csr = rows_csr(smap, direction, order)
    pass_, ps = _rows2d(pass_)
    src, ss = _rows2d(src)
    c_pass, c_pool = ps, ss
    c = c_pass + c_pool
    dev = pass_.device
    if out is None:
        out = torch.empty(tuple(pass_.shape[:-1]) + (c,), dtype=pass_.dtype, device=dev)
    if save is None:
        save = torch.empty((2, c), dtype=torch.float32, device=dev)
    nb = 0
    if training:
        nb = L.ws_bytes("shpl_concat_bn", csr.n_keys, c_pass, c_pool)
        if ws is None or ws.numel() < nb:
            ws = L.workspace(nb, dev)
    L.check(L.lib().shpl_concat_bn(direction, L.dtype_code(out), csr.ref(), L.ptr(src), ss, 0, c_pool, L.ptr(pass_),
                                   ps, 0, c_pass, L.ptr(out), c, int(bool(training)), float(eps), float(decay),
                                   L.ptr(gamma), L.ptr(beta), L.ptr(moving_mean), L.ptr(moving_var),
                                   L.ptr(batch_mean), L.ptr(batch_var), L.ptr(save), L.ptr(ws) if training else None,
                                   ws.numel() if training else 0, L.stream_of(dev)), "shpl_concat_bn")
    return out, save


def concat_bn_backward(smap, side, pass_, src, g, save, gamma=None, training=True, need_src=True, scratch=None,
                       ws=None):
    """shpl_concat_bn_backward: (g_pass, g_src or None, dbeta [C], dgamma [C]); g_src is f32 in both dtypes
    (summed from unrounded values; the caller rounds it once if it wants bf16). scratch: the pooled half's
    gradient map f32 [rows, c_pool], written and read at the occupied rows only and never cleared (any f32
    tensor of that many elements; a new one when None)."""
    direction, order = _FWD[side]
    csr = rows_csr(smap, direction, order)
    pass_, ps = _rows2d(pass_)
    src, ss = _rows2d(src)
    g, gs = _rows2d(g)
    c_pass, c_pool = ps, ss
    c = c_pass + c_pool
    dev = pass_.device
    g_pass = torch.empty_like(pass_)
    if scratch is None or scratch.numel() < csr.n_keys * c_pool or scratch.dtype != torch.float32:
        scratch = torch.empty(max(csr.n_keys * c_pool, 1), dtype=torch.float32, device=dev)
    g_src, csr_grad = None, None
    if need_src:
        csr_grad = smap.csr(*_GRAD[side])
        g_src = torch.empty(src.shape, dtype=torch.float32, device=dev)
    dbeta = torch.empty(c, dtype=torch.float32, device=dev)
    dgamma = torch.empty(c, dtype=torch.float32, device=dev)
    nb = L.ws_bytes("shpl_concat_bn_backward", csr.n_keys, c_pass, c_pool)
    if ws is None or ws.numel() < nb:
        ws = L.workspace(nb, dev)
    L.check(L.lib().shpl_concat_bn_backward(direction, L.dtype_code(g), csr.ref(),
                                            csr_grad.ref() if csr_grad is not None else None, L.ptr(src), ss, 0,
                                            c_pool, L.ptr(pass_), ps, 0, c_pass, L.ptr(g), gs, L.ptr(save),
                                            L.ptr(gamma), int(bool(training)), L.ptr(g_pass), c_pass, L.ptr(scratch),
                                            L.ptr(g_src), c_pool, L.ptr(dbeta), L.ptr(dgamma), L.ptr(ws), ws.numel(),
                                            L.stream_of(dev)), "shpl_concat_bn_backward")
    return g_pass, g_src, dbeta, dgamma


class _ConcatBNFn(torch.autograd.Function):
    """[BN(pass) || BN(pooled src)] with gradients to pass, src, beta and gamma."""

    @staticmethod
    def forward(ctx, pass_, src, beta, gamma, mod, smap, side, is_training):
        pass_, src = pass_.contiguous(), src.contiguous()
        p = mod.params[side]
        out, save = concat_bn_forward(smap, side, pass_, src, gamma, beta, p["moving_mean"], p["moving_var"],
                                      eps=mod.eps, decay=mod.decay, training=is_training,
                                      batch_mean=p["batch_mean"], batch_var=p["batch_var"],
                                      ws=mod._ws.get(("fwd", side)))
        ctx.save_for_backward(pass_, src, save, gamma if gamma is not None else torch.empty(0, device=pass_.device))
        ctx.mod, ctx.smap, ctx.side, ctx.training, ctx.has_gamma = mod, smap, side, is_training, gamma is not None
        return out

    @staticmethod
    def backward(ctx, g):
        pass_, src, save, gamma = ctx.saved_tensors
        gamma = gamma if ctx.has_gamma else None
        mod, side = ctx.mod, ctx.side
        g_pass, g_src, dbeta, dgamma = concat_bn_backward(ctx.smap, side, pass_, src, g.contiguous(), save, gamma,
                                                          training=ctx.training, need_src=ctx.needs_input_grad[1],
                                                          scratch=mod._scratch.get(side),
                                                          ws=mod._ws_for(("bwd", side), 0))
        if g_src is not None and g_src.dtype != src.dtype:
            g_src = g_src.to(src.dtype)  # the one rounding of the source's gradient
        return (g_pass if ctx.needs_input_grad[0] else None, g_src, dbeta if ctx.needs_input_grad[2] else None,
                dgamma if ctx.has_gamma and ctx.needs_input_grad[3] else None, None, None, None, None)


class FusionConcatBN:
    """The four BatchNorms of the SHPL concat under use_bn: (bev, img_pooled) of bv_fused and (img, bv_pooled)
    of img_fused. Per side one parameter vector over the fused channels, the pass-through half's first:
    ``beta_bv`` / ``beta_img`` (and ``gamma_bv`` / ``gamma_img`` with ``scale=True``), with the moving
    statistics in ``params[side]``; ``halves(side)`` gives the per-BatchNorm views.

    Limits. The map's CSRs carry key ranges, which hold fewer than 2^24 entries (``ShplMap.csr(key_range=True)``
    raises ``ValueError`` past that). A module keeps one workspace and one gradient scratch map per side, shared
    by every call and every outstanding autograd graph: calls and their backwards must run on ONE stream, in
    stream order (each kernel reads them only inside its own call)."""

    def __init__(self, c_bev, c_img, eps=1e-3, decay=0.999, scale=False, dtype=torch.float32, device="cuda"):
        self.c_bev, self.c_img = int(c_bev), int(c_img)
        self.eps, self.decay, self.scale = float(eps), float(decay), bool(scale)
        self.dtype, self.device = dtype, torch.device(device)
        c = self.c_bev + self.c_img
        f32 = dict(dtype=torch.float32, device=self.device)
        self.params = {}
        for side in SIDES:
            self.params[side] = {
                "beta": torch.zeros(c, **f32).requires_grad_(True),
                "gamma": torch.ones(c, **f32).requires_grad_(True) if self.scale else None,
                "moving_mean": torch.zeros(c, **f32), "moving_var": torch.ones(c, **f32),
                "batch_mean": torch.zeros(c, **f32), "batch_var": torch.zeros(c, **f32)}
        self._ws, self._scratch = {}, {}

    beta_bv = property(lambda self: self.params["bv"]["beta"])
    beta_img = property(lambda self: self.params["img"]["beta"])
    gamma_bv = property(lambda self: self.params["bv"]["gamma"])
    gamma_img = property(lambda self: self.params["img"]["gamma"])

    def halves(self, side, name="beta"):
        """(pass-through half's, pooled half's) views of one of the side's per-channel vectors."""
        v = self.params[side][name]
        c_pass = self.c_bev if side == "bv" else self.c_img
        return (None, None) if v is None else (v[:c_pass], v[c_pass:])

    def parameters(self):
        return [p[n] for p in self.params.values() for n in ("beta", "gamma") if p[n] is not None]

    def _ws_for(self, key, nbytes):
        ws = self._ws.get(key)
        if ws is None or ws.numel() < nbytes:
            ws = self._ws[key] = L.workspace(nbytes, self.device)
        return ws

    def _apply(self, side, pass_, src, smap, is_training):
        c_pass, c_pool = (self.c_bev, self.c_img) if side == "bv" else (self.c_img, self.c_bev)
        if pass_.shape[-1] != c_pass or src.shape[-1] != c_pool:
            raise ValueError(f"{side}_fused takes {c_pass} pass-through and {c_pool} pooled channels, got "
                             f"{pass_.shape[-1]} and {src.shape[-1]}")
        n_rows = smap.n_cells if side == "bv" else smap.n_pix
        if pass_.numel() // c_pass != n_rows:
            raise ValueError(f"{side}_fused: the map has {n_rows} destination rows, the pass-through input "
                             f"{pass_.numel() // c_pass}")
        if is_training:  # the inference forward takes no workspace
            self._ws_for(("fwd", side), L.ws_bytes("shpl_concat_bn", n_rows, c_pass, c_pool))
        if torch.is_grad_enabled() and any(t.requires_grad for t in (pass_, src, *self.parameters())):
            self._ws_for(("bwd", side), L.ws_bytes("shpl_concat_bn_backward", n_rows, c_pass, c_pool))
            s = self._scratch.get(side)
            if s is None or s.numel() < n_rows * c_pool:
                self._scratch[side] = torch.empty(n_rows * c_pool, dtype=torch.float32, device=pass_.device)
        p = self.params[side]
        return _ConcatBNFn.apply(pass_, src, p["beta"], p["gamma"], self, smap, side, bool(is_training))

    def fused(self, bev, img, smap, is_training=False):
        """bv_fused = [BN(bev) || BN(pool(img))]."""
        return self._apply("bv", bev, img, smap, is_training)

    def fused_img(self, img, bev, smap, is_training=False):
        """img_fused = [BN(img) || BN(trans(bev))]."""
        return self._apply("img", img, bev, smap, is_training)

    def __call__(self, bev, img, smap, dual=False, is_training=False):
        """The reference's (bv_fused, img_fused) pair; without dual the image map passes through."""
        bv_fused = self.fused(bev, img, smap, is_training)
        return bv_fused, (self.fused_img(img, bev, smap, is_training) if dual else img)
