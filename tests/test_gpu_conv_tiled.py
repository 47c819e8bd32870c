"""The tiled conv kernels (k_conv3x3, k_conv3x3_wgrad, k_wgrad_bf16 of shpl_conv.hip) and the wide form's pooled
operand (wide::prep), pinned in every dispatch form on MI355X.

Every case makes three assertions: the result is within the existing bound of the CPU oracle (the tolerances
of tests/test_gpu_conv.py and tests/test_gpu_conv_grad.py, imported, not re-derived); the bitwise identities the
project states hold where they apply (fused over a CSR == the conv of the materialised map; a two-map input
gradient == the one map, split; two dense sources on a chunk boundary == their concatenation); and the SHA-256
of the output's bytes equals the value recorded in tests/golden/conv_tiled_bits.json
(tests/golden/make_conv_tiled_bits.py, which runs these same case functions).

Each case takes the tiled kernel: f32 always does; a bf16 case asserts ``not fc.rows_form(...)`` where that
function applies (the forward) and has a c_out that is no multiple of 256 (the wide form needs whole 256-channel
output blocks). The comment on each case names the kernel and template arguments it reaches.

Pooled cases read a hand-made dense correspondence (dense_map): every target cell of rows 0-8 of a 2 x 10 x 40
map holds 1 to 6 entries, so a halo row's range holds more than 64 entries (find_runs' second ballot round), a
tile more than 256 (several scan rounds, a run opening in one and closing in the next), and runs exceed
POOL_BATCH. Those properties are asserted on the CPU when the map is made.
"""
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import grouped_map as gm
from oracle import shpl_oracle as orc
from sparse_pooling_amd import synth
from test_gpu_conv import ACC, DEV, TOL, _assert_within, _bf16, _bound, _np, _t, _weights
from test_gpu_conv_grad import ACC_W, _check

pytestmark = pytest.mark.gpu

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_tiled_bits.json")
TH, TW, POOL_BATCH, SCAN = 8, 32, 4, 256  # shpl_conv.hip: output tile, entries per load batch, scan width
MAP_FRAMES, MAP_HW, SRC_HW = 2, (10, 40), (6, 7)


def _rd(a):
    return orc.from_bf16_bits(orc.to_bf16_bits(a))


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from sparse_pooling_amd import _lib as L
    L.lib()
    assert torch.cuda.is_available()


# ------------------------------------------------------------------ the dense map (no GPU)
def tile_runs(counts, f, y0, x0):
    """Run lengths of the halo of output tile (f, y0, x0) in find_runs' order: halo rows, cells inside."""
    H, W = counts.shape[1:]
    out = []
    for y in range(y0 - 1, y0 + TH + 1):
        if 0 <= y < H:
            out += [int(c) for c in counts[f, y, max(x0 - 1, 0):min(x0 + TW + 1, W)] if c]
    return out


@functools.lru_cache(maxsize=None)
def dense_map(swapped=False, seed=7):
    """A seeded two-frame correspondence in the reference format. Target map 2 x 10 x 40, source map 2 x 6 x 7;
    every target cell of rows 0-8 holds 1..6 entries (each count occurs), row 9 none; values in [-2, 2).
    swapped False: M's rows are the target cells, one column per entry on a source pixel (cell-keyed use: a plain
    sum per cell). True: M's rows are the source cells and a target pixel's n entries lie in 1..n columns on
    that pixel (pixel-keyed use with ent_col: per-column partials). Entries are grouped by frame, shuffled inside."""
    rng = np.random.default_rng(seed)
    F, (H, W), (hs, ws) = MAP_FRAMES, MAP_HW, SRC_HW
    counts = rng.integers(1, 7, (F, H, W))
    counts[:, H - 1] = 0
    assert set(np.unique(counts[:, :H - 1])) == {1, 2, 3, 4, 5, 6}
    # a 34-cell halo row range (tile column 0: cells [-1, 33)) with more than 64 entries
    assert (counts[:, :, :TW + 1].sum(-1) > 64).any()
    # a tile with more than 256 entries and a run across a scan round's end
    runs = tile_runs(counts, 0, 0, 0)
    ends = set(np.cumsum(runs).tolist())
    assert sum(runs) > SCAN and any(b not in ends for b in range(SCAN, sum(runs), SCAN))
    assert counts.max() > POOL_BATCH
    n_src = hs * ws
    rows, cols, col_pix, n_frame = [], [], [], []
    for f in range(F):
        r_f, c_f = [], []
        for t in range(H * W):
            n = int(counts[f].reshape(-1)[t])
            if n == 0:
                continue
            src = rng.choice(n_src, n, replace=False) + f * n_src
            m = int(rng.integers(1, n + 1)) if swapped else n  # columns of this target
            c_f += [len(col_pix) + i % m for i in range(n)]
            r_f += [int(s) for s in src] if swapped else [f * H * W + t] * n
            col_pix += [f * H * W + t] * m if swapped else [int(s) for s in src]
        order = rng.permutation(len(r_f))
        rows += [r_f[i] for i in order]
        cols += [c_f[i] for i in order]
        n_frame.append(len(r_f))
    col_pix = np.asarray(col_pix, np.int64)
    ih, iw = (H, W) if swapped else (hs, ws)
    idx = np.stack([col_pix // (ih * iw), col_pix % (ih * iw) // iw, col_pix % iw], 1)
    mij = np.stack([np.asarray(rows, np.int64), np.asarray(cols, np.int64)], 1)
    mval = rng.uniform(-2, 2, len(mij)).astype(np.float32)
    return {"mij": np.ascontiguousarray(mij), "mval": mval, "idx": np.ascontiguousarray(idx), "counts": counts,
            "m_size": np.array([F * (n_src if swapped else H * W), len(col_pix)], np.int64),
            "img_shape": (F, ih, iw), "n_frame": n_frame}


def _smap(m):
    """The device map of dense_map(): packed as one frame, then its entry slots cut by frame."""
    from sparse_pooling_amd import shpl_map as sm
    p = sm.pack_map(_t(m["mij"]), _t(m["mval"]), m["m_size"], _t(m["idx"]), m["img_shape"])
    off = torch.tensor(np.concatenate([[0], np.cumsum(m["n_frame"])]), dtype=torch.int64, device=DEV)
    return sm.ShplMap(p.cell, p.col, p.val, p.pix, p.nnz_cap, p.n_cells, p.n_pix, p.n_cols, DEV, frame_off=off,
                      n_frames=MAP_FRAMES, err=p.err)


def _pooled(key, which, ca, cb, bf):
    """Inputs of a pooled case: (a, b device tensors, pool CSR, frame_off, materialised [a || pooled] device map,
    the oracle's [a || pooled] f32). key "cell": the cell-keyed CSR (a the target map, b the source map);
    "pixel": the pixel-keyed CSR with ent_col (a the image, b the BEV map); which: "dense" (dense_map) or
    "planted" (tests/grouped_map.py, pixel-keyed only)."""
    from sparse_pooling_amd import _lib as L, shpl_map as sm
    dev = _bf16 if bf else _t
    F, (H, W), (hs, ws) = MAP_FRAMES, MAP_HW, SRC_HW
    if which == "planted":
        m = gm.make()
        a, b = gm.features(ca, cb)
        smap = sm.pack_map(_t(m["mij"]), _t(m["mval"]), m["m_size"], _t(m["idx"]), a.shape)
    else:
        m = dense_map(key == "pixel")
        a = synth.make_features((F, H, W, ca), 101)
        b = synth.make_features((F, hs, ws, cb), 102)
        if bf:
            a, b = _rd(a), _rd(b)
        smap = _smap(m)
    ta, tb = dev(a), dev(b)
    if key == "cell":
        pool = smap.csr(L.BY_CELL, L.ORDER_ENTRY)
        mat = sm.pool_img_to_bev(smap, tb, ta.shape, bev=ta)
        ref, _ = orc.sparse_pool_layer(a.reshape(1, -1, W, ca), b, m["mij"], m["mval"], m["m_size"], m["idx"])
    else:
        pool = smap.csr(L.BY_PIXEL, L.ORDER_COL_ROW)
        assert pool.ent_col is not None
        mat = sm.pool_bev_to_img(smap, tb, ta.shape, img=ta)
        _, ref = orc.sparse_pool_layer(b.reshape(1, -1, b.shape[2], cb), a, m["mij"], m["mval"], m["m_size"],
                                       m["idx"], dual=True)
    ref = ref.reshape(a.shape[:3] + (ca + cb,))
    if bf:
        ref = _rd(ref)
    torch.cuda.synchronize()
    assert smap.error_bits() == 0
    np.testing.assert_array_equal(_np(mat.float()), ref)
    return ta, tb, pool, smap.frame_off, mat, ref


# ------------------------------------------------------------------ forward helpers
def _epilogue(cout, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(cout).astype(np.float32), rng.uniform(0.5, 2.0, cout).astype(np.float32),
            rng.standard_normal(cout).astype(np.float32))


def _conv(ta, tw, tb=None, pool=None, foff=None, epi=None, stats=False, out=None):
    """conv3x3 with the BatchNorm-inference epilogue + ReLU (epi) or raw with statistics; bf16: not the row form."""
    from sparse_pooling_amd import fusion_conv as fc
    kw = {} if epi is None else dict(center=_t(epi[0]), scale=_t(epi[1]), shift=_t(epi[2]))
    st = torch.empty((2, int(tw.shape[3])), dtype=torch.float64, device=DEV) if stats else None
    if ta.dtype == torch.bfloat16:
        assert int(tw.shape[3]) % 256 != 0
        assert not fc.rows_form(ta, tw, b=tb, pool=pool, frame_off=foff, relu=epi is not None, stats=stats, out=out)
    y = fc.conv3x3(ta, tw, b=tb, pool=pool, frame_off=foff, relu=epi is not None, stats=st, out=out, **kw)
    return y, st


def _vs_oracle(y, st, x, w, epi, bf):
    """The conv bound of test_gpu_conv.py (bf16: + the store term 2^-8 |ref|); statistics as
    test_bf16_rows_conv_stats holds them."""
    center, scale, shift = epi if epi is not None else (None, None, None)
    ref, raw = orc.conv3x3(x, w, center, scale, shift, epi is not None, raw=True)
    bound = _bound(x, w, scale)
    _assert_within(y.float(), ref, bound + np.abs(ref) * 2.0 ** -8 if bf else bound)
    if st is not None:
        cout = w.shape[3]
        r2, b2, s = raw.reshape(-1, cout), bound.reshape(-1, cout), _np(st)
        _assert_within(s[0], r2.sum(0), b2.sum(0) + 1e-5 * np.abs(r2).sum(0))
        _assert_within(s[1], (r2 * r2).sum(0), (2.0 * np.abs(r2) * b2 + b2 * b2).sum(0) + 1e-5 * (r2 * r2).sum(0))


def _outs(y, st=None):
    return {"y": y} if st is None else {"y": y, "stats": st}


def case_dense(bf, shape, stats=False):
    B, H, W, cin, cout = shape
    dev = _bf16 if bf else _t
    x = synth.make_features((B, H, W, cin), 3) + (0.25 if stats else 0.0)
    w = _weights(cin, cout, 4)
    if bf:
        x, w = _rd(x), _rd(w)
    epi = None if stats else _epilogue(cout, 5)
    y, st = _conv(dev(x), dev(w), epi=epi, stats=stats)
    _vs_oracle(y, st, x, w, epi, bf)
    return _outs(y, st)


def case_two_sources_bf16():
    a = _rd(synth.make_features((2, 12, 40, 48), 6))
    b = _rd(synth.make_features((2, 12, 40, 32), 7))
    w = _rd(_weights(80, 32, 8))
    epi = _epilogue(32, 9)
    y2, _ = _conv(_bf16(a), _bf16(w), tb=_bf16(b), epi=epi)
    x = np.concatenate([a, b], -1)
    y1, _ = _conv(_bf16(x), _bf16(w), epi=epi)
    assert torch.equal(y2, y1)  # 48 channels end on a 16-channel chunk
    _vs_oracle(y2, None, x, w, epi, True)
    return {"y": y2}


def case_offset_out_bf16():
    B, H, W, cin, cout = 2, 16, 40, 32, 32
    x = _rd(synth.make_features((B, H, W, cin), 11))
    w = _rd(_weights(cin, cout, 12))
    epi = _epilogue(cout, 13)
    n = B * H * W * cout
    flat = torch.empty(n + 16, dtype=torch.bfloat16, device=DEV)
    o = flat[1:1 + n].view(B, H, W, cout)  # 2 bytes off 16-byte alignment
    y, _ = _conv(_bf16(x), _bf16(w), epi=epi, out=o)
    _vs_oracle(y, None, x, w, epi, True)
    return {"y": y}


def case_dgrad(bf, shape, splits):
    from sparse_pooling_amd import fusion_conv as fc
    B, H, W, cg, cdx = shape
    dev = _bf16 if bf else _t
    g = synth.make_features((B, H, W, cg), 21)
    w = _weights(cdx, cg, 22)
    if bf:
        g, w = _rd(g), _rd(w)
    dx = fc.conv3x3_dgrad(dev(g), dev(w), cdx)
    ref = orc.conv3x3_dgrad(g, w)
    wt = np.ascontiguousarray(w[::-1, ::-1].transpose(0, 1, 3, 2))
    _, ab = orc.conv3x3(np.abs(g), np.abs(wt), raw=True)
    _check(dx.float(), ref, TOL + ACC * ab + (2.0 ** -8 * np.abs(ref) if bf else 0.0), "dx")
    outs = {"dx": dx}
    for c in splits:
        da, db = fc.conv3x3_dgrad(dev(g), dev(w), cdx, split=c)
        assert da.shape[-1] == c and db.shape[-1] == cdx - c
        assert torch.equal(torch.cat([da, db], -1), dx), c
        outs["da%d" % c], outs["db%d" % c] = da, db
    return outs


def case_pooled(key, which, bf, ca, cb, cout, stats):
    ta, tb, pool, foff, mat, x = _pooled(key, which, ca, cb, bf)
    w = _weights(ca + cb, cout, 31)
    if bf:
        w = _rd(w)
    tw = (_bf16 if bf else _t)(w)
    epi = None if stats else _epilogue(cout, 32)
    y, st = _conv(ta, tw, tb=tb, pool=pool, foff=foff, epi=epi, stats=stats)
    # the conv of the materialised map, as two sources (A's channels need not end on a chunk)
    yu, su = _conv(mat[..., :ca].contiguous(), tw, tb=mat[..., ca:].contiguous(), epi=epi, stats=stats)
    assert torch.equal(y, yu)
    if stats:
        assert torch.equal(st, su)
    _vs_oracle(y, st, x, w, epi, bf)
    return _outs(y, st)


# ------------------------------------------------------------------ weight gradient
def _wgrad_vs_oracle(dw, x, g):
    _check(dw, orc.conv3x3_wgrad(x, g), TOL + ACC_W * orc.conv3x3_wgrad(np.abs(x), np.abs(g)), "dw")


def case_wgrad(bf, shape, ca=None):
    """Dense; ca: the channels of the first of two sources (0: B only)."""
    from sparse_pooling_amd import fusion_conv as fc
    B, H, W, cin, cout = shape
    dev = _bf16 if bf else _t
    x = synth.make_features((B, H, W, cin), 41)
    g = synth.make_features((B, H, W, cout), 42)
    if bf:
        x, g = _rd(x), _rd(g)
    if ca is None:
        dw = fc.conv3x3_wgrad(dev(x), dev(g))
    else:
        dw = fc.conv3x3_wgrad(dev(np.ascontiguousarray(x[..., :ca])), dev(g), b=dev(np.ascontiguousarray(x[..., ca:])))
    _wgrad_vs_oracle(dw, x, g)
    return {"dw": dw}


def case_wgrad_pooled(key, bf, ca, cb, cout):
    from sparse_pooling_amd import fusion_conv as fc
    ta, tb, pool, foff, mat, x = _pooled(key, "dense", ca, cb, bf)
    g = synth.make_features(x.shape[:3] + (cout,), 43)
    if bf:
        g = _rd(g)
    dw = fc.conv3x3_wgrad(ta, (_bf16 if bf else _t)(g), b=tb, pool=pool, frame_off=foff)
    _wgrad_vs_oracle(dw, x, g)
    return {"dw": dw}


# ------------------------------------------------------------------ the wide form's pooled operand
def case_wide_prep(key):
    from sparse_pooling_amd import fusion_conv as fc
    ca = cb = 64
    cout = 256
    ta, tb, pool, foff, mat, x = _pooled(key, "dense", ca, cb, True)
    w = _rd(_weights(ca + cb, cout, 51))
    tw = _bf16(w)
    bias = np.random.default_rng(52).standard_normal(cout).astype(np.float32) * 0.5
    assert not fc.rows_form(ta, tw, b=tb, pool=pool, frame_off=foff, relu=True)
    assert fc.wide_form(ta, tw, b=tb, pool=pool, frame_off=foff, relu=True) == 2  # over the compact pooled runs
    assert fc.wide_form(mat[..., :ca].contiguous(), tw, b=mat[..., ca:].contiguous(), relu=True) == 1
    y = fc.conv3x3(ta, tw, b=tb, pool=pool, frame_off=foff, shift=_t(bias), relu=True)
    yu = fc.conv3x3(mat[..., :ca].contiguous(), tw, b=mat[..., ca:].contiguous(), shift=_t(bias), relu=True)
    assert torch.equal(y, yu)
    ref = orc.conv3x3(x, w, None, None, bias, True)
    _assert_within(y.float(), ref, _bound(x, w) + np.abs(ref) * 2.0 ** -8)
    return {"y": y}


CASES = {
    # k_conv3x3<T, false, false, 1>: partial tiles, channel tails in input and output, masked staging,
    # channel-by-channel stores (bf16: 10 channels are no multiple of 8, so not k_conv_rows)
    "dense-9x33-10-5-f32": (case_dense, (False, (1, 9, 33, 10, 5))),
    "dense-9x33-10-5-bf16": (case_dense, (True, (1, 9, 33, 10, 5))),
    # k_conv3x3<float, false, false, 1>: whole pieces by LDS-DMA, 16-byte stores
    "dense-16x64-64-32-f32": (case_dense, (False, (2, 16, 64, 64, 32))),
    # k_conv3x3<uint16_t, false, false, 1>: 3 + 2 chunks keep it off k_conv_rows; the bf16 MFMA arm, DMA staging
    "dense-48+32-32-bf16": (case_two_sources_bf16, ()),
    # k_conv3x3<uint16_t, false, false, 1>: the output view 2 bytes off alignment, slow stores
    "dense-offset-out-bf16": (case_offset_out_bf16, ()),
    # k_conv3x3<float, false, false, 1>: the smallest case
    "dense-1x1-8-1-f32": (case_dense, (False, (1, 1, 1, 8, 1))),
    # k_conv3x3<float, false, false, 2>: two output blocks per workgroup (NCB = 2), the largest map
    "dense-17x70-24-64-f32": (case_dense, (False, (3, 17, 70, 24, 64))),
    # k_conv3x3<float, false, false, 2> with transposed packing: out2 through the fast epilogue (splits 32, 24)
    # and the slow one (21)
    "dgrad-64-from-24-f32": (case_dgrad, (False, (2, 9, 35, 24, 64), (32, 24, 21))),
    # k_conv3x3<uint16_t, false, false, 1>, transposed packing: 12 gradient channels keep the one-map form off
    # k_conv_rows too, so the split at 21 is bitwise the one map
    "dgrad-64-from-12-bf16": (case_dgrad, (True, (2, 9, 35, 12, 64), (21,))),
    # k_conv3x3<T, false, true, 1>: STATS, a partial output block (40), an edge tile whose rows past H = 19 must
    # not count (bf16: 20 channels, so not k_conv_rows)
    "stats-19x37-20-40-f32": (case_dense, (False, (2, 19, 37, 20, 40), True)),
    "stats-19x37-20-32-f32": (case_dense, (False, (2, 19, 37, 20, 32), True)),
    "stats-19x37-20-40-bf16": (case_dense, (True, (2, 19, 37, 20, 40), True)),
    "stats-19x37-20-32-bf16": (case_dense, (True, (2, 19, 37, 20, 32), True)),
    # k_wgrad, dense f32: k_conv3x3_wgrad<float, false>
    "wgrad-16x64-32-32-f32": (case_wgrad, (False, (1, 16, 64, 32, 32))),     # whole: LDS-DMA staging
    "wgrad-9x35-5-7-f32": (case_wgrad, (False, (2, 9, 35, 5, 7))),           # masked staging
    "wgrad-9x35-40-7-f32": (case_wgrad, (False, (2, 9, 35, 40, 7))),         # two input blocks, chunks q >= Q
    "wgrad-9x35-0+12-7-f32": (case_wgrad, (False, (2, 9, 35, 12, 7), 0)),    # B only: c_a = 0
    # 2 x 17 x 34 = 1156 tiles > 1024 groups: two tiles per group
    "wgrad-136x1080-5-7-f32": (case_wgrad, (False, (2, 136, 1080, 5, 7))),
    # k_wgrad_bf16: 16 + 16 (c_a % 32 != 0 keeps it off k_wgrad_rows) whole; 12 -> 7 masked
    "wgrad-16x64-16+16-32-bf16": (case_wgrad, (True, (1, 16, 64, 32, 32), 16)),
    "wgrad-9x35-12-7-bf16": (case_wgrad, (True, (2, 9, 35, 12, 7))),
    # wide::prep (k_occ_frame + k_pool_runs_wide_k<GROUP, 4>) under k_conv_wide: runs of 1..6 entries start at
    # every offset inside a group of K = 4 and walk on past it
    "wide-prep-cell": (case_wide_prep, ("cell",)),
    "wide-prep-pixel": (case_wide_prep, ("pixel",)),
}
# Pooled forward, k_conv3x3<T, true, STATS, 1, GROUP>: cell-keyed (GROUP false) and pixel-keyed with ent_col (GROUP
# true) over the dense map, and over the planted map of tests/grouped_map.py (the per-column order). bf16 12 + 12
# (no multiple of 8) never takes k_conv_rows; 32 + 16 does without statistics, so it is pinned with them only
# (2 + 1 chunks: the tiled case of test_wgrad_reuse_rejects_a_tiled_forward_workspace).
for _key, _which in (("cell", "dense"), ("pixel", "dense"), ("pixel", "planted")):
    for _bf, _ca, _cb, _co, _stats in ((False, 5, 6, 7, (False, True)), (False, 16, 24, 32, (False, True)),
                                       (True, 12, 12, 32, (False, True)), (True, 32, 16, 32, (True,))):
        for _st in _stats:
            CASES["pooled-%s-%s-%d+%d-%d-%s%s" % (_key, _which, _ca, _cb, _co, "bf16" if _bf else "f32",
                                                  "-stats" if _st else "")] = (
                case_pooled, (_key, _which, _bf, _ca, _cb, _co, _st))
# Pooled weight gradient, k_conv3x3_wgrad<T, true, GROUP> (bf16: a pooled call with c_a % 32 != 0 stays tiled)
for _key in ("cell", "pixel"):
    CASES["wgrad-pooled-%s-16+24-32-f32" % _key] = (case_wgrad_pooled, (_key, False, 16, 24, 32))
    CASES["wgrad-pooled-%s-5+6-7-f32" % _key] = (case_wgrad_pooled, (_key, False, 5, 6, 7))
    CASES["wgrad-pooled-%s-16+16-32-bf16" % _key] = (case_wgrad_pooled, (_key, True, 16, 16, 32))


def digest(t):
    """SHA-256 of a tensor's bytes."""
    t = t.detach().contiguous()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def run_case(name):
    """{output name: digest} of a case, after its oracle and identity assertions."""
    fn, args = CASES[name]
    outs = fn(*args)
    torch.cuda.synchronize()
    return {k: digest(v) for k, v in outs.items()}


@functools.lru_cache(maxsize=None)
def _table():
    with open(TABLE) as fh:
        return json.load(fh)


def test_table_lists_every_case():
    assert sorted(_table()) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_tiled_case(name):
    assert run_case(name) == _table()[name]
