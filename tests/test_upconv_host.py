"""shpl_upconv3x3 on the host (no GPU): the ABI, its argument checks, the workspace query, the phase algebra
behind ``fusion_upconv.phase_weights``, and the shipped kernels' register metadata."""
import ctypes
import os
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

P = ctypes.c_void_p(256)  # a fake, aligned, non-null device pointer: never dereferenced
N = None
WS = 1 << 30


@pytest.fixture(scope="module")
def lib():
    from sparse_pooling_amd import _lib as L
    return L.lib()


def _csr(L, n_keys, cap=1000, pixel=False):
    return L.ShplCsr(256, 256, 256, 256 if pixel else None, n_keys, cap, None)


def _up(lib, L, dtype=None, n_frames=2, h=5, w=7, a=P, a_stride=16, a_off=0, c_a=16, b=P, b_stride=8, b_off=0,
        c_b=8, pool="cell", frame_off=P, wts=P, c_out=12, act=1, out=P, out_stride=12, stats=N, ws=P, ws_bytes=WS):
    pool = _csr(L, n_frames * h * w) if pool == "cell" else pool
    return lib.shpl_upconv3x3(L.F32 if dtype is None else dtype, n_frames, h, w, a, a_stride, a_off, c_a, b,
                              b_stride, b_off, c_b, None if pool is None else ctypes.byref(pool), frame_off, wts,
                              c_out, N, N, N, act, out, out_stride, stats, ws, ws_bytes, N)


def _conv(lib, L, dtype=None, n_frames=2, h=5, w=7, a=P, a_stride=16, a_off=0, c_a=16, b=P, b_stride=8, b_off=0,
          c_b=8, pool="cell", frame_off=P, wts=P, c_out=12, act=1, out=P, out_stride=12, stats=N, ws=P, ws_bytes=WS):
    pool = _csr(L, n_frames * h * w) if pool == "cell" else pool
    return lib.shpl_conv3x3(L.F32 if dtype is None else dtype, n_frames, h, w, a, a_stride, a_off, c_a, b,
                            b_stride, b_off, c_b, None if pool is None else ctypes.byref(pool), frame_off, wts,
                            c_out, N, N, N, act, out, out_stride, stats, ws, ws_bytes, N)


def test_symbols_are_declared_and_exported(lib):
    from sparse_pooling_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "shpl.h")).read()
    for name in ("shpl_upconv3x3", "shpl_upconv3x3_workspace_bytes"):
        assert f"int {name}(" in hdr
        assert hasattr(lib, name) and name in L.EXPORTED
    from sparse_pooling_amd import fusion_upconv as fu
    for name in ("upconv3x3", "upconv_ws_bytes", "phase_weights", "phase_weight_grad", "depth_to_space",
                 "space_to_depth", "FusionUpconv", "AfterVggFusion"):
        assert hasattr(fu, name)


# every bad call, by keyword: shpl_upconv3x3 must answer each exactly as shpl_conv3x3 does (same codes; where two
# defects meet, the same one wins -- the same order)
BAD = [
    (dict(dtype=7), "ERR_ARG"),
    (dict(c_out=0), "ERR_BAD_SHAPE"),
    (dict(h=-1), "ERR_BAD_SHAPE"),
    (dict(c_a=0, c_b=0, b=N, pool=None), "ERR_BAD_SHAPE"),
    (dict(act=2), "ERR_ARG"),
    (dict(wts=N), "ERR_ARG"),
    (dict(ws=N), "ERR_ARG"),
    (dict(ws_bytes=16), "ERR_WORKSPACE"),
    (dict(a_stride=15), "ERR_BAD_SHAPE"),
    (dict(out_stride=11), "ERR_BAD_SHAPE"),
    (dict(a_off=-1), "ERR_BAD_SHAPE"),
    (dict(b_stride=7), "ERR_BAD_SHAPE"),
    (dict(frame_off=N), "ERR_ARG"),                      # a pool without the frames' entry slots
    (dict(b=N), "ERR_ARG"),                              # ... without its source
    (dict(c_b=0), "ERR_ARG"),                            # ... without channels
    (dict(pool="short"), "ERR_BAD_SHAPE"),               # n_keys is not n_frames * h * w
    (dict(pool="noents"), "ERR_ARG"),
    (dict(pool=None, b=N), "ERR_ARG"),                   # a dense second source that is NULL
    (dict(out=N), "ERR_ARG"),
    (dict(a=N), "ERR_ARG"),
    # two defects at once: the earlier check wins
    (dict(dtype=7, c_out=0), "ERR_ARG"),
    (dict(act=2, ws_bytes=16), "ERR_ARG"),
    (dict(ws_bytes=16, a_stride=15), "ERR_WORKSPACE"),
    (dict(a_stride=15, out=N), "ERR_BAD_SHAPE"),
    (dict(wts=N, ws_bytes=16), "ERR_ARG"),
]


def _resolve(L, kw):
    kw = dict(kw)
    if kw.get("pool") == "short":
        kw["pool"] = _csr(L, 2 * 5 * 7 - 1)
    elif kw.get("pool") == "noents":
        c = _csr(L, 2 * 5 * 7)
        c.ent_src = None
        kw["pool"] = c
    return kw


def test_argument_checks_match_conv3x3(lib):
    from sparse_pooling_amd import _lib as L
    for kw, want in BAD:
        kw = _resolve(L, kw)
        got = _up(lib, L, **kw)
        assert got == getattr(L, want), (kw, got)
        assert got == _conv(lib, L, **kw), kw
    # the pixel-keyed pool and the empty call are accepted on the host: no pixel, nothing launched
    assert _up(lib, L, n_frames=0, pool=_csr(L, 0, pixel=True)) == L.OK
    assert _up(lib, L, h=0, pool=_csr(L, 0)) == L.OK
    # the output's 4 n_frames h w rows must index in 32 bits, where the input's alone would
    assert _up(lib, L, n_frames=1, h=1 << 15, w=(1 << 14) + 1, pool=None, b=N, c_b=0) == L.ERR_BAD_SHAPE
    nb = ctypes.c_size_t()
    assert lib.shpl_upconv3x3_workspace_bytes(L.F32, 2, 5, 7, 16, 8, 12, 1000, 1, ctypes.byref(nb)) == L.OK
    assert _up(lib, L, stats=P, ws_bytes=nb.value - 1) == L.ERR_WORKSPACE


def test_workspace_query(lib):
    from sparse_pooling_amd import _lib as L

    def q(dtype, n_frames, h, w, c_a, c_b, c_out, cap, stats):
        nb = ctypes.c_size_t()
        assert lib.shpl_upconv3x3_workspace_bytes(dtype, n_frames, h, w, c_a, c_b, c_out, cap, stats,
                                                  ctypes.byref(nb)) == L.OK
        return nb.value

    assert lib.shpl_upconv3x3_workspace_bytes(L.F32, 1, 5, 7, 16, 8, 12, -1, 0, None) == L.ERR_ARG
    assert lib.shpl_upconv3x3_workspace_bytes(9, 1, 5, 7, 16, 8, 12, -1, 0,
                                              ctypes.byref(ctypes.c_size_t())) == L.ERR_ARG
    assert lib.shpl_upconv3x3_workspace_bytes(L.F32, 1, 5, 7, 16, 8, 0, -1, 0,
                                              ctypes.byref(ctypes.c_size_t())) == L.ERR_BAD_SHAPE
    for dtype in (L.F32, L.BF16):
        for stats in (0, 1):
            last = 0
            for n_frames in (0, 1, 2, 3, 8, 9, 64):
                cur = q(dtype, n_frames, 88, 100, 256, 256, 128, 160000, stats)
                assert cur >= last and cur > 0
                last = cur
            last = 0
            for cap in (-1, 0, 1, 1000, 160000, 1 << 24):
                cur = q(dtype, 8, 88, 100, 256, 256, 128, cap, stats)
                assert cur >= last
                last = cur
    # the reference's BEV shape: the packed weights and the row pointers, nothing near a map's size
    assert q(L.BF16, 8, 88, 100, 256, 256, 128, 160000, 0) < 8 * 88 * 100 * 256 * 2 // 8
    # statistics partials: one per (tile, channel, statistic)
    assert q(L.F32, 8, 88, 100, 256, 256, 128, 160000, 1) > q(L.F32, 8, 88, 100, 256, 256, 128, 160000, 0)


# ------------------------------------------------------------------ the phase algebra, float64 on the CPU
def _definition(x, w):
    """out[f,oy,ox,co] = sum over (i,ky): 2i+ky = oy, (j,kx): 2j+kx = ox, ci of x[f,i,j,ci] W[ky,kx,co,ci]."""
    F, h, wd, ci = x.shape
    co = w.shape[2]
    out = np.zeros((F, 2 * h, 2 * wd, co))
    for i in range(h):
        for ky in range(3):
            oy = 2 * i + ky
            if oy >= 2 * h:
                continue
            for j in range(wd):
                for kx in range(3):
                    ox = 2 * j + kx
                    if ox >= 2 * wd:
                        continue
                    out[:, oy, ox, :] += x[:, i, j, :] @ w[ky, kx].T
    return out


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def test_phase_algebra_float64():
    from sparse_pooling_amd import fusion_upconv as fu
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 3, 5, 7))
    w = rng.standard_normal((3, 3, 5, 7))  # HWOI, 7 -> 5
    ref = _definition(x, w)
    xt, wt = torch.from_numpy(x), torch.from_numpy(w)
    tr = torch.nn.functional.conv_transpose2d(xt.permute(0, 3, 1, 2), wt.permute(3, 2, 0, 1), stride=2)
    tr = tr[..., :6, :10].permute(0, 2, 3, 1).numpy()
    assert _rel(tr, ref) <= 1e-12
    wp = fu.phase_weights(wt)
    assert tuple(wp.shape) == (3, 3, 7, 20)
    ph = torch.nn.functional.conv2d(xt.permute(0, 3, 1, 2), wp.permute(3, 2, 0, 1), padding=1).permute(0, 2, 3, 1)
    d2s = fu.depth_to_space(ph)
    assert tuple(d2s.shape) == (2, 6, 10, 5)
    assert _rel(d2s.numpy(), ref) <= 1e-12
    assert torch.equal(fu.space_to_depth(d2s), ph)
    # exactly 9 c_in c_out nonzeros for weights without zeros
    assert int((wp != 0).sum()) == 9 * 7 * 5 and not bool((wt == 0).any())


def test_phase_weight_grad_is_the_exact_adjoint():
    from sparse_pooling_amd import fusion_upconv as fu
    rng = np.random.default_rng(4)
    # small integers: both inner products are exact in float64
    w = torch.from_numpy(rng.integers(-8, 9, (3, 3, 5, 7)).astype(np.float64))
    d = torch.from_numpy(rng.integers(-8, 9, (3, 3, 7, 20)).astype(np.float64))
    lhs = float((fu.phase_weights(w) * d).sum())
    rhs = float((w * fu.phase_weight_grad(d)).sum())
    assert lhs == rhs
    assert torch.equal(fu.phase_weight_grad(fu.phase_weights(w)), w)


# ------------------------------------------------------------------ the shipped kernels' metadata
def test_upconv_kernels_report_no_scratch_and_no_spills():
    import test_isa_guard as guard
    so = os.path.join(ROOT, "sparse_pooling_amd", "libshpl.so")
    if not os.path.exists(so):
        from sparse_pooling_amd import build
        build.build()
    if not os.path.exists(os.path.join(guard.LLVM, "llvm-readelf")):
        pytest.skip("no ROCm LLVM tools")
    seen = {}
    with tempfile.TemporaryDirectory() as td:
        for n, co in enumerate(guard.library_code_objects(so)):
            path = os.path.join(td, f"co{n}.o")
            open(path, "wb").write(co)
            for name, md in guard.kernel_metadata(path).items():
                if "k_upconv" in name:
                    seen[name] = md
    # f32 and bf16, each: dense and pooled (plain, grouped), with and without statistics
    assert len(seen) >= 12, sorted(seen)
    assert any("k_upconv3x3If" in k for k in seen) and any("k_upconv3x3It" in k for k in seen)
    for name, md in seen.items():
        assert int(md["private_segment_fixed_size"]) == 0, (name, md)
        assert int(md["vgpr_spill_count"]) == 0, (name, md)
        assert int(md["sgpr_spill_count"]) == 0, (name, md)
