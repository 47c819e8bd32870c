"""shpl_head1x1_drop, its gradients and shpl_dropout_mask reject bad arguments on the host, their workspace
queries are host-only, and at MV3D's shape the workspaces stay far below the pooled map's size (no GPU: fake
aligned device pointers are never dereferenced, as in test_head_abi.py)."""
import ctypes
import math

import pytest


@pytest.fixture(scope="module")
def lib():
    from sparse_pooling_amd import _lib as L
    return L.lib()


P = ctypes.c_void_p(256)  # a fake, aligned, non-null device pointer
N = None
WS = 1 << 30
BAD_KEEP = (0.0, -0.1, 1.5, math.nan, math.inf)


def _cell_csr(L, n_keys, cap=1000, key_range=True):
    return L.ShplCsr(256, 256, 256, None, n_keys, cap, 256 if key_range else None)


def _pixel_csr(L, n_keys, cap=1000, identity=False):
    c = L.ShplCsr(256, 256, 256, None if identity else 256, n_keys, cap, 256)
    c.flags = L.CSR_IDENTITY_COLS if identity else 0
    return c


def _ref(pool):
    return None if pool is None else ctypes.byref(pool)


def _fwd(lib, L, dtype=None, rows=120, a=P, c_a=64, b=P, c_b=32, rows_b=80, pool="cell", w=P, c_out=18, out=P,
         keep=0.5, ws=P, ws_bytes=WS):
    pool = _cell_csr(L, rows) if pool == "cell" else pool
    return lib.shpl_head1x1_drop(L.F32 if dtype is None else dtype, rows, a, c_a, 0, c_a, b, c_b, 0, c_b, rows_b,
                                 _ref(pool), w, c_out, N, out, c_out, keep, 7, ws, ws_bytes, N)


def _dgrad(lib, L, dtype=None, gy=P, c_out=18, w=P, da=P, db=P, rows_b=80, pool="pixel", keep=0.5, ws=P,
           ws_bytes=WS):
    pool = _pixel_csr(L, 80) if pool == "pixel" else pool
    return lib.shpl_head1x1_drop_dgrad(L.F32 if dtype is None else dtype, 120, gy, c_out, c_out, w, 64, 32, da, 64,
                                       db, 32, rows_b, _ref(pool), keep, 7, ws, ws_bytes, N)


def _wgrad(lib, L, dtype=None, a=P, b=P, gy=P, c_out=18, dw=P, rows_b=80, pool="cell", keep=0.5, ws=P,
           ws_bytes=WS):
    pool = _cell_csr(L, 120) if pool == "cell" else pool
    return lib.shpl_head1x1_drop_wgrad(L.F32 if dtype is None else dtype, 120, a, 64, 0, 64, b, 32, 0, 32, rows_b,
                                       _ref(pool), gy, c_out, c_out, dw, P, keep, 7, ws, ws_bytes, N)


def test_keep_prob_range(lib):
    from sparse_pooling_amd import _lib as L
    for kp in BAD_KEEP:
        assert _fwd(lib, L, keep=kp) == L.ERR_ARG, kp
        assert _dgrad(lib, L, keep=kp) == L.ERR_ARG, kp
        assert _wgrad(lib, L, keep=kp) == L.ERR_ARG, kp
        assert lib.shpl_dropout_mask(10, 16, kp, 7, P, N) == L.ERR_ARG, kp
    assert lib.shpl_dropout_mask(10, 16, 0.5, 7, N, N) == L.ERR_ARG
    assert lib.shpl_dropout_mask(-1, 16, 0.5, 7, P, N) == L.ERR_BAD_SHAPE
    assert lib.shpl_dropout_mask(10, 0, 0.5, 7, P, N) == L.ERR_BAD_SHAPE
    assert lib.shpl_dropout_mask(0, 16, 0.5, 7, P, N) == L.OK  # no rows: nothing launched


def test_forward_argument_checks(lib):
    from sparse_pooling_amd import _lib as L
    assert _fwd(lib, L, dtype=7) == L.ERR_ARG
    for c_out in (0, 33, -1):
        assert _fwd(lib, L, c_out=c_out) == L.ERR_BAD_SHAPE
    for kw in (dict(a=N), dict(b=N), dict(w=N), dict(out=N), dict(ws=N)):
        assert _fwd(lib, L, **kw) == L.ERR_ARG, kw
    # a pool whose n_keys is not the row count of a; a pixel-keyed pool (with ent_col, or flagged identity columns)
    assert _fwd(lib, L, pool=_cell_csr(L, 119)) == L.ERR_BAD_SHAPE
    assert _fwd(lib, L, pool=_pixel_csr(L, 120)) == L.ERR_ARG
    assert _fwd(lib, L, pool=_pixel_csr(L, 120, identity=True)) == L.ERR_ARG
    # a pool without a second source; a dense second source of another row count
    assert _fwd(lib, L, b=N, c_b=0) == L.ERR_BAD_SHAPE
    assert _fwd(lib, L, pool=None, rows_b=80) == L.ERR_BAD_SHAPE
    # a workspace that is too small, for the pooled, the two-map and the one-map form
    for kw in (dict(), dict(pool=None, rows_b=120), dict(pool=None, b=N, c_b=0, rows_b=0)):
        nb = ctypes.c_size_t()
        pooled = kw.get("pool", "cell") is not None
        assert lib.shpl_head1x1_drop_workspace_bytes(L.F32, 120, 64, kw.get("rows_b", 80), kw.get("c_b", 32), 18,
                                                     int(pooled), ctypes.byref(nb)) == L.OK
        assert nb.value > 0
        assert _fwd(lib, L, ws_bytes=nb.value - 1, **kw) == L.ERR_WORKSPACE
    # row strides narrower than the channels
    pool = _cell_csr(L, 120)
    assert lib.shpl_head1x1_drop(L.F32, 120, P, 63, 0, 64, P, 32, 0, 32, 80, ctypes.byref(pool), P, 18, N, P, 18,
                                 0.5, 7, P, WS, N) == L.ERR_BAD_SHAPE
    assert lib.shpl_head1x1_drop(L.F32, 120, P, 64, 0, 64, P, 32, 0, 32, 80, ctypes.byref(pool), P, 18, N, P, 17,
                                 0.5, 7, P, WS, N) == L.ERR_BAD_SHAPE


def test_gradient_argument_checks(lib):
    from sparse_pooling_amd import _lib as L
    for fn in (_dgrad, _wgrad):
        assert fn(lib, L, dtype=9) == L.ERR_ARG
        for c_out in (0, 33):
            assert fn(lib, L, c_out=c_out) == L.ERR_BAD_SHAPE
        assert fn(lib, L, gy=N) == L.ERR_ARG
        assert fn(lib, L, ws=N) == L.ERR_ARG
        assert fn(lib, L, pool=None, rows_b=80) == L.ERR_BAD_SHAPE  # a dense second source of another row count
    # the input gradient's list is keyed by pixel, the weight gradient's (the forward's) by cell
    assert _dgrad(lib, L, pool=_cell_csr(L, 120)) == L.ERR_ARG
    assert _dgrad(lib, L, pool=_cell_csr(L, 80)) == L.ERR_ARG
    assert _dgrad(lib, L, pool=_pixel_csr(L, 79)) == L.ERR_BAD_SHAPE
    assert _wgrad(lib, L, pool=_pixel_csr(L, 80)) == L.ERR_ARG
    assert _wgrad(lib, L, pool=_pixel_csr(L, 120, identity=True)) == L.ERR_ARG
    assert _wgrad(lib, L, pool=_cell_csr(L, 119)) == L.ERR_BAD_SHAPE
    assert _dgrad(lib, L, w=N) == L.ERR_ARG
    assert _dgrad(lib, L, da=N, db=N) == L.ERR_ARG
    for kw in (dict(a=N), dict(b=N), dict(dw=N)):
        assert _wgrad(lib, L, **kw) == L.ERR_ARG, kw
    nb = ctypes.c_size_t()
    assert lib.shpl_head1x1_drop_workspace_bytes(L.F32, 120, 64, 80, 32, 18, 1, ctypes.byref(nb)) == L.OK
    assert _dgrad(lib, L, ws_bytes=nb.value - 1) == L.ERR_WORKSPACE
    assert lib.shpl_head1x1_drop_wgrad_workspace_bytes(L.F32, 120, 64, 80, 32, 18, 1, ctypes.byref(nb)) == L.OK
    assert _wgrad(lib, L, ws_bytes=nb.value - 1) == L.ERR_WORKSPACE


def _q(fn, L, dtype, rows, c_a, rows_b, c_b, c_out, pooled):
    nb = ctypes.c_size_t()
    assert fn(dtype, rows, c_a, rows_b, c_b, c_out, pooled, ctypes.byref(nb)) == L.OK
    return nb.value


def test_workspace_queries_are_host_only_and_monotone(lib):
    from sparse_pooling_amd import _lib as L
    for fn in (lib.shpl_head1x1_drop_workspace_bytes, lib.shpl_head1x1_drop_wgrad_workspace_bytes):
        assert fn(L.F32, 10, 8, 10, 8, 0, 1, ctypes.byref(ctypes.c_size_t())) == L.ERR_BAD_SHAPE
        assert fn(L.F32, 10, 8, 10, 8, 33, 1, ctypes.byref(ctypes.c_size_t())) == L.ERR_BAD_SHAPE
        assert fn(5, 10, 8, 10, 8, 18, 1, ctypes.byref(ctypes.c_size_t())) == L.ERR_ARG
        assert fn(L.F32, 10, 8, 10, 8, 18, 1, None) == L.ERR_ARG
        for dtype in (L.F32, L.BF16):
            for pooled in (0, 1):
                base = (96000, 768, 61440, 768, 18)
                assert _q(fn, L, dtype, *base, pooled) > 0
                # every step grows one of rows, c_a, rows_b, c_b, c_out: never a smaller workspace
                sizes = [1, 63, 64, 65, 4095, 4096, 4097, 16385, 20000, 96000, 200000]
                for i, steps in enumerate((sizes, [1, 5, 768, 1536], sizes, [1, 6, 768, 1536], [1, 8, 9, 18, 32])):
                    last = 0
                    for v in steps:
                        args = list(base)
                        args[i] = v
                        cur = _q(fn, L, dtype, *args, pooled)
                        assert cur >= last, (fn, dtype, pooled, i, v)
                        last = cur


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_memory_rule_at_the_mv3d_shape(lib, dtype):
    """Neither workspace holds anything of the size of the pooled map: both are below an eighth of its bytes."""
    from sparse_pooling_amd import _lib as L
    dt, e = (L.F32, 4) if dtype == "f32" else (L.BF16, 2)
    rows, c_b = 96000, 768
    for fn in (lib.shpl_head1x1_drop_workspace_bytes, lib.shpl_head1x1_drop_wgrad_workspace_bytes):
        for pooled in (0, 1):
            nb = _q(fn, L, dt, rows, 768, 61440 if pooled else rows, c_b, 18, pooled)
            print(fn.__name__, dtype, pooled, nb)
            assert nb < rows * c_b * e // 8
