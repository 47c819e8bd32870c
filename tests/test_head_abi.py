"""shpl_head1x1 and its gradients reject bad arguments on the host, and their workspace queries are host-only
(no GPU: fake aligned device pointers are never dereferenced, as in test_abi.test_argument_validation_is_host_side)."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from sparse_pooling_amd import _lib as L
    return L.lib()


P = ctypes.c_void_p(256)  # a fake, aligned, non-null device pointer
N = None
WS = 1 << 30


def _cell_csr(L, n_keys, cap=1000, key_range=True):
    return L.ShplCsr(256, 256, 256, None, n_keys, cap, 256 if key_range else None)


def _pixel_csr(L, n_keys, cap=1000, identity=False):
    c = L.ShplCsr(256, 256, 256, None if identity else 256, n_keys, cap, 256)
    c.flags = L.CSR_IDENTITY_COLS if identity else 0
    return c


def _fwd(lib, L, dtype=None, rows=120, a=P, c_a=64, b=P, c_b=32, rows_b=80, pool="cell", w=P, c_out=18, out=P,
         ws=P, ws_bytes=WS):
    pool = _cell_csr(L, rows) if pool == "cell" else pool
    return lib.shpl_head1x1(L.F32 if dtype is None else dtype, rows, a, c_a, 0, c_a, b, c_b, 0, c_b, rows_b,
                            None if pool is None else ctypes.byref(pool), w, c_out, N, out, c_out, ws, ws_bytes, N)


def test_forward_argument_checks(lib):
    from sparse_pooling_amd import _lib as L
    assert _fwd(lib, L, dtype=7) == L.ERR_ARG
    for c_out in (0, 33, -1):
        assert _fwd(lib, L, c_out=c_out) == L.ERR_BAD_SHAPE
    # null maps, weights, output, workspace
    assert _fwd(lib, L, a=N) == L.ERR_ARG
    assert _fwd(lib, L, b=N) == L.ERR_ARG
    assert _fwd(lib, L, w=N) == L.ERR_ARG
    assert _fwd(lib, L, out=N) == L.ERR_ARG
    assert _fwd(lib, L, ws=N) == L.ERR_ARG
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
        assert lib.shpl_head1x1_workspace_bytes(L.F32, 120, 64, kw.get("rows_b", 80), kw.get("c_b", 32), 18,
                                                int(pooled), ctypes.byref(nb)) == L.OK
        assert nb.value > 0
        assert _fwd(lib, L, ws_bytes=nb.value - 1, **kw) == L.ERR_WORKSPACE
    # row strides narrower than the channels
    pool = _cell_csr(L, 120)
    assert lib.shpl_head1x1(L.F32, 120, P, 63, 0, 64, P, 32, 0, 32, 80, ctypes.byref(pool), P, 18, N, P, 18, P, WS,
                            N) == L.ERR_BAD_SHAPE
    assert lib.shpl_head1x1(L.F32, 120, P, 64, 0, 64, P, 32, 0, 32, 80, ctypes.byref(pool), P, 18, N, P, 17, P, WS,
                            N) == L.ERR_BAD_SHAPE


def test_gradient_argument_checks(lib):
    from sparse_pooling_amd import _lib as L
    pix = _pixel_csr(L, 80)
    cell = _cell_csr(L, 120)

    def dgrad(dtype=L.F32, gy=P, c_out=18, w=P, da=P, db=P, rows_b=80, pool=pix, ws=P, ws_bytes=WS):
        return lib.shpl_head1x1_dgrad(dtype, 120, gy, c_out, c_out, w, 64, 32, da, 64, db, 32, rows_b,
                                      None if pool is None else ctypes.byref(pool), ws, ws_bytes, N)

    def wgrad(dtype=L.F32, a=P, b=P, gy=P, c_out=18, dw=P, rows_b=80, pool=pix, ws=P, ws_bytes=WS):
        return lib.shpl_head1x1_wgrad(dtype, 120, a, 64, 0, 64, b, 32, 0, 32, rows_b,
                                      None if pool is None else ctypes.byref(pool), gy, c_out, c_out, dw, P, ws,
                                      ws_bytes, N)

    for fn in (dgrad, wgrad):
        assert fn(dtype=9) == L.ERR_ARG
        for c_out in (0, 33):
            assert fn(c_out=c_out) == L.ERR_BAD_SHAPE
        assert fn(gy=N) == L.ERR_ARG
        assert fn(ws=N) == L.ERR_ARG
        assert fn(pool=cell) == L.ERR_ARG                        # the gradient's list is keyed by pixel
        assert fn(pool=_pixel_csr(L, 79)) == L.ERR_BAD_SHAPE     # n_keys is not the pixel count
        assert fn(pool=None, rows_b=80) == L.ERR_BAD_SHAPE       # a dense second source of another row count
    assert dgrad(w=N) == L.ERR_ARG
    assert dgrad(da=N, db=N) == L.ERR_ARG
    assert wgrad(a=N) == L.ERR_ARG
    assert wgrad(b=N) == L.ERR_ARG
    assert wgrad(dw=N) == L.ERR_ARG
    nb = ctypes.c_size_t()
    assert lib.shpl_head1x1_workspace_bytes(L.F32, 120, 64, 80, 32, 18, 1, ctypes.byref(nb)) == L.OK
    assert dgrad(ws_bytes=nb.value - 1) == L.ERR_WORKSPACE
    assert lib.shpl_head1x1_wgrad_workspace_bytes(L.F32, 120, 64, 80, 32, 18, 1, ctypes.byref(nb)) == L.OK
    assert wgrad(ws_bytes=nb.value - 1) == L.ERR_WORKSPACE


def test_workspace_queries_are_host_only_and_monotone(lib):
    from sparse_pooling_amd import _lib as L

    def q(fn, dtype, rows, c_a, rows_b, c_b, c_out, pooled):
        nb = ctypes.c_size_t()
        assert fn(dtype, rows, c_a, rows_b, c_b, c_out, pooled, ctypes.byref(nb)) == L.OK
        return nb.value

    for fn in (lib.shpl_head1x1_workspace_bytes, lib.shpl_head1x1_wgrad_workspace_bytes):
        assert fn(L.F32, 10, 8, 10, 8, 0, 1, ctypes.byref(ctypes.c_size_t())) == L.ERR_BAD_SHAPE
        assert fn(L.F32, 10, 8, 10, 8, 33, 1, ctypes.byref(ctypes.c_size_t())) == L.ERR_BAD_SHAPE
        assert fn(5, 10, 8, 10, 8, 18, 1, ctypes.byref(ctypes.c_size_t())) == L.ERR_ARG
        assert fn(L.F32, 10, 8, 10, 8, 18, 1, None) == L.ERR_ARG
        for dtype in (L.F32, L.BF16):
            for pooled in (0, 1):
                base = (96000, 768, 61440, 768, 18)
                prev = q(fn, dtype, *base, pooled)
                assert prev > 0
                # every step grows one of rows, c_a, rows_b, c_b, c_out: never a smaller workspace
                sizes = [1, 63, 64, 65, 16383, 16384, 16385, 20000, 96000, 200000]
                for i, steps in enumerate((sizes, [1, 5, 768, 1536], sizes, [1, 6, 768, 1536], [1, 8, 9, 18, 32])):
                    last = 0
                    for v in steps:
                        args = list(base)
                        args[i] = v
                        cur = q(fn, dtype, *args, pooled)
                        assert cur >= last, (fn, dtype, pooled, i, v)
                        last = cur
    # the MV3D shape: Z (61440 x 32 f32) and the packed weights fit; nothing near the maps' own size
    fwd = q(lib.shpl_head1x1_workspace_bytes, L.F32, 96000, 768, 61440, 768, 18, 1)
    assert 61440 * 32 * 4 <= fwd < 96000 * 768 * 4 // 4
