"""The upconv3 gradients' C ABI (shpl_upconv3x3_dgrad / shpl_upconv3x3_wgrad and their workspace queries): exported,
bound in _lib, and every argument check answered on the host -- no GPU: the fake, aligned, non-null device pointers
are never dereferenced (as tests/test_abi.py::test_argument_validation_is_host_side)."""
import ctypes

import pytest

from sparse_pooling_amd import _lib as L

P = ctypes.c_void_p(256)  # a fake, aligned, non-null device pointer
N = None
NAMES = ("shpl_upconv3x3_dgrad_workspace_bytes", "shpl_upconv3x3_dgrad", "shpl_upconv3x3_wgrad_workspace_bytes",
         "shpl_upconv3x3_wgrad")
# the reference's shape: 8 frames of 88 x 100, 256 + 256 -> 128
F, H, W, CA, CB, CO = 8, 88, 100, 256, 256, 128


def _bytes(fn, *args):
    out = ctypes.c_size_t(0)
    assert fn(*args, ctypes.byref(out)) == L.OK
    return out.value


def test_symbols_are_exported_and_bound():
    lib = L.lib()
    for name in NAMES:
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes, name


@pytest.mark.parametrize("dt", [L.F32, L.BF16])
def test_workspace_queries_answer_on_the_host(dt):
    lib = L.lib()
    assert lib.shpl_upconv3x3_dgrad_workspace_bytes(dt, F, H, W, CO, CA + CB, N) == L.ERR_ARG
    assert lib.shpl_upconv3x3_wgrad_workspace_bytes(dt, F, H, W, CA, CB, CO, -1, N) == L.ERR_ARG
    assert _bytes(lib.shpl_upconv3x3_dgrad_workspace_bytes, dt, F, H, W, CO, CA + CB) > 0
    dense = _bytes(lib.shpl_upconv3x3_wgrad_workspace_bytes, dt, F, H, W, CA, CB, CO, -1)
    pooled = _bytes(lib.shpl_upconv3x3_wgrad_workspace_bytes, dt, F, H, W, CA, CB, CO, 160000)
    assert dense > 0 and pooled > dense  # the pooled call's row pointers


def _dgrad(lib, dt=L.F32, n=F, h=H, gy=P, gy_stride=CO, c_gy=CO, w=P, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = _bytes(lib.shpl_upconv3x3_dgrad_workspace_bytes, L.F32, F, H, W, CO, CA + CB)
    return lib.shpl_upconv3x3_dgrad(dt, n, h, W, gy, gy_stride, c_gy, w, CA + CB, P, CA, CA, P, CB, ws, ws_bytes, N)


def _wgrad(lib, dt=L.F32, n=F, h=H, gy=P, gy_stride=CO, c_out=CO, dw=P, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = _bytes(lib.shpl_upconv3x3_wgrad_workspace_bytes, L.F32, F, H, W, CA, CB, CO, -1)
    return lib.shpl_upconv3x3_wgrad(dt, n, h, W, P, CA, 0, CA, P, CB, 0, CB, N, N, gy, gy_stride, c_out, dw, ws,
                                    ws_bytes, N)


def _forward_short_out_stride(lib):
    """What shpl_upconv3x3 answers for out_stride < c_out (everything else valid)."""
    ws = _bytes(lib.shpl_upconv3x3_workspace_bytes, L.F32, F, H, W, CA, CB, CO, -1, 0)
    return lib.shpl_upconv3x3(L.F32, F, H, W, P, CA, 0, CA, P, CB, 0, CB, N, N, P, CO, N, N, N, L.ACT_NONE, P,
                              CO - 1, N, P, ws, N)


def test_dgrad_argument_checks():
    lib = L.lib()
    full = _bytes(lib.shpl_upconv3x3_dgrad_workspace_bytes, L.F32, F, H, W, CO, CA + CB)
    assert _dgrad(lib, dt=7) == L.ERR_ARG
    assert _dgrad(lib, c_gy=0, gy_stride=0) == L.ERR_BAD_SHAPE
    assert _dgrad(lib, h=-1) == L.ERR_BAD_SHAPE
    assert _dgrad(lib, ws_bytes=full - 1) == L.ERR_WORKSPACE
    assert _dgrad(lib, w=N) == L.ERR_ARG
    assert _dgrad(lib, gy=N) == L.ERR_ARG
    short = _forward_short_out_stride(lib)
    assert short != L.OK and _dgrad(lib, gy_stride=CO - 1) == short
    assert _dgrad(lib, n=0) == L.OK


def test_wgrad_argument_checks():
    lib = L.lib()
    full = _bytes(lib.shpl_upconv3x3_wgrad_workspace_bytes, L.F32, F, H, W, CA, CB, CO, -1)
    assert _wgrad(lib, dt=7) == L.ERR_ARG
    assert _wgrad(lib, c_out=0, gy_stride=0) == L.ERR_BAD_SHAPE
    assert _wgrad(lib, h=-1) == L.ERR_BAD_SHAPE
    assert _wgrad(lib, ws_bytes=full - 1) == L.ERR_WORKSPACE
    assert _wgrad(lib, dw=N) == L.ERR_ARG  # the weights' place: the gradient it writes
    assert _wgrad(lib, gy=N) == L.ERR_ARG
    short = _forward_short_out_stride(lib)
    assert short != L.OK and _wgrad(lib, gy_stride=CO - 1) == short
    assert _wgrad(lib, n=0) == L.OK
