"""The fused concat-with-BatchNorm entry points of the C ABI (CPU only: no compute calls, no GPU needed): the four
symbols are declared in include/shpl.h and exported, the workspace queries are host arithmetic, and every bad
argument the header lists is refused on the host with SHPL_ERR_ARG before anything is launched (the pointers
handed over are fake and never dereferenced)."""
import ctypes
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("shpl_concat_bn_workspace_bytes", "shpl_concat_bn", "shpl_concat_bn_backward_workspace_bytes",
         "shpl_concat_bn_backward")
P = 256  # a fake, 16-byte aligned, non-null device pointer: never dereferenced
ROWS, C_PASS, C_POOL = 8960, 32, 32


def _lib():
    from sparse_pooling_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        from sparse_pooling_amd import build
        build.build()
    return L, L.lib()


def test_symbols_are_declared_and_exported():
    L, lib = _lib()
    header = open(os.path.join(ROOT, "include", "shpl.h")).read()
    for name in NAMES:
        assert name + "(" in header and hasattr(lib, name) and name in L.EXPORTED
    # the header names the reference lines it replaces and what the reference's own code does there
    assert "sparse_pool_utils.py:69-70" in header and ":120-124" in header and "TypeError" in header


def _need(L, lib, backward=False, rows=ROWS, c_pass=C_PASS, c_pool=C_POOL):
    nb = ctypes.c_size_t()
    q = lib.shpl_concat_bn_backward_workspace_bytes if backward else lib.shpl_concat_bn_workspace_bytes
    assert q(rows, c_pass, c_pool, ctypes.byref(nb)) == L.OK
    return nb.value


def test_workspace_queries_are_host_only():
    L, lib = _lib()
    c = C_PASS + C_POOL
    blocks = -(-ROWS // 4096)  # 4096 rows per block of partial sums: 8960 rows are three
    assert blocks == 3
    assert _need(L, lib) == blocks * 2 * c * 8 + 2 * c * 8  # f64 partials, f64 statistics (multiples of 256)
    assert _need(L, lib, backward=True) == blocks * 2 * c * 8 + 2 * c * 4  # f64 partials, the f32 mean terms
    assert _need(L, lib, rows=0) > 0 and _need(L, lib, rows=4096) < _need(L, lib, rows=4097)
    nb = ctypes.c_size_t()
    for q in (lib.shpl_concat_bn_workspace_bytes, lib.shpl_concat_bn_backward_workspace_bytes):
        assert q(ROWS, C_PASS, C_POOL, None) == L.ERR_ARG
        assert q(-1, C_PASS, C_POOL, ctypes.byref(nb)) == L.ERR_ARG
        assert q(ROWS, 0, C_POOL, ctypes.byref(nb)) == L.ERR_ARG
        assert q(ROWS, C_PASS, 0, ctypes.byref(nb)) == L.ERR_ARG


def _csr(L, key_range=True, n_keys=ROWS, nnz_cap=100, col=False):
    return L.ShplCsr(P, P, P, P if col else None, n_keys, nnz_cap, P if key_range else None)


def _fwd(L, lib, csr="rows", direction=None, dtype=None, src=P, c_pool=C_POOL, pass_=P, c_pass=C_PASS, out=P,
         out_stride=C_PASS + C_POOL, training=1, mm=P, mv=P, save=P, ws=P, ws_bytes=None):
    v = ctypes.c_void_p
    csr = _csr(L) if csr == "rows" else csr
    ws_bytes = _need(L, lib) if ws_bytes is None else ws_bytes
    return lib.shpl_concat_bn(L.BY_CELL if direction is None else direction, L.F32 if dtype is None else dtype,
                              ctypes.byref(csr) if csr is not None else None, v(src), c_pool, 0, c_pool, v(pass_),
                              c_pass, 0, c_pass, v(out), out_stride, training, 1e-3, 0.999, None, v(P), v(mm), v(mv),
                              None, None, v(save), v(ws), ws_bytes, None)


def _bwd(L, lib, csr="rows", grad="rows", direction=None, dtype=None, c_pool=C_POOL, c_pass=C_PASS, g=P,
         g_stride=C_PASS + C_POOL, save=P, gpass=P, gpool=P, gsrc=P, ws=P, ws_bytes=None):
    v = ctypes.c_void_p
    csr = _csr(L) if csr == "rows" else csr
    grad = _csr(L, key_range=False, n_keys=960, col=True) if grad == "rows" else grad
    ws_bytes = _need(L, lib, backward=True) if ws_bytes is None else ws_bytes
    return lib.shpl_concat_bn_backward(L.BY_CELL if direction is None else direction,
                                       L.F32 if dtype is None else dtype,
                                       ctypes.byref(csr) if csr is not None else None,
                                       ctypes.byref(grad) if grad is not None else None, v(P), c_pool, 0, c_pool, v(P),
                                       c_pass, 0, c_pass, v(g), g_stride, v(save), None, 1, v(gpass), c_pass, v(gpool),
                                       v(gsrc), c_pool, v(P), v(P), v(ws), ws_bytes, None)


def test_forward_rejections_launch_nothing():
    L, lib = _lib()
    E = L.ERR_ARG
    assert _fwd(L, lib, csr=None) == E
    assert _fwd(L, lib, csr=_csr(L, key_range=False)) == E  # a CSR without key_range
    for bad in (0, -4):
        assert _fwd(L, lib, c_pool=bad) == E and _fwd(L, lib, c_pass=bad) == E
    assert _fwd(L, lib, out=None) == E  # a NULL output
    assert _fwd(L, lib, src=None) == E and _fwd(L, lib, pass_=None) == E
    assert _fwd(L, lib, out_stride=C_PASS + C_POOL - 1) == E  # an output stride below c_pass + c_pool
    assert _fwd(L, lib, ws_bytes=_need(L, lib) - 1) == E  # a workspace that is too small
    assert _fwd(L, lib, dtype=L.F64) == E and _fwd(L, lib, dtype=7) == E  # a bad dtype
    assert _fwd(L, lib, direction=2) == E and _fwd(L, lib, direction=-1) == E  # a bad direction
    assert _fwd(L, lib, ws=None) == E and _fwd(L, lib, save=None) == E  # training with no workspace
    assert _fwd(L, lib, training=0, mm=None, ws=None) == E and _fwd(L, lib, training=0, mv=None, ws=None) == E
    # a pixel-keyed CSR that neither carries columns nor is marked as identity columns (shpl_pull's rule)
    assert _fwd(L, lib, direction=L.BY_PIXEL) == E
    # an empty batch is accepted and launches nothing (the fake pointers are never touched)
    assert _fwd(L, lib, csr=_csr(L, n_keys=0, nnz_cap=0)) == L.OK
    assert _fwd(L, lib, csr=_csr(L, n_keys=0, nnz_cap=0), training=0, ws=None, ws_bytes=0) == L.OK


def test_backward_rejections_launch_nothing():
    L, lib = _lib()
    E = L.ERR_ARG
    assert _bwd(L, lib, csr=None) == E
    assert _bwd(L, lib, csr=_csr(L, key_range=False)) == E
    for bad in (0, -4):
        assert _bwd(L, lib, c_pool=bad) == E and _bwd(L, lib, c_pass=bad) == E
    assert _bwd(L, lib, gpass=None) == E and _bwd(L, lib, gpool=None) == E and _bwd(L, lib, g=None) == E
    assert _bwd(L, lib, save=None) == E
    assert _bwd(L, lib, g_stride=C_PASS + C_POOL - 1) == E
    assert _bwd(L, lib, ws=None) == E and _bwd(L, lib, ws_bytes=_need(L, lib, backward=True) - 1) == E
    assert _bwd(L, lib, dtype=7) == E and _bwd(L, lib, direction=2) == E
    assert _bwd(L, lib, grad=None) == E  # a source gradient asked for without the CSR that carries it back
