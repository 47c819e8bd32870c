"""The ragged index entry points of the C ABI (CPU only: no compute calls, no GPU needed): both are exported, and
bad arguments are rejected on the host in shpl_build_index's order -- pointers (d_im_sizes among them), then
shapes (the padded map's size among them), then the 2^31 bound and the bucket limits on img_rows * img_cols."""
import ctypes
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from sparse_pooling_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        from sparse_pooling_amd import build
        build.build()
    return L, L.lib()


def test_ragged_symbols_are_declared_and_exported():
    L, lib = _lib()
    header = open(os.path.join(ROOT, "include", "shpl.h")).read()
    for name in ("shpl_build_index_ragged", "shpl_build_index_buckets_ragged"):
        assert name + "(" in header
        assert hasattr(lib, name)
        assert name in L.EXPORTED


P = ctypes.c_void_p(256)  # a fake, aligned, non-null device pointer: never dereferenced
N = None


def _index(lib, n_frames=1, off=P, maxp=10, pts=P, vox=P, vstride=2, Pm=P, sizes=P, rows=94, cols=310, s_img=4.,
           s_bv=4., cell=P, ws=P, ws_bytes=1 << 20):
    return lib.shpl_build_index_ragged(n_frames, off, N, maxp, pts, 2, vox, 1, vstride, Pm, sizes, rows, cols, 704.,
                                       800., s_img, s_bv, N, cell, P, P, N, N, P, P, N, ws, ws_bytes, N)


def _buckets(lib, n_frames=4, off=P, maxp=20000, vstride=2, sizes=P, rows=47, cols=155, s_img=8., s_bv=8., ws=P,
             ws_bytes=1 << 20, nnz_cap=80000, bkt=P, bkt_bytes=1 << 24, nnz=P, cell_copy=N, pixel_copy=N):
    return lib.shpl_build_index_buckets_ragged(n_frames, off, N, maxp, P, 2, P, 1, vstride, P, sizes, rows, cols,
                                               704., 800., s_img, s_bv, N, P, P, P, nnz, P, P, ws, ws_bytes, nnz_cap,
                                               bkt, bkt_bytes, cell_copy, pixel_copy, N)


def test_ragged_index_rejections_in_index_args_order():
    L, lib = _lib()
    assert L.F64 == 2 and L.I64 == 1
    # 1. frames and pointers, d_im_sizes among them
    assert _index(lib, n_frames=0) == L.ERR_ARG
    assert _index(lib, off=N) == L.ERR_ARG
    assert _index(lib, Pm=N) == L.ERR_ARG
    assert _index(lib, ws=N) == L.ERR_ARG
    assert _index(lib, sizes=N) == L.ERR_ARG
    # ... before the shapes: a missing size array with a bad map is still an argument error
    assert _index(lib, sizes=N, rows=0) == L.ERR_ARG
    assert _index(lib, sizes=N, vstride=1) == L.ERR_ARG
    # 2. the point arrays (only when frames may hold points)
    assert _index(lib, pts=N) == L.ERR_ARG
    assert _index(lib, cell=N) == L.ERR_ARG
    assert _index(lib, pts=N, rows=0) == L.ERR_ARG
    # 3. shapes: voxel stride, strides, the padded map's size
    assert _index(lib, vstride=1) == L.ERR_BAD_SHAPE
    assert _index(lib, s_img=0.) == L.ERR_BAD_SHAPE
    assert _index(lib, s_bv=float("nan")) == L.ERR_BAD_SHAPE
    for rows, cols in ((0, 310), (94, 0), (-1, 310), (94, -5)):
        assert _index(lib, rows=rows, cols=cols) == L.ERR_BAD_SHAPE
    # 4. global ids in 32 bits, on img_rows * img_cols (and a product past 2^63 is refused, not wrapped)
    assert _index(lib, n_frames=64, rows=8192, cols=4096) == L.ERR_BAD_SHAPE  # 64 * 2^25 = 2^31
    assert _index(lib, rows=1 << 40, cols=1 << 40) == L.ERR_BAD_SHAPE
    assert _index(lib, n_frames=63, rows=8192, cols=4096, ws_bytes=16) == L.ERR_WORKSPACE  # in bounds: the next check
    # 5. the workspace is shpl_build_index's
    need = L.index_ws_bytes(64, 100000)
    assert _index(lib, n_frames=64, maxp=100000, ws_bytes=need - 1) == L.ERR_WORKSPACE


def test_ragged_bucket_index_rejections():
    L, lib = _lib()
    assert _buckets(lib, sizes=N) == L.ERR_ARG
    assert _buckets(lib, sizes=N, rows=0) == L.ERR_ARG
    assert _buckets(lib, rows=0) == L.ERR_BAD_SHAPE
    assert _buckets(lib, cols=0) == L.ERR_BAD_SHAPE
    assert _buckets(lib, vstride=1) == L.ERR_BAD_SHAPE
    # index_args' checks come before the bucket call's own pointers
    assert _buckets(lib, bkt=N, rows=0) == L.ERR_BAD_SHAPE
    assert _buckets(lib, bkt=N) == L.ERR_ARG
    assert _buckets(lib, nnz=N) == L.ERR_ARG
    # the bucket limits on the padded map: at most 65536 pixels per frame
    assert _buckets(lib, rows=256, cols=257) == L.ERR_BAD_SHAPE
    assert _buckets(lib, rows=256, cols=256, bkt_bytes=64) == L.ERR_WORKSPACE  # inside the limit: the next check
    assert _buckets(lib, bkt_bytes=64) == L.ERR_WORKSPACE
    # the workspace-size query is the uniform entry's, with pix_per_frame = img_rows * img_cols
    need = L.bucket_ws_bytes(4, 20000, 80000, 88 * 100, 47 * 155)
    assert _buckets(lib, bkt_bytes=need - 1) == L.ERR_WORKSPACE
    # the riders' shape rule is unchanged
    odd = L.ShplPassCopy(L.BF16, 256, 12, 256, 24, 12)  # 24-byte rows: not 16-byte pieces
    assert _buckets(lib, cell_copy=ctypes.byref(odd)) == L.ERR_BAD_SHAPE


def test_index_args_ragged_helper_layout():
    """_lib.index_args_ragged: index_args with (im_w, im_h) replaced by (d_im_sizes, img_rows, img_cols)."""
    import torch
    L, _ = _lib()
    i64 = lambda *s: torch.zeros(s, dtype=torch.int64)  # noqa: E731
    off, pts, vox, Pm = i64(3), torch.zeros((4, 3), dtype=torch.float64), i64(4, 2), torch.zeros((2, 12), dtype=torch.float64)
    cell = pix = torch.zeros(4, dtype=torch.int32)
    val = torch.zeros(4)
    sizes = torch.tensor([[1242., 375.], [1224., 370.]], dtype=torch.float64)
    uni = L.index_args(2, off, None, 4, pts, vox, Pm, (1242, 376), (704, 800), (4, 4), None, cell, pix, val)
    rag = L.index_args_ragged(2, off, None, 4, pts, vox, Pm, sizes, (94, 310), (704, 800), (4, 4), None, cell, pix,
                              val)
    assert len(uni) == 20 and len(rag) == 21
    val_of = lambda a: a.value if isinstance(a, ctypes.c_void_p) else a  # noqa: E731
    assert [val_of(a) for a in rag[:10]] == [val_of(a) for a in uni[:10]]
    assert rag[10].value == sizes.data_ptr() and rag[11:13] == (94, 310)
    assert [val_of(a) for a in rag[13:]] == [val_of(a) for a in uni[12:]]
