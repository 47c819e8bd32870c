"""ctypes binding of libshpl.so (include/shpl.h).

The product path has no fallback: if the HIP library is missing or cannot be
loaded, every SHPL op raises ``ShplLibraryError``. Tensors cross the C ABI as
raw device pointers plus the current HIP stream of the calling thread.
"""
import collections
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# SHPL_LIB: an alternative build of the same sources (A/B measurements of compile-time variants)
LIB_PATH = os.environ.get("SHPL_LIB") or os.path.join(_HERE, "libshpl.so")

# enums of include/shpl.h
OK, ERR_BAD_SHAPE, ERR_INDEX_OOB, ERR_HIP, ERR_WORKSPACE, ERR_ARG = range(6)
EBIT_ROW, EBIT_COL, EBIT_PIXEL, EBIT_VALUES, EBIT_CAPACITY, EBIT_BARRIER, EBIT_GATHER = 1, 2, 4, 8, 16, 32, 64
F32, BF16, F64 = 0, 1, 2
I32, I64 = 0, 1
BY_CELL, BY_PIXEL = 0, 1
ORDER_ENTRY, ORDER_COL_ROW, ORDER_COL_ENTRY = 0, 1, 2
OUT_POOL, OUT_CONCAT, OUT_ADD = 0, 1, 2
ACT_NONE, ACT_RELU = 0, 1
CSR_AUTO, CSR_FRAME, CSR_SEGMENT, CSR_RANGE = 0, 1, 2, 3
CSR_IDENTITY_COLS = 1
CSR_MAX_HEAD = 32

_lib = None


class ShplLibraryError(RuntimeError):
    pass


LIVE_MAX_FRAMES = 1024  # SHPL_LIVE_MAX_FRAMES


class ShplCsr(ctypes.Structure):
    """struct shpl_csr of include/shpl.h (device pointers + sizes)."""
    _fields_ = [("ent_dst", ctypes.c_void_p), ("ent_src", ctypes.c_void_p),
                ("ent_val", ctypes.c_void_p), ("ent_col", ctypes.c_void_p),
                ("n_keys", ctypes.c_int64), ("nnz_cap", ctypes.c_int64), ("key_range", ctypes.c_void_p),
                ("frame_off", ctypes.c_void_p), ("frame_nnz", ctypes.c_void_p), ("n_frames", ctypes.c_int64),
                ("flags", ctypes.c_int64), ("heads", ctypes.c_void_p), ("head_k", ctypes.c_int64)]


class Csr:
    """Device buffers of one destination-sorted entry list (owned tensors + the ABI struct)."""

    def __init__(self, n_keys, nnz_cap, device, with_col, key_range=False, identity_cols=False, head_k=0):
        """key_range: also keep the (first, end) entry of every destination
        (shpl_csr.key_range): shpl_pull then runs its one-launch row-keyed form.
        identity_cols: a pixel-keyed CSR of shpl_build_csr_buckets without ent_col (SHPL_CSR_IDENTITY_COLS).
        head_k: run heads of that many entries per destination (shpl_csr.heads; shpl_build_csr_buckets)."""
        i32 = dict(dtype=torch.int32, device=device)
        cap = max(int(nnz_cap), 1)
        self.n_keys, self.nnz_cap = int(n_keys), int(nnz_cap)
        self.ent_dst = torch.empty(cap, **i32)
        if self.nnz_cap == 0:
            # an empty map keeps one padding slot, which no builder writes (nnz_cap 0) and which ops._csr counts as
            # capacity (the tensor's length): mark it empty, or the sparse pass reads whatever the allocator left
            self.ent_dst.fill_(-1)
        self.ent_src = torch.empty(cap, **i32)
        self.ent_val = torch.empty(cap, dtype=torch.float32, device=device)
        self.ent_col = torch.empty(cap, **i32) if with_col else None
        self.key_range = torch.empty((max(self.n_keys, 1), 2), **i32) if key_range else None
        self.ws = workspace(csr_ws_bytes(self.n_keys, self.nnz_cap), device)
        self.struct = ShplCsr(self.ent_dst.data_ptr(), self.ent_src.data_ptr(), self.ent_val.data_ptr(),
                              self.ent_col.data_ptr() if with_col else None, self.n_keys, self.nnz_cap,
                              self.key_range.data_ptr() if key_range else None)
        self.struct.flags = CSR_IDENTITY_COLS if identity_cols else 0
        self.heads = None
        if head_k:
            assert key_range and 1 <= head_k <= CSR_MAX_HEAD
            self.heads = torch.empty((max(self.n_keys, 1), int(head_k), 2), **i32)
            self.struct.heads, self.struct.head_k = self.heads.data_ptr(), int(head_k)

    def live_frames(self, frame_off, frame_nnz):
        """Hand the sparse pass the frame layout the CSR was built with (device i64 [F+1] / [F],
        kept alive here): it then walks only the live entries of each frame's capacity."""
        if frame_nnz is None or frame_nnz.numel() > LIVE_MAX_FRAMES:
            self._frames = None
            self.struct.frame_off, self.struct.frame_nnz, self.struct.n_frames = None, None, 0
            return self
        assert frame_off.dtype == torch.int64 and frame_nnz.dtype == torch.int64
        assert frame_off.numel() == frame_nnz.numel() + 1
        self._frames = (frame_off, frame_nnz)
        self.struct.frame_off, self.struct.frame_nnz = frame_off.data_ptr(), frame_nnz.data_ptr()
        self.struct.n_frames = int(frame_nnz.numel())
        return self

    def ref(self):
        return ctypes.byref(self.struct)


class ShplBuckets(ctypes.Structure):
    """struct shpl_buckets of include/shpl.h."""
    _fields_ = [("n_frames", ctypes.c_int), ("max_points_per_frame", ctypes.c_int64), ("nnz_cap", ctypes.c_int64),
                ("cells_per_frame", ctypes.c_int64), ("pix_per_frame", ctypes.c_int64),
                ("frame_off", ctypes.c_void_p), ("frame_nnz", ctypes.c_void_p), ("cell", ctypes.c_void_p),
                ("pix", ctypes.c_void_p), ("val", ctypes.c_void_p), ("ws", ctypes.c_void_p),
                ("ws_bytes", ctypes.c_size_t), ("err", ctypes.c_void_p)]


class ShplPullDesc(ctypes.Structure):
    """struct shpl_pull_desc of include/shpl.h: shpl_pull's arguments after its csr (shpl_pull_pair)."""
    _fields_ = [("dtype", ctypes.c_int), ("src", ctypes.c_void_p), ("src_stride", ctypes.c_int64),
                ("src_off", ctypes.c_int64), ("c_pool", ctypes.c_int64), ("pass_", ctypes.c_void_p),
                ("pass_stride", ctypes.c_int64), ("pass_off", ctypes.c_int64), ("c_pass", ctypes.c_int64),
                ("mode", ctypes.c_int), ("out", ctypes.c_void_p), ("out_stride", ctypes.c_int64)]


class ShplPassCopy(ctypes.Structure):
    """struct shpl_pass_copy of include/shpl.h (a rider of shpl_build_index_buckets)."""
    _fields_ = [("dtype", ctypes.c_int), ("src", ctypes.c_void_p), ("src_stride", ctypes.c_int64),
                ("out", ctypes.c_void_p), ("out_stride", ctypes.c_int64), ("channels", ctypes.c_int64)]


class ShplIndexLevel(ctypes.Structure):
    """struct shpl_index_level of include/shpl.h: one fusion level of shpl_build_index_levels."""
    _fields_ = [("s_img", ctypes.c_double), ("s_bv", ctypes.c_double), ("bv_h", ctypes.c_double),
                ("bv_w", ctypes.c_double), ("cell", ctypes.c_void_p), ("pix", ctypes.c_void_p),
                ("val", ctypes.c_void_p), ("mij", ctypes.c_void_p), ("flip", ctypes.c_void_p),
                ("frame_nnz", ctypes.c_void_p)]


MAX_INDEX_LEVELS = 4  # SHPL_MAX_INDEX_LEVELS


def _addr(t, col=0):
    """Device pointer of a tensor as an integer, `col` elements on (None for None)."""
    return None if t is None else t.data_ptr() + (col and col * t.element_size())


class Pull(collections.namedtuple("Pull", [n for n, _ in ShplPullDesc._fields_])):
    """shpl_pull's twelve arguments after its csr, pointers as integers (None: NULL)."""

    @classmethod
    def of(cls, src, src_stride, src_off, c_pool, pass_, pass_stride, pass_off, c_pass, mode, out, out_stride,
           out_col=0, dtype=None):
        """From tensors, in shpl_pull's order. out_col: the pull writes out's rows from that column on (the pooled
        half of a fused row: the one place its pointer is formed). dtype: out's, unless given."""
        return cls(dtype_code(out) if dtype is None else dtype, _addr(src), src_stride, src_off, c_pool, _addr(pass_),
                   pass_stride, pass_off, c_pass, mode, _addr(out, out_col), out_stride)

    def args(self, direction, csr):
        """The arguments of shpl_pull / _dense / _sparse / _once before the stream."""
        p = ctypes.c_void_p  # (c_void_p(None) is NULL)
        dtype, src, src_stride, src_off, c_pool, pass_, pass_stride, pass_off, c_pass, mode, out, out_stride = self
        return (direction, dtype, csr.ref(), p(src), src_stride, src_off, c_pool, p(pass_), pass_stride, pass_off,
                c_pass, mode, p(out), out_stride)

    def desc(self):
        """The ShplPullDesc of shpl_pull_pair."""
        return ShplPullDesc(*self)


def pull_desc(dtype, *fields):
    """A ShplPullDesc from tensors (the same argument order as shpl_pull after its csr)."""
    return Pull.of(*fields, dtype=dtype).desc()


def _declare(lib):
    p, i32, i64, d, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double, ctypes.c_size_t
    psz, u64 = ctypes.POINTER(ctypes.c_size_t), ctypes.c_uint64
    pull_args = [i32, i32, ctypes.POINTER(ShplCsr), p, i64, i64, i64, p, i64, i64, i64, i32, p, i64, p]
    sig = {
        "shpl_version": (ctypes.c_char_p, []),
        "shpl_status_string": (ctypes.c_char_p, [i32]),
        "shpl_build_index_workspace_bytes": (i32, [i32, i64, psz]),
        "shpl_build_index": (i32, [i32, p, p, i64, p, i32, p, i32, i64, p, d, d, d, d, d, d, p,
                                   p, p, p, p, p, p, p, p, p, sz, p]),
        "shpl_build_index_ragged": (i32, [i32, p, p, i64, p, i32, p, i32, i64, p, p, i64, i64, d, d, d, d, p,
                                          p, p, p, p, p, p, p, p, p, sz, p]),
        "shpl_build_index_levels_workspace_bytes": (i32, [i32, i64, i32, psz]),
        "shpl_build_index_levels": (i32, [i32, p, p, i64, p, i32, p, i32, i64, p, d, d, p, i32,
                                          ctypes.POINTER(ShplIndexLevel), p, p, p, sz, p]),
        "shpl_build_index_levels_ragged": (i32, [i32, p, p, i64, p, i32, p, i32, i64, p, p, p, i32,
                                                 ctypes.POINTER(ShplIndexLevel), ctypes.POINTER(ctypes.c_int64),
                                                 p, p, p, sz, p]),
        "shpl_bev_workspace_bytes": (i32, [i64, i32, psz]),
        "shpl_mv3d_workspace_bytes": (i32, [i64, psz]),
        "shpl_mv3d_voxels": (i32, [i32, p, i64, p, i64, p, p, p, p, d, d, i32, p, i64, p, p, p, p, p, p,
                                   sz, p]),
        "shpl_mv3d_augment_points": (i32, [i32, p, i64, p, i32, i64, p, p, p, p, i64, p, p, i64, p, p]),
        "shpl_mv3d_voxels_aug": (i32, [i32, p, i64, p, i32, i64, p, p, p, p, p, p, i64, p, d, d, i32, p, i64, p, p, p,
                                       p, p, p, p, sz, p]),
        "shpl_bev_slices": (i32, [i32, p, p, i64, p, i32, p, p, d, i32, p, p, d, d, d, p, p, p, p, p, p,
                                  p, p, sz, p]),
        "shpl_bev_maps": (i32, [i32, p, i64, p, i32, p, p, d, i32, p, p, d, d, d, p, p, p, i32, p, sz, p]),
        "shpl_bev_input": (i32, [i32, p, i64, p, i32, p, p, d, i32, p, p, d, d, d, p, p, p, sz, p]),
        "shpl_velo_workspace_bytes": (i32, [i32, i64, psz]),
        "shpl_velo_to_cam": (i32, [i32, p, i64, p, p, p, p, d, p, p, p, p, p, sz, p]),
        "shpl_gen_index": (i32, [i64, p, i32, p, i32, i64, p, d, d, p, p, i64, p, p, sz, p]),
        "shpl_produce_index": (i32, [i64, p, i32, i64, p, i64, d, d, d, d, d, d, p, p, p, p, p,
                                     p, p, sz, p]),
        "shpl_pack_map": (i32, [i64, p, p, i64, i64, i64, p, i32, i64, i64, i64, i64, i64, i64,
                                p, p, p, p, p, p]),
        "shpl_csr_workspace_bytes": (i32, [i64, i64, psz]),
        "shpl_build_csr": (i32, [i32, i32, i32, p, p, i64, p, p, p, p, ctypes.POINTER(ShplCsr), p, sz,
                                 p]),
        "shpl_build_csr_path": (i32, [i32, i32, i32, i32, p, p, i64, p, p, p, p, ctypes.POINTER(ShplCsr), p,
                                      sz, p]),
        "shpl_bucket_workspace_bytes": (i32, [i32, i64, i64, i64, i64, psz]),
        "shpl_bucket_workspace_reset": (i32, [i32, p, sz, p]),
        "shpl_build_index_buckets": (i32, [i32, p, p, i64, p, i32, p, i32, i64, p, d, d, d, d, d, d, p,
                                           p, p, p, p, p, p, p, sz, i64, p, sz, ctypes.POINTER(ShplPassCopy),
                                           ctypes.POINTER(ShplPassCopy), p]),
        "shpl_build_index_buckets_ragged": (i32, [i32, p, p, i64, p, i32, p, i32, i64, p, p, i64, i64, d, d, d, d, p,
                                                  p, p, p, p, p, p, p, sz, i64, p, sz,
                                                  ctypes.POINTER(ShplPassCopy), ctypes.POINTER(ShplPassCopy), p]),
        "shpl_build_csr_buckets": (i32, [ctypes.POINTER(ShplBuckets), ctypes.POINTER(ShplCsr),
                                         ctypes.POINTER(ShplCsr), p]),
        "shpl_pull_pair": (i32, [ctypes.POINTER(ShplCsr), ctypes.POINTER(ShplPullDesc), ctypes.POINTER(ShplCsr),
                                 ctypes.POINTER(ShplPullDesc), p]),
        "shpl_pull": (i32, pull_args),
        "shpl_pull_dense": (i32, pull_args),
        "shpl_pull_sparse": (i32, pull_args),
        "shpl_pull_once": (i32, pull_args),
        "shpl_pull_clear": (i32, [i32, ctypes.POINTER(ShplCsr), i64, p, i64, i64, p]),
        "shpl_conv3x3_workspace_bytes": (i32, [i32, i32, i64, i64, i64, i64, i64, i64, i32, psz]),
        "shpl_conv3x3": (i32, [i32, i32, i64, i64, p, i64, i64, i64, p, i64, i64, i64,
                               ctypes.POINTER(ShplCsr), p, p, i64, p, p, p, i32, p, i64, p, p, sz, p]),
        "shpl_conv3x3_rows_form": (i32, [i32, i32, i64, i64, p, i64, i64, i64, p, i64, i64, i64,
                                         ctypes.POINTER(ShplCsr), p, p, i64, i32, p, i64, i32,
                                         ctypes.POINTER(ctypes.c_int)]),
        "shpl_conv3x3_wide_form": (i32, [i32, i32, i64, i64, p, i64, i64, i64, p, i64, i64, i64,
                                         ctypes.POINTER(ShplCsr), p, p, i64, i32, p, i64, i32,
                                         ctypes.POINTER(ctypes.c_int)]),
        "shpl_batch_norm": (i32, [i32, i64, p, p, i64, i64, p, d, ctypes.c_float, p, p, i32, p, p,
                                  ctypes.c_float, p, p, p, p]),
        "shpl_batch_norm_backward_workspace_bytes": (i32, [i64, i64, psz]),
        "shpl_batch_norm_backward": (i32, [i32, i64, p, p, p, i64, i64, p, p, p, p, i32, i32, p, p, p, p, sz, p]),
        "shpl_conv3x3_dgrad": (i32, [i32, i32, i64, i64, p, i64, i64, p, i64, p, i64, i64, p, i64, p, sz, p]),
        "shpl_conv3x3_dgrad_reuse": (i32, [i32, i32, i64, i64, p, i64, i64, p, i64, p, i64, i64, p, i64, p, sz,
                                           ctypes.POINTER(ShplCsr), p, sz, i32, p]),
        "shpl_conv3x3_wgrad_workspace_bytes": (i32, [i32, i32, i64, i64, i64, i64, i64, i64, psz]),
        "shpl_conv3x3_wgrad": (i32, [i32, i32, i64, i64, p, i64, i64, i64, p, i64, i64, i64,
                                     ctypes.POINTER(ShplCsr), p, p, i64, i64, p, p, sz, p]),
        "shpl_conv3x3_wgrad_reuse": (i32, [i32, i32, i64, i64, p, i64, i64, i64, p, i64, i64, i64,
                                           ctypes.POINTER(ShplCsr), p, p, i64, i64, p, p, sz, p, sz, i32, p]),
        "shpl_upconv3x3_workspace_bytes": (i32, [i32, i32, i64, i64, i64, i64, i64, i64, i32, psz]),
        "shpl_upconv3x3": (i32, [i32, i32, i64, i64, p, i64, i64, i64, p, i64, i64, i64,
                                 ctypes.POINTER(ShplCsr), p, p, i64, p, p, p, i32, p, i64, p, p, sz, p]),
        "shpl_upconv3x3_dgrad_workspace_bytes": (i32, [i32, i32, i64, i64, i64, i64, psz]),
        "shpl_upconv3x3_dgrad": (i32, [i32, i32, i64, i64, p, i64, i64, p, i64, p, i64, i64, p, i64, p, sz, p]),
        "shpl_upconv3x3_wgrad_workspace_bytes": (i32, [i32, i32, i64, i64, i64, i64, i64, i64, psz]),
        "shpl_upconv3x3_wgrad": (i32, [i32, i32, i64, i64, p, i64, i64, i64, p, i64, i64, i64,
                                       ctypes.POINTER(ShplCsr), p, p, i64, i64, p, p, sz, p]),
        "shpl_head1x1_workspace_bytes": (i32, [i32, i64, i64, i64, i64, i64, i32, psz]),
        "shpl_head1x1": (i32, [i32, i64, p, i64, i64, i64, p, i64, i64, i64, i64, ctypes.POINTER(ShplCsr), p, i64,
                               p, p, i64, p, sz, p]),
        "shpl_head1x1_dgrad": (i32, [i32, i64, p, i64, i64, p, i64, i64, p, i64, p, i64, i64,
                                     ctypes.POINTER(ShplCsr), p, sz, p]),
        "shpl_head1x1_wgrad_workspace_bytes": (i32, [i32, i64, i64, i64, i64, i64, i32, psz]),
        "shpl_head1x1_wgrad": (i32, [i32, i64, p, i64, i64, i64, p, i64, i64, i64, i64, ctypes.POINTER(ShplCsr), p,
                                     i64, i64, p, p, p, sz, p]),
        "shpl_dropout_mask": (i32, [i64, i64, d, u64, p, p]),
        "shpl_head1x1_drop_workspace_bytes": (i32, [i32, i64, i64, i64, i64, i64, i32, psz]),
        "shpl_head1x1_drop": (i32, [i32, i64, p, i64, i64, i64, p, i64, i64, i64, i64, ctypes.POINTER(ShplCsr), p,
                                    i64, p, p, i64, d, u64, p, sz, p]),
        "shpl_head1x1_drop_dgrad": (i32, [i32, i64, p, i64, i64, p, i64, i64, p, i64, p, i64, i64,
                                          ctypes.POINTER(ShplCsr), d, u64, p, sz, p]),
        "shpl_head1x1_drop_wgrad_workspace_bytes": (i32, [i32, i64, i64, i64, i64, i64, i32, psz]),
        "shpl_head1x1_drop_wgrad": (i32, [i32, i64, p, i64, i64, i64, p, i64, i64, i64, i64, ctypes.POINTER(ShplCsr),
                                          p, i64, i64, p, p, d, u64, p, sz, p]),
        "shpl_concat_bn_workspace_bytes": (i32, [i64, i64, i64, psz]),
        "shpl_concat_bn": (i32, [i32, i32, ctypes.POINTER(ShplCsr), p, i64, i64, i64, p, i64, i64, i64, p, i64, i32,
                                 ctypes.c_float, ctypes.c_float, p, p, p, p, p, p, p, p, sz, p]),
        "shpl_concat_bn_backward_workspace_bytes": (i32, [i64, i64, i64, psz]),
        "shpl_concat_bn_backward": (i32, [i32, i32, ctypes.POINTER(ShplCsr), ctypes.POINTER(ShplCsr), p, i64, i64, i64,
                                          p, i64, i64, i64, p, i64, p, p, i32, p, i64, p, p, i64, p, p, p, sz, p]),
    }
    for name, (res, args) in sig.items():
        f = getattr(lib, name)
        f.restype = res
        f.argtypes = args
    return sig


EXPORTED = None


def lib():
    """Load libshpl.so once; raise loudly if it is absent (no CPU fallback)."""
    global _lib, EXPORTED
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ShplLibraryError(
                f"{LIB_PATH} not found: build it with `python -m sparse_pooling_amd.build` "
                "(the SHPL path has no CPU fallback)")
        try:
            _lib = ctypes.CDLL(LIB_PATH)
        except OSError as e:
            raise ShplLibraryError(f"cannot load {LIB_PATH}: {e}") from e
        EXPORTED = sorted(_declare(_lib))
    return _lib


def check(rc, what):
    if rc != OK:
        msg = lib().shpl_status_string(rc).decode()
        raise ShplLibraryError(f"{what} failed: {msg} (status {rc})")


def ptr(t):
    """Device pointer of a tensor (NULL for None)."""
    if t is None:
        return None
    return ctypes.c_void_p(t.data_ptr())


def index_args(n_frames, point_offsets, point_counts, max_points, points, voxels, P, im_size, bv_size, stride, mval,
               cell, pix, val):
    """The twenty leading arguments shpl_build_index and shpl_build_index_buckets share."""
    return (n_frames, ptr(point_offsets), ptr(point_counts), int(max_points), ptr(points),
            F64 if points.dtype == torch.float64 else F32, ptr(voxels), I64 if voxels.dtype == torch.int64 else I32,
            int(voxels.stride(0)), ptr(P), float(im_size[0]), float(im_size[1]), float(bv_size[0]), float(bv_size[1]),
            float(stride[0]), float(stride[1]), ptr(mval), ptr(cell), ptr(pix), ptr(val))


def index_args_ragged(n_frames, point_offsets, point_counts, max_points, points, voxels, P, im_sizes, img_hw, bv_size,
                      stride, mval, cell, pix, val):
    """The twenty-one leading arguments shpl_build_index_ragged and shpl_build_index_buckets_ragged share:
    im_sizes [n_frames, 2] f64 on the device ((W, H) per frame), img_hw the padded map's (rows, cols)."""
    assert im_sizes.dtype == torch.float64 and im_sizes.is_contiguous() and im_sizes.numel() == 2 * n_frames
    lead = index_args(n_frames, point_offsets, point_counts, max_points, points, voxels, P, (0, 0), bv_size, stride,
                      mval, cell, pix, val)
    return lead[:10] + (ptr(im_sizes), int(img_hw[0]), int(img_hw[1])) + lead[12:]


# Row-keyed pulls (shpl_csr.key_range: one launch per pull) are the default for batches of fewer than ROWS_FRAMES
# frames with at most ROWS_MAX_KEYS destinations per frame: latency-bound layers (config 3). The range CSR carries
# entry offsets in 24 bits: capacities under ROWS_MAX_CAP slots.
ROWS_FRAMES, ROWS_MAX_KEYS, ROWS_MAX_CAP = 32, 65536, 1 << 24


def row_pulls(n_frames, keys_per_frame, nnz_cap):
    return n_frames < ROWS_FRAMES and keys_per_frame <= ROWS_MAX_KEYS and nnz_cap < ROWS_MAX_CAP


def stream_of(device=None):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def workspace(nbytes, device):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def ws_bytes(symbol, *args):
    """The size a ``<symbol>_workspace_bytes`` query of the library reports for these arguments (the size_t
    out-parameter is appended here); None, a pooling CSR's entry capacity without a pool, goes as -1."""
    out = ctypes.c_size_t()
    name = symbol + "_workspace_bytes"
    check(getattr(lib(), name)(*[-1 if a is None else int(a) for a in args], ctypes.byref(out)), name)
    return out.value


def index_ws_bytes(n_frames, max_points):
    return ws_bytes("shpl_build_index", n_frames, max_points)


def index_levels_ws_bytes(n_frames, max_points, n_levels):
    return ws_bytes("shpl_build_index_levels", n_frames, max_points, n_levels)


def index_levels(levels):
    """The host array shpl_build_index_levels takes: levels = [(stride, bv_size, cell, pix, val, mij, flip,
    frame_nnz)], tensors or None."""
    arr = (ShplIndexLevel * len(levels))()
    for a, (stride, bv_size, *tensors) in zip(arr, levels):
        a.s_img, a.s_bv, a.bv_h, a.bv_w = float(stride[0]), float(stride[1]), float(bv_size[0]), float(bv_size[1])
        a.cell, a.pix, a.val, a.mij, a.flip, a.frame_nnz = (_addr(t) for t in tensors)
    return arr


def index_level_maps(img_hws):
    """The host array level_img_hw of shpl_build_index_levels_ragged: [n_levels][2] i64, each level's padded image
    feature map as (img_rows, img_cols) in that level's strided pixels."""
    arr = (ctypes.c_int64 * (2 * len(img_hws)))()
    for l, (rows, cols) in enumerate(img_hws):
        arr[2 * l], arr[2 * l + 1] = int(rows), int(cols)
    return arr


def csr_ws_bytes(n_keys, nnz_cap):
    return ws_bytes("shpl_csr", n_keys, nnz_cap)


def dtype_code(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise TypeError(f"SHPL features must be float32 or bfloat16, got {t.dtype}")


def bucket_ws_bytes(n_frames, max_points, nnz_cap, cells_per_frame, pix_per_frame):
    return ws_bytes("shpl_bucket", n_frames, max_points, nnz_cap, cells_per_frame, pix_per_frame)


def bucket_workspace(n_frames, max_points, nnz_cap, cells_per_frame, pix_per_frame, device):
    """A bucket workspace for shpl_build_index_buckets, ZEROED: its frame barrier words must start at zero
    (include/shpl.h; every call leaves them so, and shpl_bucket_workspace_reset restores them after a
    SHPL_EBIT_BARRIER)."""
    nb = bucket_ws_bytes(n_frames, max_points, nnz_cap, cells_per_frame, pix_per_frame)
    return torch.zeros(max(int(nb), 256), dtype=torch.uint8, device=device)


def bucket_workspace_reset(n_frames, ws, device=None):
    """shpl_bucket_workspace_reset on the current stream."""
    check(lib().shpl_bucket_workspace_reset(int(n_frames), ptr(ws), ws.numel(), stream_of(device)),
          "shpl_bucket_workspace_reset")
