"""k_copy_rows: shpl_pull_dense over a concat without pooled channels (the pass-through copy alone), bit for bit
against torch slicing. The output starts as 0x5A bytes: the columns past the pass-through half (the pooled half
and any padding of the row) and everything past the last row must keep them.

k_copy_rows takes one chunk per thread (U = 1) in workgroups of 256, on a grid rounded up to a multiple of 8
whose workgroup ids are remapped; the row counts below put the end of the chunks one short of a workgroup, one
past it, inside the first workgroup, and far enough for more than 8 workgroups with idle ones at the end."""
import ctypes

import pytest
import torch

DEV = "cuda"
TAIL = 512  # bytes behind the last output row

# (dtype, channels): f32 4 / 8 / 64 chunks per row, 6 and 3 (the division instead of the shift), bf16 4 chunks
SHAPES = [("f32", 16), ("f32", 32), ("f32", 256), ("f32", 24), ("f32", 12), ("bf16", 32)]
# 31 * U + 1 = 32; at 3 chunks per row (f32 C = 12): 85 rows = 255 chunks and 1365 rows = 4095 chunks (the last
# workgroup one chunk short), 171 rows = 513 and 939 rows = 2817 chunks (one chunk over 2 and 11 workgroups:
# 12 workgroups on a grid of 16)
ROWS = [0, 1, 32, 85, 171, 939, 1365]


def _esz(dtype):
    return 2 if dtype == "bf16" else 4


def _run(dtype, C, rows, pass_stride=None, pass_off=0, out_stride=None, out_shift=0, c_pool=0):
    """shpl_pull_dense(CONCAT, c_pass = C, c_pool) over random source bytes into 0x5A bytes; returns (output
    rows as bytes [rows, out_stride * esz], the bytes behind them, the source rows as bytes)."""
    from sparse_pooling_amd import _lib as L
    esz = _esz(dtype)
    pass_stride = C if pass_stride is None else pass_stride
    out_stride = 2 * C if out_stride is None else out_stride
    g = torch.Generator(device="cpu").manual_seed(1000 * C + rows)
    src = torch.randint(0, 256, (max(rows, 1) * pass_stride * esz,), dtype=torch.uint8, generator=g).to(DEV)
    buf = torch.full((out_shift + rows * out_stride * esz + TAIL,), 0x5A, dtype=torch.uint8, device=DEV)
    csr = L.ShplCsr()
    csr.n_keys = rows
    rc = L.lib().shpl_pull_dense(L.BY_CELL, L.BF16 if dtype == "bf16" else L.F32, ctypes.byref(csr),
                                 L.ptr(src) if c_pool else None, pass_stride, 0, c_pool, L.ptr(src), pass_stride,
                                 pass_off, C, L.OUT_CONCAT, ctypes.c_void_p(buf.data_ptr() + out_shift), out_stride,
                                 L.stream_of(torch.device(DEV)))
    assert rc == L.OK
    torch.cuda.synchronize()
    assert bool((buf[:out_shift] == 0x5A).all())
    body = buf[out_shift:out_shift + rows * out_stride * esz].view(rows, out_stride * esz)
    return body, buf[out_shift + rows * out_stride * esz:], src[:rows * pass_stride * esz].view(rows, pass_stride * esz)


def _check(dtype, C, rows, **kw):
    esz = _esz(dtype)
    pass_off = kw.get("pass_off", 0)
    body, tail, src = _run(dtype, C, rows, **kw)
    assert torch.equal(body[:, :C * esz], src[:, pass_off * esz:(pass_off + C) * esz])
    assert bool((body[:, C * esz:] == 0x5A).all()), "bytes past the pass-through half were written"
    assert bool((tail == 0x5A).all()), "bytes past the last row were written"


@pytest.mark.gpu
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("dtype,C", SHAPES)
def test_copy_rows_16_byte_chunks(dtype, C, rows):
    _check(dtype, C, rows)


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [1, 32, 171, 1365])
@pytest.mark.parametrize("dtype,C,out_shift", [("f32", 6, 0), ("f32", 16, 4), ("bf16", 12, 0)])
def test_copy_rows_element_wise(dtype, C, out_shift, rows):
    """Rows that are no multiple of 16 bytes, or an output 4 bytes off a 16-byte boundary: one element per thread."""
    _check(dtype, C, rows, out_shift=out_shift)


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [1, 171, 1365])
@pytest.mark.parametrize("dtype,C,pass_stride,pass_off,out_stride", [
    ("f32", 32, 48, 8, None),    # a column slice of wider source rows, 16-byte chunks
    ("f32", 32, 48, 8, 72),      # ... into output rows with padding behind the pooled half
    ("f32", 32, 32, 0, 72),      # contiguous source, padded output rows
    ("f32", 12, 20, 4, 28),      # the same at 3 chunks per row
    ("f32", 16, 23, 3, 37),      # odd strides and offset: element-wise
    ("bf16", 32, 64, 16, 80),
    ("f32", 32, 32, 0, 32),      # contiguous output rows: no pooled half at all
])
def test_copy_rows_strides(dtype, C, pass_stride, pass_off, out_stride, rows):
    _check(dtype, C, rows, pass_stride=pass_stride, pass_off=pass_off, out_stride=out_stride)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,C,rows", [("f32", 32, 171), ("bf16", 32, 85), ("f32", 6, 32)])
def test_pooled_channels_keep_k_dense(dtype, C, rows):
    """A concat with pooled channels is still k_dense's: the pass-through half copied, the pooled half zero
    bits, the bytes behind the last row untouched."""
    esz = _esz(dtype)
    body, tail, src = _run(dtype, C, rows, c_pool=C)
    assert torch.equal(body[:, :C * esz], src)
    assert bool((body[:, C * esz:] == 0).all())
    assert bool((tail == 0x5A).all())
