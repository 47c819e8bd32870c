"""The wide bf16 conv (k_pack_wide, k_conv_wide of shpl_conv_wide.hip, and wide::prep under it), pinned in
every dispatch form on MI355X.

Every case asserts, before it runs, that the library's own predicate (``fc.wide_form``: shpl_conv3x3_wide_form,
the code conv_launch decides by) gives the form its table row names -- 1 wide with B dense or absent, 2 wide
over the compact pooled runs, 3 wide over the materialised pooled map, 0 not the wide kernel -- so a case that
fell to the tiled kernel would fail instead of passing a tolerance. Every case runs twice into separate outputs
and the two results agree bit for bit (the kernel orders its LDS-DMAs by hand: a race would otherwise show as a
rare tolerance failure). The SHA-256 of every output is held in tests/golden/conv_wide_bits.json
(tests/golden/make_conv_wide_bits.py).

Two kinds of data.

Exact ("x"): inputs are integers in [-3, 3], weights integers in [-2, 2], pool values in {+-0.5, +-1, +-2} over
runs of at most 10 entries, no scale or center, an integer shift. Every product and every partial sum is then
exact in f32 in any order and every pooled sum a multiple of 0.5 below 64, exact in bf16, so the output equals
``to_bf16_bits(oracle.conv3x3(...))`` bit for bit: no tolerance, and any dropped, doubled or misplaced term
shows. The premise (twice sum |x| |w| < 2^24 per output: the inputs may be odd multiples of 0.5) is asserted.
These digests come from the oracle alone ("pinned_to": "oracle"); tests/test_conv_wide_cases.py re-derives them
without a GPU.

Float ("f"): synth.make_features rounded to bf16, held to the bound of test_bf16_wide_conv_dense (imported:
_bound(x, w, scale) + |ref| 2^-8); digests recorded on the GPU ("pinned_to": "gpu").

The cases, each beside the form it reaches (Q input chunks of 64 channels, QA of them from A; tiles of 16 x 16):
dense-*      form 1. A only (128 + 0), 64 + 64 (Q = 2, both halo buffers live from the first chunk), 128 + 64 and
             64 + 128 (Q = 3, QA = 2 / 1), 256 + 256 (Q = 8, 72 steps); one and two output blocks; maps of 1 x 1
             (every halo piece from the zero piece), 16 x 16, 17 x 17, 1 x 40, 40 x 1, 3 frames of 16 x 40 (9 tiles)
             and 2 of 17 x 64 (16 tiles: two whole XCD rounds); the ten epilogues. Two sources are bitwise the
             conv of their concatenation.
view-*       raw ABI calls: A and B as channel slices of wider rows, out as a slice of wider rows prefilled with
             NaN. Offset 8: form 1, bitwise the contiguous call; offset 3: form 0 (the tiled kernel).
pooled-*     form 2. Cell-keyed and pixel-keyed (ent_col) over test_gpu_conv_tiled.dense_map, cell-keyed over
             hand_map below, an empty pool; each bitwise the conv of the materialised [a || pooled].
map-*        form 3: the 18433 x 3 map, the smallest past the occupancy table; the oracle on its first and last
             20 rows.
frame31-*    form 0: a frame whose rows end 2^31 bytes past its start. k_conv_wide keeps a lane's halo source
             as a signed 32-bit byte offset inside its frame; the shared predicate therefore hands such a call to
             the tiled kernel, which addresses in 64 bits. Its last two output rows equal those of the same conv
             over a contiguous crop of the last four rows (form 1), and the oracle.
"""
import collections
import ctypes
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from oracle import shpl_oracle as orc
from sparse_pooling_amd import synth
from test_gpu_conv import DEV, _assert_within, _bf16, _bound, _np, _t, _weights
from test_gpu_conv_tiled import dense_map

pytestmark = pytest.mark.gpu

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_wide_bits.json")
TILE, KC, NT = 16, 64, 256  # shpl_conv_wide: output tile, input channels per chunk, output channels per block
SENTINEL = -77.0            # exact in bf16
EPILOGUES = ("none", "shift", "scale", "center+scale", "all")
POOL_VALUES = np.array([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], np.float32)
HAND_SHAPE, SRC_HW = (2, 17, 70), (6, 7)
TALL_HW, TALL_SRC_HW, BAND = (18433, 3), (15, 17), 20
# frame31: 1025 x 256 pixels in rows of 4096 elements, (h w - 1) * stride * 2 = 2^31 + 2^21 - 8192 bytes
BIG_HW, BIG_STRIDE, BIG_CROP = (1025, 256), 4096, 4

# fn: the case function's name; form: what wide_form must answer; shape: (frames, h, w); kind: B's source -- "none",
# "dense", "cmp" (compact pooled runs), "map" (materialised); data: "x" exact / "f" float; extra: the function's own
Case = collections.namedtuple("Case", "fn form shape ca cb cout kind data epi relu extra")


def _rd(a):
    return orc.from_bf16_bits(orc.to_bf16_bits(a))


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from sparse_pooling_amd import _lib as L
    L.lib()
    assert torch.cuda.is_available()


# ------------------------------------------------------------------ the maps (no GPU)
def _entries(counts, rng, n_src_frame):
    """Cell-keyed reference-format entries of counts [F, H, W]: one column per entry on a source pixel of the
    same frame, grouped by frame and shuffled inside; values from POOL_VALUES."""
    F, H, W = counts.shape
    rows, col_pix, n_frame = [], [], []
    for f in range(F):
        r_f, p_f = [], []
        for t in np.flatnonzero(counts[f].reshape(-1)):
            n = int(counts[f].reshape(-1)[t])
            r_f += [f * H * W + int(t)] * n
            p_f += [int(s) + f * n_src_frame for s in rng.choice(n_src_frame, n, replace=False)]
        order = rng.permutation(len(r_f))
        rows += [r_f[i] for i in order]
        col_pix += [p_f[i] for i in order]
        n_frame.append(len(r_f))
    return np.asarray(rows, np.int64), np.asarray(col_pix, np.int64), n_frame


def _as_map(rows, col_pix, n_frame, counts, src_shape, rng):
    F, hs, ws = src_shape
    idx = np.stack([col_pix // (hs * ws), col_pix % (hs * ws) // ws, col_pix % ws], 1)
    mij = np.stack([rows, np.arange(len(rows), dtype=np.int64)], 1)
    return {"mij": np.ascontiguousarray(mij), "mval": rng.choice(POOL_VALUES, len(rows)),
            "idx": np.ascontiguousarray(idx), "counts": counts, "n_frame": n_frame, "img_shape": src_shape,
            "m_size": np.array([counts.size, len(rows)], np.int64)}


HAND_ROW, HAND_TILE, HAND_CORNER = 5, (16, 48), (15, 64)


@functools.lru_cache(maxsize=None)
def hand_map(seed=23):
    """A cell-keyed map onto 2 x 17 x 70 (source 2 x 6 x 7), runs of 1 .. 10 entries with values from POOL_VALUES.
    Frame 0 is empty, so frame 1's entry slots start at 0 and its run ranks count from its own first word. In
    frame 1: runs on x = 31 and x = 32 of row 5 (the last bit of an occupancy word and the first of the next); a
    run on the last pixel; row 0 fully occupied; the 18 x 18 halo of the tile at (16, 48) holds one run only, on
    its corner pixel (15, 64). test_conv_wide_cases.py asserts these on the map's entries."""
    rng = np.random.default_rng(seed)
    F, H, W = HAND_SHAPE
    counts = np.where(rng.random(HAND_SHAPE) < 0.3, rng.integers(1, 5, HAND_SHAPE), 0)
    counts[0] = 0
    counts[1, 0] = np.maximum(counts[1, 0], 1)
    counts[1, HAND_ROW, 31], counts[1, HAND_ROW, 32] = 2, 3
    counts[1, H - 1, W - 1] = 10
    (y0, x0), (cy, cx) = HAND_TILE, HAND_CORNER
    counts[1, y0 - 1:y0 + TILE + 1, x0 - 1:x0 + TILE + 1] = 0
    counts[1, cy, cx] = 1
    rows, col_pix, n_frame = _entries(counts, rng, SRC_HW[0] * SRC_HW[1])
    return _as_map(rows, col_pix, n_frame, counts, (F,) + SRC_HW, rng)


@functools.lru_cache(maxsize=None)
def tall_map(exact, seed=91):
    """The one-frame map onto 18433 x 3 of test_bf16_wide_fused_materialised_map, cell-keyed from a 15 x 17 image:
    400 entries at random cells, every cell of the first and the last row among them, one cell with 10."""
    rng = np.random.default_rng(seed)
    (H, W), (hs, ws) = TALL_HW, TALL_SRC_HW
    R, n = H * W, 300
    rows = rng.integers(0, R, n)
    rows[:6] = [0, 1, 2, R - 3, R - 2, R - 1]
    rows[100:110] = rows[100]
    col_pix = rng.integers(0, hs * ws, n)
    extra = rng.integers(0, n, 100)  # 100 more entries on columns already there
    rows, col_pix = np.concatenate([rows, rng.integers(0, R, 100)]), np.concatenate([col_pix, col_pix[extra]])
    order = rng.permutation(len(rows))
    rows, col_pix = rows[order].astype(np.int64), col_pix[order].astype(np.int64)
    counts = np.bincount(rows, minlength=R).reshape(1, H, W)
    assert counts[0, 0].all() and counts[0, -1].all() and counts.max() >= 10
    m = _as_map(rows, col_pix, [len(rows)], counts, (1, hs, ws), rng)
    if not exact:
        m["mval"] = rng.uniform(-2, 2, len(rows)).astype(np.float32)
    return m


def exact_dense_map(swapped):
    """test_gpu_conv_tiled.dense_map (runs of 1 .. 6 entries) with its values replaced from POOL_VALUES."""
    m = dict(dense_map(swapped))
    m["mval"] = np.random.default_rng(29).choice(POOL_VALUES, len(m["mval"]))
    return m


def case_map(c):
    """(the map of a pooled case, its key)."""
    if c.fn == "materialised":
        return tall_map(c.data == "x"), "cell"
    which, key = c.extra["map"], c.extra["key"]
    if which == "hand":
        return hand_map(), key
    return (exact_dense_map(key == "pixel") if c.data == "x" else dense_map(key == "pixel")), key


def pooled_x(m, key, a, b):
    """The oracle's [a || pooled b] over a's map, rounded to bf16 (f32 array)."""
    ca, cb = a.shape[-1], b.shape[-1]
    if key == "cell":
        ref, _ = orc.sparse_pool_layer(a.reshape(1, -1, a.shape[2], ca), b, m["mij"], m["mval"], m["m_size"], m["idx"])
    else:
        _, ref = orc.sparse_pool_layer(b.reshape(1, -1, b.shape[2], cb), a, m["mij"], m["mval"], m["m_size"],
                                       m["idx"], dual=True)
    return _rd(ref.reshape(a.shape[:3] + (ca + cb,)))


# ------------------------------------------------------------------ inputs and references (no GPU)
def _ints(shape, seed, k):
    return np.random.default_rng(seed).integers(-k, k + 1, shape).astype(np.float32)


def _features(c, shape, seed):
    return _ints(shape, seed, 3) if c.data == "x" else _rd(synth.make_features(shape, seed))


def b_shape(c):
    """The shape of B's tensor: the map's for a dense B, the pooled source's otherwise."""
    if c.kind in ("none", "dense"):
        return c.shape + (c.cb,)
    if c.fn == "empty_pool":
        return (1,) + SRC_HW + (c.cb,)
    m, key = case_map(c)
    return (tuple(m["img_shape"]) if key == "cell" else (c.shape[0],) + SRC_HW) + (c.cb,)


def epilogue(c):
    """(center, scale, shift) of c.epi; exact cases know "none" and an integer shift."""
    rng = np.random.default_rng(104)
    if c.data == "x":
        assert c.epi in ("none", "shift")
        return None, None, (rng.integers(-4, 5, c.cout).astype(np.float32) if c.epi == "shift" else None)
    center = rng.standard_normal(c.cout).astype(np.float32) * 0.1
    scale = rng.uniform(0.5, 2.0, c.cout).astype(np.float32)
    shift = rng.standard_normal(c.cout).astype(np.float32) * 0.5
    return {"none": (None, None, None), "shift": (None, None, shift), "scale": (None, scale, None),
            "center+scale": (center, scale, None), "all": (center, scale, shift)}[c.epi]


def inputs(c):
    """(a, b or None, w, (center, scale, shift)) as f32 arrays holding bf16 values (frame31: big_blocks() for a, b)."""
    a = _features(c, c.shape + (c.ca,), 101) if c.fn != "frame31" else None
    b = _features(c, b_shape(c), 102) if c.cb and c.fn != "frame31" else None
    w = _ints((3, 3, c.ca + c.cb, c.cout), 103, 2) if c.data == "x" else _rd(_weights(c.ca + c.cb, c.cout, 103))
    if c.cout > NT:  # block 1's weights are its own
        assert not np.array_equal(w[..., :NT], w[..., NT:2 * NT])
    return a, b, w, epilogue(c)


def conv_x(c, a, b):
    """The conv's whole input [a || B] as the oracle reads it."""
    if c.kind == "none":
        return a
    if c.kind == "dense":
        return np.concatenate([a, b], -1)
    if c.fn == "empty_pool":
        return np.concatenate([a, np.zeros(a.shape[:3] + (c.cb,), np.float32)], -1)
    return pooled_x(*case_map(c), a, b)


def exact_premise(x, w):
    """Every product and partial sum of the conv is exact in f32 in any order: x in whole halves, w whole, and
    twice sum |x| |w| below 2^24 at every output."""
    assert np.array_equal(2 * x, np.round(2 * x)) and np.array_equal(w, np.round(w))
    _, ab = orc.conv3x3(np.abs(x), np.abs(w), raw=True)
    assert 2.0 * ab.max() < 2.0 ** 24
    return ab


def bands(x):
    """The first and the last BAND rows of a tall map with their halo row: ((rows of x, rows of the result) ..)."""
    H = x.shape[1]
    return ((slice(0, BAND + 1), slice(0, BAND)), (slice(H - BAND - 1, H), slice(1, BAND + 1)))


def big_blocks():
    """frame31's data: every image row repeats one [w, 128] block of integers, the last BIG_CROP rows their own."""
    w = BIG_HW[1]
    return _ints((w, 2 * KC), 111, 3), _ints((BIG_CROP, w, 2 * KC), 112, 3)


def references(c):
    """{output name: (oracle result f32, x, the rows of x's conv it holds)}: what the case's outputs are held to."""
    a, b, w, epi = inputs(c)
    if c.fn == "frame31":
        x = big_blocks()[1][None]
        ref = orc.conv3x3(x, w, *epi, c.relu)
        return {"last2": (ref[:, -2:], x, slice(BIG_CROP - 2, BIG_CROP))}
    x = conv_x(c, a, b)
    if c.fn == "materialised":
        out = {}
        for name, (rows, keep) in zip(("first", "last"), bands(x)):
            out[name] = (orc.conv3x3(x[:, rows], w, *epi, c.relu)[:, keep], x[:, rows], keep)
        return out
    return {"y": (orc.conv3x3(x, w, *epi, c.relu), x, slice(None))}


def oracle_bits(c):
    """{output name: bf16 bits} of an exact case, from the oracle alone."""
    assert c.data == "x"
    _, _, w, _ = inputs(c)
    out = {}
    for name, (ref, x, _) in references(c).items():
        exact_premise(x, w)
        out[name] = orc.to_bf16_bits(ref)
    return out


def sha(bits):
    return hashlib.sha256(np.ascontiguousarray(bits).tobytes()).hexdigest()


def reach(c):
    """(Q, QA, B's source, output blocks) of a case."""
    return (c.ca + c.cb) // KC, c.ca // KC, c.kind, c.cout // NT


def abi_call(c):
    """The arguments tests/golden/make_conv_host_plan.py's wide_form takes for this case's call."""
    F, H, W = c.shape
    kw = dict(c.extra.get("abi", {}), act=int(c.relu))
    if c.fn == "view":
        off = c.extra["off"]
        kw.update(a_off=off, a_stride=c.ca + 16, b_off=off, b_stride=c.cb + 16, out_stride=c.cout + 8)
    if c.kind in ("cmp", "map"):
        kw["pool"] = 0 if c.fn == "empty_pool" else len(case_map(c)[0]["mij"])  # the entry capacity
    return (F, H, W, c.ca, c.cb, c.cout), kw


# ------------------------------------------------------------------ on the GPU
def _bits(y):
    return _np(y.contiguous().view(torch.int16)).view(np.uint16)


def _same(y1, y2):
    return torch.equal(y1.contiguous().view(torch.int16), y2.contiguous().view(torch.int16))


def _f32(v):
    return None if v is None else _t(v)


def _conv(c, ta, tw, epi, tb=None, pool=None, foff=None, form=None, twice=True):
    """conv3x3 after the form assertion; twice: into two outputs that must agree."""
    from sparse_pooling_amd import fusion_conv as fc
    want = c.form if form is None else form
    assert fc.wide_form(ta, tw, b=tb, pool=pool, frame_off=foff, relu=c.relu) == want
    kw = dict(b=tb, pool=pool, frame_off=foff, center=_f32(epi[0]), scale=_f32(epi[1]), shift=_f32(epi[2]),
              relu=c.relu)
    y = fc.conv3x3(ta, tw, **kw)
    if twice:
        assert _same(y, fc.conv3x3(ta, tw, **kw))
    return y


def _held(c, outs, w, epi):
    """Every output against its reference: bit for bit (exact) or within the bound of test_bf16_wide_conv_dense."""
    for name, (ref, x, keep) in references(c).items():
        if c.data == "x":
            exact_premise(x, w)
            np.testing.assert_array_equal(_bits(outs[name]), orc.to_bf16_bits(ref))
        else:
            bound = _bound(x, w, epi[1])[:, keep] + np.abs(ref) * 2.0 ** -8
            _assert_within(outs[name].float(), ref, bound)
    return outs


def case_dense(c):
    a, b, w, epi = inputs(c)
    tw = _bf16(w)
    y = _conv(c, _bf16(a), tw, epi, tb=None if b is None else _bf16(b))
    if b is not None:  # two sources == their concatenation (the same 64-channel chunks)
        assert _same(y, _conv(c, _bf16(np.concatenate([a, b], -1)), tw, epi, twice=False))
    if c.extra.get("zeros"):  # the ReLU's sign test on the packed bf16: exact zeros and negatives before it
        _, raw = orc.conv3x3(conv_x(c, a, b), w, raw=True)
        pre = raw + epi[2]
        assert c.relu and (pre == 0).any() and (pre < 0).any() and (pre > 0).any()
    return _held(c, {"y": y}, w, epi)


def _in_view(t, off, extra=16):
    """t's channels at [off, off + C) of a buffer whose rows are C + extra wide, the sentinel elsewhere."""
    buf = torch.full(tuple(t.shape[:-1]) + (t.shape[-1] + extra,), SENTINEL, dtype=t.dtype, device=t.device)
    buf[..., off:off + t.shape[-1]] = t
    return buf


def case_view(c):
    """Raw shpl_conv3x3 calls: A and B at channel offset `off` of rows 16 channels wider, out at column 8 of rows
    8 channels wider, prefilled with NaN."""
    from sparse_pooling_amd import _lib as L, fusion_conv as fc
    a, b, w, epi = inputs(c)
    off, (F, H, W) = c.extra["off"], c.shape
    ta, tb, tw, shift = _bf16(a), _bf16(b), _bf16(w), _f32(epi[2])
    assert epi[0] is None and epi[1] is None
    va, vb = _in_view(ta, off), _in_view(tb, off)
    lib, act = L.lib(), L.ACT_RELU if c.relu else L.ACT_NONE
    ws = L.workspace(L.ws_bytes("shpl_conv3x3", L.BF16, F, H, W, c.ca, c.cb, c.cout, None, False), DEV)
    outs = []
    for _ in range(2):
        buf = torch.full((F, H, W, c.cout + 8), float("nan"), dtype=torch.bfloat16, device=DEV)
        out = ctypes.c_void_p(buf.data_ptr() + 16)
        head = (L.BF16, F, H, W, L.ptr(va), c.ca + 16, off, c.ca, L.ptr(vb), c.cb + 16, off, c.cb, None, None,
                L.ptr(tw), c.cout)
        form = ctypes.c_int(-1)
        L.check(lib.shpl_conv3x3_wide_form(*head, act, out, c.cout + 8, 0, ctypes.byref(form)), "wide_form")
        assert form.value == c.form
        L.check(lib.shpl_conv3x3(*head, None, None, L.ptr(shift), act, out, c.cout + 8, None, L.ptr(ws), ws.numel(),
                                 L.stream_of(buf.device)), "shpl_conv3x3")
        assert bool(torch.isnan(buf[..., :8]).all()) and not bool(torch.isnan(buf[..., 8:]).any())
        outs.append(buf[..., 8:])
    assert _same(outs[0], outs[1])
    for v, t in ((va, ta), (vb, tb)):  # the sources as they were
        assert _same(v, _in_view(t, off))
    if c.form:  # the same kernel over the same chunks: bitwise the contiguous call
        assert _same(outs[0], _conv(c, ta, tw, epi, tb=tb, twice=False))
    return _held(c, {"y": outs[0].contiguous()}, w, epi)


def _smap(m, n_frames):
    """The device map of m: packed as one frame, then its entry slots cut by frame."""
    from sparse_pooling_amd import shpl_map as sm
    p = sm.pack_map(_t(m["mij"]), _t(m["mval"]), m["m_size"], _t(m["idx"]), m["img_shape"])
    off = torch.tensor(np.concatenate([[0], np.cumsum(m["n_frame"])]), dtype=torch.int64, device=DEV)
    return sm.ShplMap(p.cell, p.col, p.val, p.pix, p.nnz_cap, p.n_cells, p.n_pix, p.n_cols, DEV, frame_off=off,
                      n_frames=n_frames, err=p.err)


def case_pooled(c):
    """Forms 2 and 3: fused over the CSR == the conv of the materialised [a || pooled], which is the oracle's."""
    from sparse_pooling_amd import _lib as L, shpl_map as sm
    a, b, w, epi = inputs(c)
    m, key = case_map(c)
    ta, tb, tw = _bf16(a), _bf16(b), _bf16(w)
    smap = _smap(m, c.shape[0])
    if key == "cell":
        pool = smap.csr(L.BY_CELL, L.ORDER_ENTRY)
        mat = sm.pool_img_to_bev(smap, tb, ta.shape, bev=ta)
    else:
        pool = smap.csr(L.BY_PIXEL, L.ORDER_COL_ROW)
        assert pool.ent_col is not None
        mat = sm.pool_bev_to_img(smap, tb, ta.shape, img=ta)
    x = conv_x(c, a, b)
    if c.data == "x":  # every pooled sum is exact in bf16
        assert np.abs(x[..., c.ca:]).max() < 64 and (x[..., c.ca:] != 0).any()
    torch.cuda.synchronize()
    assert smap.error_bits() == 0
    np.testing.assert_array_equal(_np(mat.float()), x)
    y = _conv(c, ta, tw, epi, tb=tb, pool=pool, foff=smap.frame_off)
    yu = _conv(c, mat[..., :c.ca].contiguous(), tw, epi, tb=mat[..., c.ca:].contiguous(), form=1, twice=False)
    assert _same(y, yu)
    if c.fn != "materialised":
        return _held(c, {"y": y}, w, epi)
    outs = _held(c, {"first": y[:, :BAND], "last": y[:, -BAND:]}, w, epi)
    return outs if c.data == "x" else dict(outs, y=y)


def case_empty_pool(c):
    """nnz_cap == 0: no run, the occupancy words all clear -- bitwise the dense conv over a zero B."""
    from sparse_pooling_amd import _lib as L, shpl_map as sm
    a, b, w, epi = inputs(c)
    ta, tb, tw = _bf16(a), _bf16(b), _bf16(w)
    smap = sm.pack_map(torch.zeros((0, 2), dtype=torch.int64, device=DEV), torch.zeros(0, device=DEV),
                       [a.shape[1] * a.shape[2], 0], torch.zeros((0, 3), dtype=torch.int32, device=DEV), b.shape)
    pool = smap.csr(L.BY_CELL, L.ORDER_ENTRY)
    assert pool.nnz_cap == 0 and c.shape[0] == 1
    y = _conv(c, ta, tw, epi, tb=tb, pool=pool, foff=smap.frame_off)
    zero = torch.zeros(ta.shape[:3] + (c.cb,), dtype=torch.bfloat16, device=DEV)
    assert _same(y, _conv(c, ta, tw, epi, tb=zero, form=1, twice=False))
    return _held(c, {"y": y}, w, epi)


def big_frame_rows(c, form_big=None):
    """frame31's two results: the last two output rows of the conv over the strided frame, and of the conv over
    a contiguous crop of its last BIG_CROP rows. A is channels [0, 64) and B channels [64, 128) of one buffer
    of BIG_STRIDE-element rows. form_big: what wide_form must answer for the strided call (None: not asked)."""
    from sparse_pooling_amd import _lib as L
    (H, W), S = BIG_HW, BIG_STRIDE
    assert (H * W - 1) * S * 2 >= 2 ** 31 and H * W * S * 2 < 2 ** 32 and c.shape == (1, H, W)
    _, _, w, epi = inputs(c)
    block, last = big_blocks()
    tw, shift = _bf16(w), _f32(epi[2])
    buf = torch.empty((H, W, S), dtype=torch.bfloat16, device=DEV)
    buf[..., 2 * KC:4 * KC] = SENTINEL  # the channels beside the two sources
    buf[..., :2 * KC] = _bf16(block)[None]
    buf[H - BIG_CROP:, :, :2 * KC] = _bf16(last)
    lib, act = L.lib(), L.ACT_RELU if c.relu else L.ACT_NONE
    head = (L.BF16, 1, H, W, L.ptr(buf), S, 0, c.ca, L.ptr(buf), S, c.ca, c.cb, None, None, L.ptr(tw), c.cout)
    ws = L.workspace(L.ws_bytes("shpl_conv3x3", L.BF16, 1, H, W, c.ca, c.cb, c.cout, None, False), DEV)
    last2 = []
    for _ in range(2):
        out = torch.empty((1, H, W, c.cout), dtype=torch.bfloat16, device=DEV)
        if form_big is not None:
            form = ctypes.c_int(-1)
            L.check(lib.shpl_conv3x3_wide_form(*head, act, L.ptr(out), c.cout, 0, ctypes.byref(form)), "wide_form")
            assert form.value == form_big
        L.check(lib.shpl_conv3x3(*head, None, None, L.ptr(shift), act, L.ptr(out), c.cout, None, L.ptr(ws),
                                 ws.numel(), L.stream_of(buf.device)), "shpl_conv3x3")
        last2.append(out[:, -2:].clone())
    assert _same(*last2)
    crop = buf[H - BIG_CROP:, :, :2 * KC][None]
    y_crop = _conv(c, crop[..., :KC].contiguous(), tw, epi, tb=crop[..., KC:].contiguous(), form=1)
    return last2[0], y_crop[:, -2:]


def case_frame31(c):
    big, crop = big_frame_rows(c, form_big=c.form)
    assert _same(big, crop)
    _, _, w, epi = inputs(c)
    return _held(c, {"last2": big}, w, epi)


FNS = {"dense": case_dense, "view": case_view, "pooled": case_pooled, "materialised": case_pooled,
       "empty_pool": case_empty_pool, "frame31": case_frame31}


def _case(fn, form, shape, ca, cb, cout, data, epi="none", relu=False, kind=None, **extra):
    kind = kind or ("dense" if cb else "none")
    name = "%s-%s-%d+%d-%d-%s-%s%s" % (fn, data, ca, cb, cout, "x".join(str(s) for s in shape), epi,
                                       "-relu" if relu else "")
    for k in ("map", "key", "off"):
        if k in extra:
            name += "-%s%s" % ("off" if k == "off" else "", extra[k])
    assert name not in CASES, name
    CASES[name] = Case(fn, form, tuple(shape), ca, cb, cout, kind, data, epi, relu, extra)


CASES = {}
# k_conv_wide, B dense or absent. Sources and tiles, exact:
_case("dense", 1, (1, 1, 1), 128, 0, 256, "x")                                    # every halo piece the zero piece
_case("dense", 1, (1, 16, 16), 128, 0, 256, "x", "shift", True, zeros=True)       # one whole tile; the ReLU's sign test
_case("dense", 1, (1, 17, 17), 64, 64, 256, "x", "none", True)                    # Q = 2; four tiles, three 1 wide / high
_case("dense", 1, (1, 1, 40), 128, 64, 256, "x", "shift")                         # Q = 3, QA = 2
_case("dense", 1, (1, 40, 1), 64, 128, 256, "x", "shift", True)                   # Q = 3, QA = 1
_case("dense", 1, (1, 17, 19), 256, 256, 256, "x")                                # Q = 8: 72 steps
_case("dense", 1, (3, 16, 40), 64, 64, 512, "x", "shift", True)                   # 9 tiles, two output blocks
_case("dense", 1, (2, 17, 64), 64, 64, 256, "x")                                  # 16 tiles
# the same forms on float data
_case("dense", 1, (1, 1, 1), 128, 0, 256, "f", "shift")
_case("dense", 1, (1, 16, 16), 128, 0, 512, "f", "all", True)
_case("dense", 1, (1, 17, 17), 128, 64, 256, "f", "shift", True)
_case("dense", 1, (1, 1, 40), 64, 128, 256, "f", "scale")
_case("dense", 1, (1, 40, 1), 64, 64, 256, "f", "center+scale", True)
_case("dense", 1, (1, 17, 19), 256, 256, 256, "f", "shift", True)
_case("dense", 1, (3, 16, 40), 64, 64, 512, "f", "all")
# every epilogue with and without the ReLU
for _epi in EPILOGUES:
    for _relu in (False, True):
        _case("dense", 1, (2, 17, 33), 64, 64, 256, "f", _epi, _relu)
# views
_case("view", 1, (2, 17, 33), 64, 64, 256, "x", "shift", True, off=8)
_case("view", 1, (2, 17, 33), 64, 64, 256, "f", "shift", True, off=8)
_case("view", 0, (2, 17, 33), 64, 64, 256, "f", "shift", True, off=3)             # off the 16-byte grid: tiled
# wide::prep + k_conv_wide over the compact pooled runs
for _key in ("cell", "pixel"):
    _case("pooled", 2, (2, 10, 40), 64, 64, 256, "x", "shift", True, kind="cmp", map="dense", key=_key)
_case("pooled", 2, (2, 10, 40), 128, 64, 256, "f", "shift", True, kind="cmp", map="dense", key="cell")
_case("pooled", 2, (2, 10, 40), 64, 128, 256, "f", "all", True, kind="cmp", map="dense", key="pixel")
_case("pooled", 2, HAND_SHAPE, 64, 64, 256, "x", "none", False, kind="cmp", map="hand", key="cell")
_case("pooled", 2, HAND_SHAPE, 64, 64, 512, "f", "shift", True, kind="cmp", map="hand", key="cell")
_case("empty_pool", 2, (1, 17, 33), 64, 64, 256, "x", "shift", True, kind="cmp")
_case("empty_pool", 2, (1, 17, 33), 64, 64, 256, "f", "shift", True, kind="cmp")
# shpl_pull into the workspace + k_conv_wide over the map
_case("materialised", 3, (1,) + TALL_HW, 64, 64, 256, "x", "shift", True, kind="map")
_case("materialised", 3, (1,) + TALL_HW, 64, 64, 256, "f", "shift", True, kind="map")
# the tiled kernel for a frame past k_conv_wide's 31-bit offsets
_case("frame31", 0, (1,) + BIG_HW, 64, 64, 256, "x", "shift", True,
      abi=dict(a_stride=BIG_STRIDE, b_stride=BIG_STRIDE, b_off=KC))


def digest(t):
    """SHA-256 of a bf16 tensor's bytes."""
    return sha(_bits(t.detach()))


def run_case(name):
    """{output name: digest} of a case, after its form, determinism, identity and oracle assertions."""
    c = CASES[name]
    outs = FNS[c.fn](c)
    torch.cuda.synchronize()
    return {k: digest(v) for k, v in outs.items()}


@functools.lru_cache(maxsize=None)
def table():
    with open(TABLE) as fh:
        return json.load(fh)


def test_table_lists_every_case():
    assert sorted(table()) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_wide_case(name):
    assert run_case(name) == table()[name]["digests"]
