"""Kept zeros: shpl_pull_clear alone, and FusedPipeline's kept-zeros steps (bv_fused's pooled half kept zero
between steps, only the previous step's cells cleared) against the CPU oracle. Everything is compared bit for
bit: the zeros are k_dense's +0 and the sums are k_sparse's."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import shpl_oracle as orc
from sparse_pooling_amd import synth

DEV = "cuda"
B = 3
# CONFIG1's geometry (2,000 points, stride 4: BEV 176x200) at 32 + 32 channels
SPEC32 = synth.FrameSpec(2000, synth.CONFIG1.im_size, synth.CONFIG1.bv_size, synth.CONFIG1.stride, 32, 32)
N_OUT = 10     # points per frame the clip drops: empty slots (dst = -1) in every frame's capacity
LONG = 12      # points of one frame moved onto one voxel: a run longer than k_sparse's 8 entries


def _np(t):
    return t.detach().cpu().numpy()


def _oracle_frame(fr):
    gen = orc.gen_sparse_pooling_input_avod(fr.points, fr.voxel_indices, fr.P, list(fr.spec.im_size),
                                            tuple(fr.spec.bv_size))
    return orc.produce_sparse_pooling_input(gen, stride=fr.spec.stride)


@functools.lru_cache(maxsize=None)
def _case(k):
    """Step k's frames (their own seeds) and the oracle's index of each; in the even steps one frame carries
    a run of LONG entries on one cell (a different frame and cell each time)."""
    frames = [synth.make_frame(SPEC32, seed=400 + 10 * k + f, n_outside=N_OUT) for f in range(B)]
    if k % 2 == 0:
        vox = frames[(k // 2) % B].voxel_indices
        vox[:LONG + N_OUT] = vox[0]
    return frames, [_oracle_frame(fr) for fr in frames]


def _cells(k):
    """The occupied (frame, cell) rows of step k, from the oracle's index."""
    _, refs = _case(k)
    return [set(np.unique(r["Mij_pool"][:int(r["M_size"][1]), 0]).tolist()) for r in refs]


@functools.lru_cache(maxsize=None)
def _features(dtype):
    Hb, Wb = SPEC32.bev_feat_hw
    Hi, Wi = SPEC32.img_feat_hw
    bev = synth.make_features((B, Hb, Wb, SPEC32.c_bev), 11)
    img = synth.make_features((B, Hi, Wi, SPEC32.c_img), 12)
    if dtype == "bf16":
        bev, img = (orc.from_bf16_bits(orc.to_bf16_bits(a)) for a in (bev, img))
    return bev, img


@functools.lru_cache(maxsize=None)
def _expected_bits(k, dtype):
    """The oracle's bv_fused of step k as bits (u32 of f32, u16 of bf16)."""
    bev, img = _features(dtype)
    _, refs = _case(k)
    out = []
    for f, ref in enumerate(refs):
        eb, _ = orc.sparse_pool_layer(bev[f:f + 1], img[f:f + 1], ref["Mij_pool"], ref["M_val"], ref["M_size"],
                                      ref["img_index_flip_pool"])
        out.append(eb)
    eb = np.ascontiguousarray(np.concatenate(out, axis=0), np.float32)
    return orc.to_bf16_bits(eb) if dtype == "bf16" else eb.view(np.uint32)


def _bits(t):
    if t.dtype == torch.bfloat16:
        return _np(t.view(torch.int16)).view(np.uint16)
    return _np(t).view(np.uint32)


def _same(pl, k, dtype):
    torch.cuda.synchronize()
    assert int(pl.err.item()) == 0
    np.testing.assert_array_equal(_bits(pl.bv_fused), _expected_bits(k, dtype))


class _Run:
    """A 3-frame pipeline over SPEC32 (not row-keyed: config 2's launches, which so few frames would not pick
    by themselves) with device input buffers that step k's frames are copied into."""

    def __init__(self, dtype, **kw):
        kw.setdefault("rows", False)
        from sparse_pooling_amd import pipeline
        self.pipeline = pipeline
        self.dtype = dtype
        frames, _ = _case(0)
        self.pts, self.vox, self.off, self.P, maxp, N = pipeline.stack_frames(frames, DEV)
        tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
        self.pl = pipeline.FusedPipeline(B, maxp, N, SPEC32.im_size, SPEC32.bv_size, SPEC32.stride, SPEC32.c_bev,
                                         SPEC32.c_img, dtype=tdt, **kw)
        bev, img = _features(dtype)
        self.tb, self.ti = torch.from_numpy(bev).to(DEV).to(tdt), torch.from_numpy(img).to(DEV).to(tdt)
        self.side = torch.cuda.Stream(device=DEV)

    def load(self, k):
        pts, vox, off, P, _, _ = self.pipeline.stack_frames(_case(k)[0], DEV)
        assert torch.equal(off, self.off)  # every step's frames have the same sizes
        for dst, src in ((self.pts, pts), (self.vox, vox), (self.P, P)):
            dst.copy_(src)

    def overlapped(self):
        self.pl.step_overlapped(self.pts, self.vox, self.off, self.P, self.tb, self.ti, self.side)

    def plain(self):
        self.pl.step(self.pts, self.vox, self.off, self.P, self.tb, self.ti)


# ---------------------------------------------------------------- the sequence's own properties (CPU)

def test_sequence_has_long_runs_and_leftover_cells():
    """What the steps below rely on, from the oracle's index alone: a destination with more than 8 entries in
    the sequence (k_sparse_long's runs: the clear must take them too), and at least 100 cells occupied in step k
    that step k + 1 leaves empty (stale sums if they were not cleared)."""
    longest = 0
    for k in range(4):
        _, refs = _case(k)
        longest = max(longest, max(np.unique(r["Mij_pool"][:int(r["M_size"][1]), 0], return_counts=True)[1].max()
                                   for r in refs))
        left = sum(len(a - b) for a, b in zip(_cells(k), _cells(k + 1)))
        assert left >= 100, (k, left)
    assert longest > 8, longest


# ---------------------------------------------------------------- shpl_pull_clear alone

def _built_csr(spec, n_points, n_outside, frames=2):
    """A cell-keyed CSR of `frames` frames (FusedPipeline's index build and CSR build) and the oracle's
    occupied rows."""
    from sparse_pooling_amd import pipeline
    fs = synth.FrameSpec(n_points, spec.im_size, spec.bv_size, spec.stride, spec.c_bev, spec.c_img)
    frs = [synth.make_frame(fs, seed=70 + f, n_outside=n_outside) for f in range(frames)]
    pts, vox, off, P, maxp, N = pipeline.stack_frames(frs, DEV)
    pl = pipeline.FusedPipeline(frames, maxp, N, fs.im_size, fs.bv_size, fs.stride, fs.c_bev, fs.c_img, rows=False)
    pl.build_index(pts, vox, off, P)
    pl.build_csr(("cell",))
    torch.cuda.synchronize()
    assert int(pl.err.item()) == 0
    R = pl.Hb * pl.Wb
    rows = []
    for f, fr in enumerate(frs):
        ref = _oracle_frame(fr)
        rows.append(np.unique(ref["Mij_pool"][:int(ref["M_size"][1]), 0]) + f * R)
    return pl, np.concatenate(rows).astype(np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,c_pool,out_off,out_stride,n_points,n_outside", [
    ("f32", 16, 16, 32, 2000, 0),     # 16-byte chunks, the concat's layout
    ("f32", 32, 32, 68, 2000, 0),     # padding after the pooled columns
    ("bf16", 32, 32, 72, 2000, 0),    # 8 bf16 per chunk
    ("f32", 6, 6, 13, 2000, 0),       # the 1-element form
    ("f32", 16, 2, 19, 2000, 0),      # 16-byte-able channels at an unaligned offset: the 1-element form
    ("f32", 16, 16, 32, 2000, 40),    # capacity above the entries: empty slots (dst = -1)
    ("bf16", 32, 32, 64, 0, 30),      # a built CSR with no entry at all
])
def test_pull_clear_zeroes_exactly_the_csr_rows(dtype, c_pool, out_off, out_stride, n_points, n_outside):
    """Over 0x5A5A5A5A: after shpl_pull_clear exactly the pooled chunks of the CSR's rows are zero bits; the
    pass-through columns, the rows without an entry and the padding keep the pattern."""
    from sparse_pooling_amd import _lib as L
    pl, rows = _built_csr(synth.CONFIG1, n_points, n_outside)
    dst = _np(pl.csr.ent_dst)
    np.testing.assert_array_equal(np.unique(dst[dst >= 0]), rows)  # the CSR names the oracle's rows
    if n_outside:
        assert (dst == -1).sum() >= 2 * n_outside
    if n_points == 0:
        assert rows.size == 0 and (dst == -1).all()
    esz = 2 if dtype == "bf16" else 4
    buf = torch.full((pl.n_cells * out_stride * esz,), 0x5A, dtype=torch.uint8, device=DEV)
    rc = L.lib().shpl_pull_clear(L.BF16 if dtype == "bf16" else L.F32, pl.csr.ref(), c_pool, L.ptr(buf), out_stride,
                                 out_off, L.stream_of(torch.device(DEV)))
    assert rc == L.OK
    torch.cuda.synchronize()
    want = np.full((pl.n_cells, out_stride * esz), 0x5A, dtype=np.uint8)
    want[rows, out_off * esz:(out_off + c_pool) * esz] = 0
    np.testing.assert_array_equal(_np(buf).reshape(pl.n_cells, out_stride * esz), want)


@pytest.mark.gpu
def test_pull_clear_empty_capacity_launches_nothing():
    """nnz_cap == 0, n_keys == 0 or c_pool == 0: SHPL_OK and the output untouched."""
    from sparse_pooling_amd import _lib as L
    buf = torch.full((64 * 64 * 4,), 0x5A, dtype=torch.uint8, device=DEV)
    ent = torch.zeros(16, dtype=torch.int32, device=DEV)
    st = L.stream_of(torch.device(DEV))
    for n_keys, cap, c_pool in ((64, 0, 32), (0, 16, 32), (64, 16, 0)):
        csr = L.ShplCsr(ent.data_ptr(), ent.data_ptr(), ent.data_ptr(), None, n_keys, cap)
        assert L.lib().shpl_pull_clear(L.F32, ctypes.byref(csr), c_pool, L.ptr(buf), 64, 32, st) == L.OK
    torch.cuda.synchronize()
    assert bool((buf == 0x5A).all())


def test_pull_clear_argument_statuses():
    """Every bad-argument branch answers on the host (fake device pointers, nothing launched)."""
    from sparse_pooling_amd import _lib as L
    fn = L.lib().shpl_pull_clear
    P, N = ctypes.c_void_p(256), None
    csr = L.ShplCsr(256, 256, 256, None, 100, 10)
    ok = (L.F32, ctypes.byref(csr), 32, P, 64, 32, N)

    def call(**kw):
        a = dict(zip(("dtype", "csr", "c_pool", "out", "out_stride", "out_off", "stream"), ok))
        a.update(kw)
        return fn(*a.values())
    assert call(csr=None) == L.ERR_ARG
    assert call(dtype=7) == L.ERR_ARG
    assert call(out=N) == L.ERR_ARG
    assert call(csr=ctypes.byref(L.ShplCsr(None, 256, 256, None, 100, 10))) == L.ERR_ARG  # no ent_dst
    assert call(c_pool=-1) == L.ERR_BAD_SHAPE
    assert call(out_off=-4) == L.ERR_BAD_SHAPE
    assert call(out_stride=-64) == L.ERR_BAD_SHAPE
    assert call(out_stride=63) == L.ERR_BAD_SHAPE       # out_stride < out_off + c_pool
    assert call(out_stride=1 << 31, out_off=0) == L.ERR_BAD_SHAPE
    assert call(csr=ctypes.byref(L.ShplCsr(256, 256, 256, None, -1, 10))) == L.ERR_BAD_SHAPE
    assert call(csr=ctypes.byref(L.ShplCsr(256, 256, 256, None, 100, -1))) == L.ERR_BAD_SHAPE
    assert call(csr=ctypes.byref(L.ShplCsr(256, 256, 256, None, (1 << 31) - 1, 10))) == L.ERR_BAD_SHAPE
    # valid and empty: SHPL_OK without a launch
    assert call(c_pool=0) == L.OK
    assert call(csr=ctypes.byref(L.ShplCsr(None, None, None, None, 100, 0))) == L.OK


# ---------------------------------------------------------------- pipeline sequence

@pytest.mark.gpu
@pytest.mark.parametrize("dtype,form", [("f32", "beside"), ("bf16", "beside"), ("f32", "serial"), ("bf16", "serial"),
                                        ("f32", "step"), ("bf16", "off")])
def test_pipeline_sequence_matches_oracle(dtype, form, monkeypatch):
    """Four steps over frames of different seeds in the same input buffers: after each, bv_fused is the
    oracle's of that step's frames, bit for bit -- no sum of the step before left standing, short run or long.
    beside / serial: step_overlapped's two kept-zeros forms; step: FusedPipeline.step; off: KEEP_ZEROS False
    (the full stream every step), the same bits."""
    from sparse_pooling_amd import pipeline
    monkeypatch.setattr(pipeline.FusedPipeline, "KEEP_ZEROS", form != "off")
    monkeypatch.setattr(pipeline.FusedPipeline, "KEEP_ZEROS_SERIAL", form == "serial")
    r = _Run(dtype)
    clears = []
    clear = r.pl._clear_pooled
    monkeypatch.setattr(r.pl, "_clear_pooled", lambda: (clears.append(1), clear()))
    assert not r.pl._pooled_clean
    for k in range(4):
        r.load(k)
        r.plain() if form == "step" else r.overlapped()
        _same(r.pl, k, dtype)
        assert r.pl._pooled_clean == (form != "off")
    assert len(clears) == (0 if form == "off" else 3)  # the first step is the full one


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_graph_of_clean_step_replays_over_new_frames(dtype):
    """One eager step, then the kept-zeros step captured in a HIP graph; three replays, the inputs overwritten
    with the next seeds' frames before each: every replay's bv_fused is the oracle's."""
    r = _Run(dtype)
    r.load(0)
    r.overlapped()
    _same(r.pl, 0, dtype)
    assert r.pl._pooled_clean
    g = torch.cuda.CUDAGraph()
    gs = torch.cuda.Stream(device=DEV)
    gs.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=gs):
        r.overlapped()
    assert r.pl._pooled_clean
    for k in (1, 2, 3):
        r.load(k)
        g.replay()
        _same(r.pl, k, dtype)


# ---------------------------------------------------------------- state

@pytest.mark.gpu
def test_invalidate_gives_the_full_step():
    r = _Run("f32")
    r.load(0)
    r.overlapped()
    assert r.pl._pooled_clean
    r.pl.bv_fused.fill_(float("nan"))
    r.pl.invalidate()
    assert not r.pl._pooled_clean
    r.load(1)
    r.overlapped()
    _same(r.pl, 1, "f32")  # every element rewritten
    assert r.pl._pooled_clean


@pytest.mark.gpu
def test_flagged_step_gives_the_full_step():
    """A step whose index build sets an error bit (every point declared to be frame 0's: more than
    max_points_per_frame, SHPL_EBIT_CAPACITY): check() raises and marks the pipeline dirty, and the next step is
    the full one -- right over a bv_fused of NaNs."""
    from sparse_pooling_amd.errors import InvalidArgumentError
    r = _Run("f32")
    r.load(0)
    r.overlapped()
    assert r.pl._pooled_clean
    good = r.off
    n = int(good[-1].item())
    r.off = torch.tensor([0] + [n] * B, dtype=torch.int64, device=DEV)
    r.overlapped()
    torch.cuda.synchronize()
    with pytest.raises(InvalidArgumentError):
        r.pl.check()
    assert not r.pl._pooled_clean
    r.off = good
    r.pl.bv_fused.fill_(float("nan"))
    r.load(2)
    r.overlapped()
    _same(r.pl, 2, "f32")
    r.pl.check()


@pytest.mark.gpu
def test_dirty_pipeline_under_capture_stays_dirty():
    """A pipeline whose first call is under stream capture captures the full step and stays dirty: its replay
    rewrites every element, whatever bv_fused held."""
    r = _Run("f32")
    r.load(1)
    g = torch.cuda.CUDAGraph()
    gs = torch.cuda.Stream(device=DEV)
    gs.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=gs):
        r.overlapped()
    assert not r.pl._pooled_clean
    for k in (1, 2):
        r.load(k)
        r.pl.bv_fused.fill_(float("nan"))
        g.replay()
        _same(r.pl, k, "f32")
    assert not r.pl._pooled_clean


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["dual", "split"])
def test_other_pipelines_never_keep_zeros(kind, monkeypatch):
    """Dual and split pipelines write every element every step: no clear is ever issued and _pooled_clean
    stays False, through step and the overlapped steps."""
    kw = {"dual": dict(dual=True), "split": dict(split=True)}[kind]
    r = _Run("f32", **kw)
    assert not r.pl._keeps_zeros()

    def no_clear():
        raise AssertionError("shpl_pull_clear on a pipeline that does not keep zeros")
    monkeypatch.setattr(r.pl, "_clear_pooled", no_clear)
    side2 = torch.cuda.Stream(device=DEV)
    chain = torch.cuda.Stream(device=DEV, priority=-1)
    for k in range(3):
        r.load(k)
        if kind == "split":
            r.pl.step_split(r.pts, r.vox, r.off, r.P, r.tb, r.ti, r.side, chain)
        elif k == 1:
            r.plain()
        else:
            r.pl.step_overlapped(r.pts, r.vox, r.off, r.P, r.tb, r.ti, r.side, side2=side2)
        assert not r.pl._pooled_clean
        r.pl.bv_fused.fill_(float("nan"))  # theirs to rewrite whole
    r.load(3)
    if kind == "split":
        r.pl.step_split(r.pts, r.vox, r.off, r.P, r.tb, r.ti, r.side, chain)
    else:
        r.plain()
    _same(r.pl, 3, "f32")
