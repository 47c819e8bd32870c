"""The three sorting CSR builders of csrc/shpl_csr.hip (k_csr_frame; k_csr_count / k_csr_bucket /
k_csr_segment; k_csr_range) called by name through shpl_build_csr_path, bit for bit against a numpy
expectation built here, on MI355X. No GPU result is ever a reference, and this file has no tolerance.

Expectation, per frame: the valid entries -- cell >= 0, col >= 0, pix[col] >= 0 and the destination inside the
frame's key range -- sorted stably by (destination, order key, entry), the order key being nothing for
ORDER_ENTRY, (col, cell) for ORDER_COL_ROW and col for ORDER_COL_ENTRY, written from frame_off[f]; every other
slot's ent_dst is -1 (ent_src / ent_val / ent_col are compared at the occupied slots only). key_range, where
filled: the range builder gives every destination of the frames (first, end) with first = the slots before its
run, empty runs included; the frame builder's k_key_range gives empty runs (0, 0); destinations past the last
frame's are (0, 0) in both.

One input (_host()) serves every case, the smallest at which each branch is live:
  2 frames, capacities 12,288 and 6,144, live counts 12,000 and 5,000 (holes to clear), 64 slots after the
  last frame; 40,000 cells per frame (k_csr_frame's log_tile 2, the segment builder's log_bin 6) and 3,000
  pixels per frame (log_tile 0, log_bin 2); the capacity per frame is 4.5 x SEG_TARGET, so S = 5 segments;
  frame 0 has more than CSR_WIN = 10,240 valid entries, and the tile at that sorted slot straddles the LDS
  window; 4,800 of its entries share 64 cells of one bin and 4 pixels of one bin, so one segment holds more
  than SEG_WIN = 4,096 entries in either direction (and a destination's run passes 1,000 entries); one cell
  and one pixel hold a run of 300, and a cell's and a pixel's run of 200 lie across sorted slot 10,240; about 1 % of the entries are invalid in each way (cell -1, col -1, pix -1,
  a cell of the other frame, a pixel of the other frame); the slots past the live counts hold valid-looking
  garbage; weights in (-2, 2). The column array repeats columns; d_col = NULL is the identity.
All of this is asserted on the CPU before the first launch (_preconditions)."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from sparse_pooling_amd import _lib as L  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CAPS, LIVE = (12288, 6144), (12000, 5000)
N_CELLS, N_PIX = 40000, 3000
NNZ_CAP = sum(CAPS) + 64
CSR_WIN, SEG_WIN, SEG_TARGET, SEG_MAX, CSR_TILES = 10240, 4096, 2048, 1024, 16384
HOT, RUN, EDGE = 4800, 300, 200
PATHS = {"frame": L.CSR_FRAME, "segment": L.CSR_SEGMENT, "range": L.CSR_RANGE}
ORDERS = {"entry": L.ORDER_ENTRY, "col_row": L.ORDER_COL_ROW, "col_entry": L.ORDER_COL_ENTRY}


@functools.lru_cache(maxsize=None)
def _host():
    rng = np.random.default_rng(20240607)
    F = len(CAPS)
    off = np.concatenate([[0], np.cumsum(CAPS)]).astype(np.int64)
    cell = np.empty(NNZ_CAP, np.int32)
    col = np.empty(NNZ_CAP, np.int32)
    pix = np.empty(NNZ_CAP, np.int32)
    val = rng.uniform(-2.0, 2.0, NNZ_CAP).astype(np.float32)
    # valid-looking values everywhere first: the slots past the live counts must be ignored
    cell[:] = rng.integers(0, F * N_CELLS, NNZ_CAP)
    pix[:] = rng.integers(0, F * N_PIX, NNZ_CAP)
    col[:] = rng.integers(0, NNZ_CAP, NNZ_CAP)
    for f in range(F):
        e0, n = int(off[f]), LIVE[f]
        live = np.arange(e0, e0 + n)
        other = (f + 1) % F
        cell[live] = f * N_CELLS + rng.integers(0, N_CELLS, n)
        pix[live] = f * N_PIX + rng.integers(0, N_PIX, n)
        col[live] = e0 + rng.integers(0, n, n)  # repeated columns
        special = np.zeros(n, bool)
        if f == 0:
            pick = rng.permutation(n)
            hot, run = e0 + pick[:HOT], e0 + pick[HOT:HOT + RUN]
            cell[hot] = 6400 + rng.integers(0, 64, HOT)   # bin 100 of 64 cells
            pix[hot] = 1000 + rng.integers(0, 4, HOT)     # bin 250 of 4 pixels
            col[hot] = rng.choice(hot, HOT)
            cell[run], pix[run], col[run] = 12345, 2000, rng.choice(run, RUN)
            edge = e0 + pick[HOT + RUN:HOT + RUN + EDGE]
            cell[edge], pix[edge], col[edge] = N_CELLS - 1, N_PIX - 1, rng.choice(edge, EDGE)  # placed below
            special[pick[:HOT + RUN + EDGE]] = True
        for arr, bad in ((cell, -1), (col, -1), (pix, -1), (cell, None), (pix, None)):
            sel = live[(rng.random(n) < 0.01) & ~special]
            if bad is None:  # a destination of the other frame
                arr[sel] = other * (N_CELLS if arr is cell else N_PIX) + 5
            else:
                arr[sel] = bad
    # a run of EDGE entries on the cell, and on the pixel, whose run starts about EDGE / 2 sorted slots before
    # CSR_WIN: the tile at the window's edge then straddles it in both directions, whichever columns are used
    c0, p0 = cell[:LIVE[0]], pix[:LIVE[0]]
    ok = (c0 >= 0) & (p0 >= 0) & (c0 < N_CELLS - 1) & (p0 < N_PIX - 1)
    cell[edge] = np.sort(c0[ok & (c0 < N_CELLS)])[CSR_WIN - EDGE // 2]
    pix[edge] = np.sort(p0[ok & (p0 < N_PIX)])[CSR_WIN - EDGE // 2]
    nnz = np.array(LIVE, np.int64)
    return dict(off=off, nnz=nnz, cell=cell, col=col, pix=pix, val=val)


@functools.lru_cache(maxsize=None)
def _device():
    return {k: torch.from_numpy(v).to(DEV) for k, v in _host().items()}


def _expect(direction, order, identity, kpf):
    """(ent_dst, ent_src, ent_val bits, ent_col) over the whole capacity; only ent_dst is defined at empty slots."""
    h = _host()
    col = np.arange(NNZ_CAP, dtype=np.int32) if identity else h["col"]
    dst_o = np.full(NNZ_CAP, -1, np.int32)
    src_o = np.zeros(NNZ_CAP, np.int32)
    val_o = np.zeros(NNZ_CAP, np.uint32)
    col_o = np.zeros(NNZ_CAP, np.int32)
    for f in range(len(CAPS)):
        e = np.arange(h["off"][f], h["off"][f] + h["nnz"][f])
        c, k = h["cell"][e], col[e]
        p = np.where(k >= 0, h["pix"][np.maximum(k, 0)], -1)
        d = c if direction == L.BY_CELL else p
        ok = (c >= 0) & (k >= 0) & (p >= 0) & (d >= f * kpf) & (d < (f + 1) * kpf)
        e, c, k, p, d = e[ok], c[ok], k[ok], p[ok], d[ok]
        keys = {L.ORDER_ENTRY: (e, d), L.ORDER_COL_ROW: (e, c, k, d), L.ORDER_COL_ENTRY: (e, k, d)}[order]
        s = np.lexsort(keys)  # the last key is the primary one
        o = slice(int(h["off"][f]), int(h["off"][f]) + len(s))
        dst_o[o], col_o[o] = d[s], k[s]
        src_o[o] = (p if direction == L.BY_CELL else c)[s]
        val_o[o] = h["val"][e[s]].view(np.uint32)
    return dst_o, src_o, val_o, col_o


def _expect_key_range(dst, n_keys, kpf, empty_runs_placed):
    """(first, end) per destination from the expected ent_dst."""
    h = _host()
    kr = np.zeros((n_keys, 2), np.int32)
    for f in range(len(CAPS)):
        e0 = int(h["off"][f])
        d = dst[e0:e0 + CAPS[f]]
        d = d[d >= 0]
        keys = np.arange(f * kpf, (f + 1) * kpf)
        first = e0 + np.searchsorted(d, keys, "left")
        end = e0 + np.searchsorted(d, keys, "right")
        if not empty_runs_placed:
            first, end = np.where(end > first, first, 0), np.where(end > first, end, 0)
        kr[keys, 0], kr[keys, 1] = first, end
    return kr


def _preconditions(dst, kpf, ws_bytes):
    h = _host()
    F = len(CAPS)
    d0 = dst[:CAPS[0]]
    d0 = d0[d0 >= 0]
    assert len(d0) > CSR_WIN  # frame 0 fills more than one LDS window of k_csr_frame
    log_tile = 0
    while ((kpf - 1) >> log_tile) + 1 > CSR_TILES:
        log_tile += 1
    assert log_tile == (2 if kpf == N_CELLS else 0)
    assert d0[CSR_WIN - 1] >> log_tile == d0[CSR_WIN] >> log_tile  # a tile straddles the window edge
    log_bin = 0
    while ((kpf - 1) >> log_bin) + 1 > SEG_MAX:
        log_bin += 1
    n_bins = ((kpf - 1) >> log_bin) + 1
    est = (NNZ_CAP + F - 1) // F
    S = min(max((est + SEG_TARGET - 1) // SEG_TARGET, 1), n_bins)
    assert S >= 2 and F * (n_bins + S) <= NNZ_CAP // 16 + 65536  # SEGMENT is taken, not replaced by FRAME
    assert np.bincount(d0 >> log_bin).max() > SEG_WIN  # a segment (whole bins) past its LDS window
    assert np.bincount(d0).max() >= RUN
    assert ws_bytes >= L.csr_ws_bytes(F * kpf + 7, NNZ_CAP)
    assert h["nnz"][0] < CAPS[0] and NNZ_CAP > h["off"][-1]  # holes in a frame and after the last one


CASES = [(p, kr) for p in PATHS for kr in ((False, True) if p == "frame" else (p == "range",))]


@pytest.mark.parametrize("identity", [False, True], ids=["cols", "identity"])
@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("direction", ["by_cell", "by_pixel"])
@pytest.mark.parametrize("path,kr", CASES, ids=[p + ("-key_range" if kr else "") for p, kr in CASES])
def test_builder_matches_numpy(path, kr, direction, order, identity):
    d = _device()
    dirn = L.BY_CELL if direction == "by_cell" else L.BY_PIXEL
    kpf = N_CELLS if dirn == L.BY_CELL else N_PIX
    n_keys = len(CAPS) * kpf + 7  # destinations past the last frame's: empty runs
    want = _expect(dirn, ORDERS[order], identity, kpf)
    c = L.Csr(n_keys, NNZ_CAP, DEV, with_col=True, key_range=kr)
    _preconditions(want[0], kpf, c.ws.numel())
    for t in (c.ent_dst, c.ent_src, c.ent_col):
        t.fill_(0x5A5A5A5A)
    c.ent_val.fill_(float("nan"))
    if kr:
        c.key_range.fill_(0x5A5A5A5A)
    L.check(L.lib().shpl_build_csr_path(PATHS[path], dirn, ORDERS[order], len(CAPS), L.ptr(d["off"]), L.ptr(d["nnz"]),
                                        kpf, L.ptr(d["cell"]), None if identity else L.ptr(d["col"]), L.ptr(d["val"]),
                                        L.ptr(d["pix"]), c.ref(), L.ptr(c.ws), c.ws.numel(),
                                        L.stream_of(torch.device(DEV))), "shpl_build_csr_path")
    torch.cuda.synchronize()
    got = [c.ent_dst.cpu().numpy(), c.ent_src.cpu().numpy(), c.ent_val.cpu().numpy().view(np.uint32),
           c.ent_col.cpu().numpy()]
    np.testing.assert_array_equal(got[0], want[0])
    occupied = want[0] >= 0
    for g, w, name in zip(got[1:], want[1:], ("ent_src", "ent_val", "ent_col")):
        np.testing.assert_array_equal(g[occupied], w[occupied], err_msg=name)
    if kr:
        np.testing.assert_array_equal(c.key_range.cpu().numpy(),
                                      _expect_key_range(want[0], n_keys, kpf, empty_runs_placed=path == "range"))
