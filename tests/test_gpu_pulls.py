"""The pull kernels of csrc/shpl_pull.hip (k_dense, k_sparse, k_sparse_long, k_once / seg_window, k_rows,
k_rows2) on their own against the CPU oracle, in every form the host dispatch can reach, on MI355X.

Reference. The oracle's four pooling functions, applied to the channel slice [src_off, src_off + c_pool) of
the source: sparse_pool_op (BY_CELL / ORDER_ENTRY, "pool" below), sparse_pool_trans_op (BY_PIXEL /
ORDER_COL_ROW, "trans"), sparse_pool_grad_img (BY_PIXEL / ORDER_COL_ENTRY, "gimg"),
sparse_pool_trans_grad_bev (BY_CELL / ORDER_COL_ENTRY, "gbev"). The modes are composed in numpy float32: POOL
as is, CONCAT [pass bits || pooled], ADD pass + pooled. bf16: the inputs are bf16 values, the oracle runs in
f32 on them, the ADD sum is formed in f32 and one RNE rounding follows (orc.to_bf16_bits). Every comparison
is on the bit patterns (uint32 / uint16); this file has no tolerance. No GPU result is ever a reference.

Buffers. Every source and pass buffer has padding columns, guard rows and a tail of NaN, so a wrong column,
row or stride poisons the result. Every output buffer starts as a non-NaN sentinel pattern; after the call all
of it outside the rows' [0, width) columns -- the padding, the columns before a shifted output, the guard
rows -- must still hold the sentinel. The ADD operand carries -0.0 at an empty and at an occupied
destination; a CONCAT pass-through half carries -0.0, +-inf, a NaN with a payload and a denormal (a copy:
the bits are compared). Default calls already use src_off = 8, pass_off = 16 and strides 8 elements wider
than the row, all on the 16-byte grid of both dtypes.

Maps (built once, _maps()). One frame, 37 x 29 = 1073 BEV cells, 23 x 31 = 713 pixels.
  main   1600 entries in ~900 columns, shuffled entry order, weights in (-2, 2), columns repeating inside
         pixel runs; the cell runs and the pixel runs each hold every length of RUN_LENGTHS and one of 600
         (asserted from the sorted CSRs): k_sparse's WALK (2), LONG_RUN (8 / 9), k_sparse_long's LONG_WALK
         (16 / 17), k_rows' index batches (G / G + 1 for G = 8 .. 64), the run heads (head_k / head_k + 1),
         seg_window's 64 entries, LONG_IDX = 512. First and last destination occupied, ~3/4 empty.
  ident  the same runs with col = arange(nnz): the pixel CSR is pulled with ent_col = NULL and
         SHPL_CSR_IDENTITY_COLS.
  cap    3000 live entries in 2048 * 320 capacity slots (a ShplMap with frame_off = [0, cap], frame_nnz =
         [n]): k_sparse_long's workgroups take a second round of slots, and a run of 20 starts at sorted slot
         260 (260 mod 320 >= 256, asserted) in both directions.
  tiny   5 entries: a capacity of at most LONG_RUN slots, where k_sparse takes every run unsplit.
  empty  nnz 0.

Dispatch table: template instance -> the tests that launch it (T = float / uint16_t; "vec" = VEC 4 / 8,
"scalar" = VEC 1; every line holds for both dtypes unless it names one).
  k_dense<T, VEC, POW2>            vec POW2: test_chunk_counts[*-flat-k1/k8-*]; vec !POW2:
                                   test_entry_points[*-flat-*] (3 chunks); scalar: test_chunk_counts[*-flat-c3-*]
                                   (POW2 for POOL c = 4 in test_vector_predicate[*-flat-*-c_pool], else not)
  k_sparse<.., GROUP, SPLIT, POW2, LIVE>
      SPLIT, !LIVE                 test_entry_points[*-flat-*] and [*-split-*] (GROUP: trans / gimg; POW2 by
                                   test_chunk_counts[*-flat-k1/k8-*]); scalar: test_chunk_counts[*-flat-c3/c12-*]
      !SPLIT, LIVE                 test_entry_points[*-live-*]
      !SPLIT, !LIVE                test_tiny_capacity (nnz_cap <= LONG_RUN)
      SPLIT, LIVE                  unreachable: sparse() sets split = !live
  k_sparse_long<T, VEC, GROUP>     every flat / split case (runs of 9 .. 600); its second round per workgroup:
                                   test_capacity_second_round
  k_once<T, VEC, GROUP, POW2>      test_entry_points[*-once-*], test_chunk_counts[*-once-*] (POW2: k1, k8;
                                   not: k3 .. k65), test_once_switch (seg_window from 32 chunks, !GROUP only;
                                   GROUP keeps the thread form); scalar: test_chunk_counts[*-once-c3/c12-*]
  k_rows<T, VEC, GROUP, G>         G = 8: k1, k3, k8, c3; 16: k9, c12; 32: k17; 64: k33, k65 (a second pc0
                                   round) of test_chunk_counts[*-rows-*]; GROUP: trans, !GROUP: pool; the run
                                   heads: test_run_heads[*-rows-*]
  k_rows2<T, VEC, G, GR1, MODE>    MODE POOL / CONCAT / ADD: test_entry_points[*-pair-*],
                                   test_chunk_counts[*-pair-*] (G as k_rows); MODE -1:
                                   test_pair_mixed_modes; GR1 false: test_pair_identity_cols[*-null]; one
                                   side absent (MODE of the other): test_pair_one_side; G from the wider
                                   side: test_pair_narrow_beside_wide; heads: test_run_heads[*-pair-*]
  two-launch fallback of shpl_pull_pair (k_rows twice): test_pair_two_launches
  Not launched by any public call: k_sparse<SPLIT, LIVE> (above). Every other instantiated combination is a
  product of the parameters listed, each of which is launched at least once per kernel; the full product is
  not run.

Statuses: test_statuses walks every SHPL_ERR_ARG / SHPL_ERR_BAD_SHAPE branch of plan(), shpl_pull_once and
shpl_pull_pair; each returns before any launch (the sentinel output is unchanged).
"""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

from oracle import shpl_oracle as orc
from sparse_pooling_amd import _lib as L

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = "f32", "bf16"
VEC = {F32: 4, BF16: 8}  # elements of a 16-byte chunk
NPT = {F32: np.uint32, BF16: np.uint16}
NPI = {F32: np.int32, BF16: np.int16}
TORCH = {F32: torch.float32, BF16: torch.bfloat16}
TINT = {F32: torch.int32, BF16: torch.int16}
CODE = {F32: L.F32, BF16: L.BF16}
NAN = {F32: 0x7FC00000, BF16: 0x7FC0}
SENTINEL = {F32: 0x5A5A5A5A, BF16: 0x5A5A}  # 1.5e16 / 1.5e16: not a NaN, not a value any case produces
NEG0 = {F32: 0x80000000, BF16: 0x8000}
# -0.0, +inf, -inf, a quiet NaN with a payload, the smallest denormal
SPECIALS = {F32: [0x80000000, 0x7F800000, 0xFF800000, 0x7FC12345, 0x00000001],
            BF16: [0x8000, 0x7F80, 0xFF80, 0x7FC1, 0x0001]}

HB, WB, H, W = 37, 29, 23, 31
R, NP = HB * WB, H * W
RUN_LENGTHS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 150)
BIG_RUN = 600
N_MAIN = 1600
CAP = 2048 * 320  # LONG_GRID workgroups of k_sparse_long x 320 slots each: a second round of SHPL_BLOCK = 256
N_CAP = 3000
WMAX = 576  # widest row of the master data (65 bf16 chunks + offsets)
GUARD = 2   # guard rows before and after every buffer's rows

# order name -> (direction, order, source rows, destination rows)
ORD = {"pool": (L.BY_CELL, L.ORDER_ENTRY, NP, R), "trans": (L.BY_PIXEL, L.ORDER_COL_ROW, R, NP),
       "gimg": (L.BY_PIXEL, L.ORDER_COL_ENTRY, R, NP), "gbev": (L.BY_CELL, L.ORDER_COL_ENTRY, NP, R)}
MODES = {"POOL": L.OUT_POOL, "CONCAT": L.OUT_CONCAT, "ADD": L.OUT_ADD}


@pytest.fixture(scope="module", autouse=True)
def _lib():
    L.lib()
    assert torch.cuda.is_available()


# ------------------------------------------------------------------------------------------------ maps

def _fill_lens(rng, head, total, hi):
    """head + random lengths in [1, hi] summing to total."""
    lens = list(head)
    left = total - sum(lens)
    assert left >= 0
    while left > 0:
        k = int(min(left, rng.integers(1, hi + 1)))
        lens.append(k)
        left -= k
    return lens


def _gen_map(seed, cell_lens, pix_lens, identity=False):
    """A host map in the reference's format whose cell runs have the lengths cell_lens (the i-th occupied
    cell, in increasing order, has cell_lens[i] entries) and whose pixel runs have pix_lens, entries
    associated at random; first and last destination occupied. Columns: identity, or about one per two entries with
    the entries of one column on one pixel and on distinct cells (no duplicate (row, col)), column ids and
    entry order shuffled."""
    rng = np.random.default_rng(seed)
    n = int(sum(cell_lens))
    assert n == int(sum(pix_lens))

    def dests(lens, total):
        mid = rng.choice(np.arange(1, total - 1), len(lens) - 2, replace=False)
        return np.sort(np.concatenate([[0, total - 1], mid])).astype(np.int64)

    cell = np.repeat(dests(cell_lens, R), cell_lens)
    pix = np.repeat(dests(pix_lens, NP), pix_lens)[rng.permutation(n)]
    if identity:
        col, col_pix = np.arange(n, dtype=np.int64), pix.copy()
    else:
        col = np.empty(n, np.int64)
        col_pix = []
        by_pix = np.lexsort((cell, pix))  # entries grouped by pixel, by cell inside
        starts = np.flatnonzero(np.r_[True, pix[by_pix][1:] != pix[by_pix][:-1]])
        for a, b in zip(starts, np.r_[starts[1:], n]):
            grp = by_pix[a:b]
            most = int(np.unique(cell[grp], return_counts=True)[1].max())
            m = max(int(np.ceil(0.5 * (b - a))), most)
            col[grp] = len(col_pix) + np.arange(b - a) % m  # equal cells are adjacent: distinct columns
            col_pix += [pix[grp[0]]] * m
        col_pix = np.asarray(col_pix, np.int64)
        relabel = rng.permutation(len(col_pix))
        col = relabel[col]
        col_pix = col_pix[np.argsort(relabel)]
    assert len(np.unique(np.stack([cell, col], 1), axis=0)) == n
    assert np.array_equal(col_pix[col], pix)
    e = rng.permutation(n)
    mij = np.stack([cell[e], col[e]], 1).astype(np.int64)
    mval = rng.uniform(-2, 2, n).astype(np.float32)
    idx = np.stack([np.zeros(len(col_pix), np.int64), col_pix // W, col_pix % W], 1)
    return types.SimpleNamespace(mij=mij, mval=mval, idx=idx, ncols=len(col_pix), nnz=n, csr={}, runs={},
                                 tabs={}, identity=identity)


def _main_lens(rng):
    return [int(v) for v in rng.permutation(_fill_lens(rng, RUN_LENGTHS + (BIG_RUN,), N_MAIN, 3))]


def _pack(m):
    from sparse_pooling_amd import shpl_map as sm
    t = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    return sm.pack_map(t(m.mij), t(m.mval), np.array([R, m.ncols]), t(m.idx), (1, H, W, 1))


@functools.lru_cache(maxsize=None)
def _maps():
    from sparse_pooling_amd import shpl_map as sm
    rng = np.random.default_rng(31)
    maps = {}
    cl, pl = _main_lens(rng), _main_lens(rng)
    maps["main"] = _gen_map(32, cl, pl)
    assert 850 <= maps["main"].ncols <= 1000, maps["main"].ncols
    maps["ident"] = _gen_map(33, cl, pl, identity=True)
    maps["tiny"] = _gen_map(34, [3, 2], [1, 4])
    maps["empty"] = types.SimpleNamespace(mij=np.zeros((0, 2), np.int64), mval=np.zeros(0, np.float32),
                                          idx=np.zeros((0, 3), np.int64), ncols=0, nnz=0, csr={}, runs={}, tabs={},
                                          identity=False)
    for name in ("main", "ident", "tiny", "empty"):
        maps[name].smap = _pack(maps[name])
    # the capacity map: the live entries in the first slots of one frame of CAP slots
    m = _gen_map(35, _fill_lens(rng, [260, 20], N_CAP, 12), _fill_lens(rng, [260, 20], N_CAP, 12))
    cell = np.full(CAP, -1, np.int32)
    col = np.zeros(CAP, np.int32)
    val = np.zeros(CAP, np.float32)
    cell[:m.nnz], col[:m.nnz], val[:m.nnz] = m.mij[:, 0], m.mij[:, 1], m.mval
    pix = (m.idx[:, 1] * W + m.idx[:, 2]).astype(np.int32)
    t = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    m.smap = sm.ShplMap(t(cell), t(col), t(val), t(pix), CAP, R, NP, m.ncols, DEV,
                        frame_off=torch.tensor([0, CAP], dtype=torch.int64, device=DEV),
                        frame_nnz=torch.tensor([m.nnz], dtype=torch.int64, device=DEV), n_frames=1)
    maps["cap"] = m
    return maps


def _csr(mname, order, kr):
    """The sorted CSR of a map for one order (flat, or with key_range), built once; its runs on the host."""
    m = _maps()[mname]
    key = (order, kr)
    if key not in m.csr:
        direction, o, _, n_keys = ORD[order]
        s = m.smap
        c = L.Csr(n_keys, s.nnz_cap, DEV, with_col=direction == L.BY_PIXEL, key_range=kr)
        L.check(L.lib().shpl_build_csr_path(L.CSR_AUTO, direction, o, 1, L.ptr(s.frame_off), L.ptr(s.frame_nnz),
                                            n_keys, L.ptr(s.cell), L.ptr(s.col), L.ptr(s.val), L.ptr(s.pix),
                                            c.ref(), L.ptr(c.ws), c.ws.numel(), L.stream_of(torch.device(DEV))),
                "shpl_build_csr_path")
        torch.cuda.synchronize()
        m.csr[key] = c
        if s.nnz_cap:
            d = c.ent_dst.cpu().numpy()
            slots = np.flatnonzero(d >= 0)
            keys, first, counts = np.unique(d[slots], return_index=True, return_counts=True)
            runs = types.SimpleNamespace(keys=keys, first=slots[first], counts=counts)
            assert counts.sum() == m.nnz and np.all(np.diff(d[slots]) >= 0)
            if kr:  # key_range restates the runs
                k = c.key_range.cpu().numpy()
                assert np.array_equal(k[keys, 0], runs.first) and np.array_equal(k[keys, 1], runs.first + counts)
                assert np.array_equal(np.flatnonzero(k[:, 1] - k[:, 0]), keys)
        else:
            runs = types.SimpleNamespace(keys=np.zeros(0, np.int64), first=np.zeros(0, np.int64),
                                         counts=np.zeros(0, np.int64))
        m.runs[order] = runs
        _check_runs(mname, runs, n_keys)
    return m.csr[key]


def _check_runs(mname, runs, n_keys):
    """Host assertions on a sorted CSR: a change to the generator cannot silently drop an edge."""
    have = set(int(c) for c in runs.counts)
    if mname in ("main", "ident"):
        missing = [k for k in RUN_LENGTHS if k not in have]
        assert not missing, (mname, missing)
        assert max(have) >= BIG_RUN
        assert runs.keys[0] == 0 and runs.keys[-1] == n_keys - 1
        assert len(runs.keys) < n_keys // 2  # plenty of empty destinations
    elif mname == "cap":
        # k_sparse_long's second round: a long run whose first slot is past the workgroup's first 256 slots
        per_block = CAP // 2048
        assert any(c > 8 and f % per_block >= 256 for c, f in zip(runs.counts, runs.first)), mname
        assert max(have) > 8
    elif mname == "tiny":
        assert _maps()[mname].smap.nnz_cap <= 8


def _runs(mname, order):
    _csr(mname, order, False)
    return _maps()[mname].runs[order]


def _with(csr, **fields):
    """A copy of a CSR's ABI struct with some fields replaced (the tensors stay owned by csr)."""
    s = L.ShplCsr.from_buffer_copy(csr.struct)
    for k, v in fields.items():
        setattr(s, k, v)
    return s


def _live(mname, order):
    """The flat CSR with the frame layout attached (Csr.live_frames): LIVE, which takes every run."""
    m = _maps()[mname]
    key = ("live", order)
    if key not in m.tabs:
        m.tabs[key] = (torch.tensor([0, m.smap.nnz_cap], dtype=torch.int64, device=DEV),
                       torch.tensor([m.nnz], dtype=torch.int64, device=DEV))
    off, nnz = m.tabs[key]
    s = _with(_csr(mname, order, False), frame_off=off.data_ptr(), frame_nnz=nnz.data_ptr(), n_frames=1)
    return s


def _heads(mname, order, k):
    """The key_range CSR of a cell-keyed order with run heads filled on the host from the sorted entries:
    (source, weight bits) of the first min(run, k) entries of each destination. Slots past a run's length
    hold a valid source row and a NaN weight: a kernel that uses them gives a wrong number, no wild read."""
    m = _maps()[mname]
    c = _csr(mname, order, True)
    key = ("heads", order, k)
    if key not in m.tabs:
        runs, n_src, n_keys = m.runs[order], ORD[order][2], ORD[order][3]
        src = c.ent_src.cpu().numpy()
        wbits = c.ent_val.cpu().numpy().view(np.int32)
        tab = np.empty((n_keys, k, 2), np.int32)
        tab[:, :, 0] = (np.arange(n_keys)[:, None] * 7 + np.arange(k)[None, :] * 3) % n_src
        tab[:, :, 1] = np.int32(NAN[F32])
        for d, f, cnt in zip(runs.keys, runs.first, runs.counts):
            j = min(int(cnt), k)
            tab[d, :j, 0] = src[f:f + j]
            tab[d, :j, 1] = wbits[f:f + j]
        assert tab[:, :, 0].min() >= 0 and tab[:, :, 0].max() < n_src
        m.tabs[key] = torch.from_numpy(tab).to(DEV)
    return _with(c, heads=m.tabs[key].data_ptr(), head_k=k)


# ------------------------------------------------------------------------------------------------ data

def _bf(a):
    return orc.from_bf16_bits(orc.to_bf16_bits(a))


@functools.lru_cache(maxsize=None)
def _master(dt, rows, what):
    """Host data [rows, WMAX] f32 (bf16: bf16 values), read-only; "src" and "pass" differ."""
    rng = np.random.default_rng([41, rows, VEC[dt], int(what == "src")])
    a = rng.standard_normal((rows, WMAX)).astype(np.float32)
    if dt == BF16:
        a = _bf(a)
    a.setflags(write=False)
    return a


def _bits(dt, a):
    a = np.ascontiguousarray(a, np.float32)
    return a.view(np.uint32) if dt == F32 else orc.to_bf16_bits(a)


def _vals(dt, b):
    return b.view(np.float32) if dt == F32 else orc.from_bf16_bits(b)


def _oracle(m, order, x):
    """The oracle's pooling function of one order on x [source rows, c] -> [destination rows, c] f32."""
    c = x.shape[1]
    n_dst = ORD[order][3]
    if c == 0:
        return np.zeros((n_dst, 0), np.float32)
    ms = [R, m.ncols]
    x = np.ascontiguousarray(x, np.float32)
    if order == "pool":
        return orc.sparse_pool_op(m.mij, m.mval, ms, x.reshape(1, H, W, c), m.idx).reshape(n_dst, c)
    if order == "trans":
        return orc.sparse_pool_trans_op(m.mij, m.mval, ms, x, m.idx, (1, H, W, c)).reshape(n_dst, c)
    if order == "gimg":
        return orc.sparse_pool_grad_img(m.mij, m.mval, ms, x, m.idx, (1, H, W, c)).reshape(n_dst, c)
    return orc.sparse_pool_trans_grad_bev(m.mij, m.mval, ms, x.reshape(1, H, W, c), m.idx).reshape(n_dst, c)


def _buffer(dt, rows, stride, shift, fill, span=None, data=None, col0=0):
    """A flat device buffer of `fill` bits: GUARD rows, then `rows` rows of `stride` elements starting `shift`
    elements past a 256-byte boundary, then GUARD rows and a tail; data bits [rows, w] at columns
    [col0, col0 + w). Returns (flat tensor, the view from row 0 on, its first element's index)."""
    span = max(stride, span or 0, 1)
    base = (GUARD * span + 127) // 128 * 128 + shift
    host = np.full(base + (rows + GUARD) * span + 128, fill, NPT[dt])
    if data is not None and data.shape[1]:
        at = base + np.arange(rows)[:, None] * stride + col0 + np.arange(data.shape[1])[None, :]
        host[at] = data
    flat = torch.from_numpy(host.view(NPI[dt])).to(DEV).view(TORCH[dt])
    return flat, flat[base:], base


class Call:
    """One pull: its device buffers, its arguments after the csr, and the oracle's expectation in bits."""

    def __init__(self, dt, order, mode, c_pool, c_pass=None, src_off=8, pass_off=16, src_stride=None,
                 pass_stride=None, out_stride=None, out_shift=0, src_shift=0, pass_shift=0, mname="main",
                 null_src=False):
        m = _maps()[mname]
        self.dt, self.order, self.mname = dt, order, mname
        self.mode = MODES[mode]
        n_src, n_dst = ORD[order][2], ORD[order][3]
        self.n_dst = n_dst
        if mode == "POOL":
            c_pass, pass_off = 0, 0
        elif c_pass is None:
            c_pass = c_pool if mode == "ADD" else 2 * VEC[dt]
        self.c_pool, self.c_pass, self.src_off, self.pass_off = c_pool, c_pass, src_off, pass_off
        self.width = c_pool + (c_pass if mode == "CONCAT" else 0)
        self.src_stride = src_off + c_pool + 8 if src_stride is None else src_stride
        self.pass_stride = 0 if mode == "POOL" else pass_off + c_pass + 8 if pass_stride is None else pass_stride
        self.out_stride = self.width + 8 if out_stride is None else out_stride
        self.shifts = (out_shift, src_shift, pass_shift)
        # the oracle on the source's channel slice
        x = _master(dt, n_src, "src")[:, :c_pool]
        pooled = _oracle(m, order, x)
        self.src = None
        if not null_src:
            self._src, self.src, _ = _buffer(dt, n_src, self.src_stride, src_shift, NAN[dt], data=_bits(dt, x),
                                             col0=src_off)
        self.pass_ = None
        if mode == "POOL":
            exp = _bits(dt, pooled)
        else:
            pb = _bits(dt, _master(dt, n_dst, "pass")[:, :c_pass]).copy()
            runs = _runs(mname, order)
            occupied = np.zeros(n_dst, bool)
            occupied[runs.keys] = True
            rows = [int(np.flatnonzero(~occupied)[0])] + ([int(runs.keys[1])] if len(runs.keys) > 1 else [])
            for r in rows:  # an empty and an occupied destination
                if mode == "ADD":
                    pb[r, ::3] = NEG0[dt]
                else:
                    k = min(c_pass, len(SPECIALS[dt]))
                    pb[r, :k] = SPECIALS[dt][:k]
            # (the ADD operand is read at key * pass_stride; the span keeps any row stride of the call inside)
            self._pass, self.pass_, _ = _buffer(dt, n_dst, self.pass_stride, pass_shift, NAN[dt],
                                                span=self.out_stride, data=pb, col0=pass_off)
            if mode == "CONCAT":
                exp = np.concatenate([pb, _bits(dt, pooled)], 1)
            else:
                exp = _bits(dt, _vals(dt, pb) + pooled)
        self.exp = exp
        self._out, self.out, self.out_base = _buffer(dt, n_dst, self.out_stride, out_shift, SENTINEL[dt])

    def vec(self):
        """plan()'s v16 predicate, restated: 16-byte chunks need every row start and every channel split on
        a 16-byte boundary."""
        v = VEC[self.dt]
        out_shift, src_shift, pass_shift = self.shifts
        ok = self.c_pool % v == 0 and self.out_stride % v == 0 and out_shift % v == 0
        if self.c_pool > 0:
            ok = ok and self.src_stride % v == 0 and self.src_off % v == 0 and src_shift % v == 0
        if self.mode != L.OUT_POOL:
            ok = ok and self.c_pass % v == 0 and self.pass_stride % v == 0 and self.pass_off % v == 0 \
                and pass_shift % v == 0
        return ok

    def args(self):
        return (L.ptr(self.src), self.src_stride, self.src_off, self.c_pool, L.ptr(self.pass_), self.pass_stride,
                self.pass_off, self.c_pass, self.mode, L.ptr(self.out), self.out_stride)

    def desc(self):
        return L.pull_desc(CODE[self.dt], self.src, self.src_stride, self.src_off, self.c_pool, self.pass_,
                           self.pass_stride, self.pass_off, self.c_pass, self.mode, self.out, self.out_stride)

    def check(self, what=""):
        """The rows' [0, width) columns equal the expectation bit for bit; everything else is untouched."""
        got = self._out.view(TINT[self.dt]).cpu().numpy().view(NPT[self.dt]).copy()
        at = self.out_base + np.arange(self.n_dst)[:, None] * self.out_stride + np.arange(self.width)[None, :]
        np.testing.assert_array_equal(got[at], self.exp, err_msg=f"{what}: rows differ from the oracle")
        got[at] = SENTINEL[self.dt]
        bad = np.flatnonzero(got != SENTINEL[self.dt])
        assert bad.size == 0, f"{what}: {bad.size} elements outside the rows' columns written, first at " \
                              f"{bad[0] - self.out_base} from the output pointer"

    def untouched(self):
        got = self._out.view(TINT[self.dt]).cpu().numpy().view(NPT[self.dt])
        return bool((got == SENTINEL[self.dt]).all())


def _stream():
    return L.stream_of(torch.device(DEV))


def _ref(s):
    return s.ref() if isinstance(s, L.Csr) else ctypes.byref(s)


def _csr_for(form, call, csr=None):
    if csr is not None:
        return csr
    if form == "live":
        return _live(call.mname, call.order)
    return _csr(call.mname, call.order, form in ("rows", "once", "pair"))


def launch(form, call, csr=None):
    """One pull through an entry point: flat (shpl_pull over a CSR without key_range: k_dense + k_sparse +
    k_sparse_long), live (the same with the frame layout), split (shpl_pull_dense, then shpl_pull_sparse),
    rows (shpl_pull over a key_range CSR: k_rows), once (shpl_pull_once), pair (shpl_pull_pair, one side)."""
    direction = ORD[call.order][0]
    if form == "pair":
        return pair(call if direction == L.BY_CELL else None, call if direction == L.BY_PIXEL else None,
                    cell_csr=csr if direction == L.BY_CELL else None,
                    pix_csr=csr if direction == L.BY_PIXEL else None)
    c = _csr_for(form, call, csr)
    lib = L.lib()
    fns = {"flat": [lib.shpl_pull], "live": [lib.shpl_pull], "rows": [lib.shpl_pull],
           "split": [lib.shpl_pull_dense, lib.shpl_pull_sparse], "once": [lib.shpl_pull_once]}[form]
    for fn in fns:
        rc = fn(direction, CODE[call.dt], _ref(c), *call.args(), _stream())
        assert rc == L.OK, (form, rc)
    torch.cuda.synchronize()


def pair(cell, pix, cell_csr=None, pix_csr=None):
    """shpl_pull_pair of a cell-keyed and a pixel-keyed Call (either None)."""
    cc = None if cell is None and cell_csr is None else _csr_for("pair", cell, cell_csr)
    pc = None if pix is None and pix_csr is None else _csr_for("pair", pix, pix_csr)
    dc = cell.desc() if cell is not None else None
    dp = pix.desc() if pix is not None else None
    rc = L.lib().shpl_pull_pair(_ref(cc) if cc is not None else None, ctypes.byref(dc) if dc else None,
                                _ref(pc) if pc is not None else None, ctypes.byref(dp) if dp else None, _stream())
    assert rc == L.OK, rc
    torch.cuda.synchronize()


DTS = [F32, BF16]
FORMS = ["flat", "live", "split", "rows", "once", "pair"]


def _modes(form):
    return ["POOL"] if form == "once" else ["POOL", "CONCAT", "ADD"]


# ------------------------------------------------------------------------------------------------ tests

def test_maps_hold_every_run_length():
    """The sorted CSRs of the main, identity and capacity maps hold every run length the kernels have an
    edge at, in both directions and every order (asserted in _csr on the host, from ent_dst / key_range)."""
    for mname in ("main", "ident"):
        for order in ORD:
            for kr in (False, True):
                _csr(mname, order, kr)
            assert set(RUN_LENGTHS) <= set(int(c) for c in _runs(mname, order).counts)
    for order in ("pool", "trans"):
        _csr("cap", order, False)
    # columns repeat inside the pixel runs, inside an index batch of 8 and across two batches
    m = _maps()["main"]
    pix = (m.idx[:, 1] * W + m.idx[:, 2])[m.mij[:, 1]]
    per_col = np.unique(m.mij[:, 1], return_counts=True)[1]
    assert per_col.max() >= 2 and np.unique(pix).size < m.ncols < m.nnz
    c = _csr("main", "trans", False)
    col = c.ent_col.cpu().numpy()
    runs = _runs("main", "trans")
    f = int(runs.first[np.argmax(runs.counts)])
    seq = col[f:f + int(runs.counts.max())]
    change = np.flatnonzero(seq[1:] != seq[:-1]) + 1
    assert np.any(change % 8 != 0) and np.any(change % 8 == 0) and change.size < seq.size - 1


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("order", list(ORD))
@pytest.mark.parametrize("dt", DTS)
def test_entry_points(dt, order, form):
    """Matrix item 1 / 2: all four orders through each entry point, every mode it has, 3 chunks wide (not a
    power of two), a CONCAT pass-through half of another width, non-trivial offsets and strides."""
    for mode in _modes(form):
        call = Call(dt, order, mode, 3 * VEC[dt])
        assert call.vec()
        launch(form, call)
        call.check(f"{form} {mode}")


@pytest.mark.parametrize("form", ["flat", "rows", "once", "pair"])
@pytest.mark.parametrize("order", ["pool", "trans"])
@pytest.mark.parametrize("c_pass", ["on", "off"])
@pytest.mark.parametrize("dt", DTS)
def test_pool_into_wider_row(dt, c_pass, order, form):
    """POOL written into the pooled columns of a wider row: out = base + c_pass elements, out_stride =
    c_pass + c_pool, for c_pass on and off the vector grid; the row's first c_pass columns stay untouched."""
    cp = 2 * VEC[dt] if c_pass == "on" else 5
    call = Call(dt, order, "POOL", 3 * VEC[dt], out_shift=cp, out_stride=cp + 3 * VEC[dt])
    assert call.vec() == (c_pass == "on")
    launch(form, call)
    call.check(form)


@pytest.mark.parametrize("form", ["flat", "split", "rows", "pair"])
@pytest.mark.parametrize("order", ["pool", "trans"])
@pytest.mark.parametrize("dt", DTS)
def test_concat_without_pooled_part(dt, order, form):
    """CONCAT with c_pool = 0 (and no source at all): the pass-through copy alone, vector and scalar."""
    for c_pass in (3 * VEC[dt], 5):
        call = Call(dt, order, "CONCAT", 0, c_pass=c_pass, null_src=True)
        launch(form, call)
        call.check(f"{form} c_pass {c_pass}")


TERMS = ["aligned", "out_ptr", "src_ptr", "pass_ptr", "out_stride", "src_stride", "pass_stride", "src_off",
         "pass_off", "c_pool", "c_pass"]


def _predicate_call(dt, order, mode, term):
    """A fully aligned call whose offsets and strides are all non-trivial multiples of the vector width,
    with one term of plan()'s v16 predicate broken."""
    v = VEC[dt]
    kw = dict(c_pool=3 * v, c_pass=3 * v if mode == "ADD" else 2 * v, src_off=2 * v, pass_off=3 * v)
    width = kw["c_pool"] + (kw["c_pass"] if mode == "CONCAT" else 0)
    kw.update(src_stride=kw["src_off"] + kw["c_pool"] + v, pass_stride=kw["pass_off"] + kw["c_pass"] + 2 * v,
              out_stride=width + v)
    if term.endswith("_ptr"):
        kw[term[:-4] + "_shift"] = 1  # a view one element into a larger tensor
    elif term != "aligned":
        kw[term] += 1
        if mode == "ADD" and term in ("c_pool", "c_pass"):
            kw["c_pool"] = kw["c_pass"] = max(kw["c_pool"], kw["c_pass"])
    return Call(dt, order, mode, kw.pop("c_pool"), **kw)


# shpl_pull_once is POOL only, and POOL reads no pass operand: its terms are not in the predicate
PREDICATE = [(form, term) for form in ("flat", "rows", "once", "pair") for term in TERMS
             if not (form == "once" and "pass" in term)]


@pytest.mark.parametrize("form,term", PREDICATE, ids=[f"{f}-{t}" for f, t in PREDICATE])
@pytest.mark.parametrize("order", ["pool", "trans"])
@pytest.mark.parametrize("dt", DTS)
def test_vector_predicate(dt, order, form, term):
    """Matrix item 3: the aligned call takes the vector form and is right; with any one term of the
    predicate broken (a base pointer one element on, a stride, an offset or a channel count + 1) the call
    takes the scalar form and is still right."""
    modes = ["POOL"] if form == "once" else ["CONCAT", "ADD"]
    for mode in modes:
        call = _predicate_call(dt, order, mode, term)
        assert call.vec() == (term == "aligned"), (mode, term)
        launch(form, call)
        call.check(f"{form} {mode} {term}")


# pooled widths: k<n> = n 16-byte chunks (G = 8 / 16 / 32 / 64, a second pc0 round at 65, powers of two
# and not), c<n> = n channels in the scalar form (bf16 c12: 12 scalar chunks)
WIDTHS = ["k1", "k3", "k8", "k9", "k17", "k33", "k65", "c3", "c12"]


def _width(dt, wd):
    n = int(wd[1:])
    return n * VEC[dt] if wd[0] == "k" else n


# the flat form's chunk loops have no edge past 33 chunks; 12 f32 channels are 3 vector chunks (test_entry_points)
CHUNKS = [(dt, form, wd) for dt in DTS for form in ("flat", "rows", "once", "pair") for wd in WIDTHS
          if not (form == "flat" and wd == "k65") and not (dt == F32 and wd == "c12")]


@pytest.mark.parametrize("dt,form,wd", CHUNKS, ids=[f"{d}-{f}-{w}" for d, f, w in CHUNKS])
@pytest.mark.parametrize("order", ["pool", "trans"])
def test_chunk_counts(order, dt, form, wd):
    """Matrix item 4: pooled widths of 1 to 65 chunks and the scalar widths, every mode; CONCAT with a
    pass-through half wider than a lane group beside a narrow pooled part (and a narrow one beside a wide
    pooled part)."""
    c = _width(dt, wd)
    scalar = wd[0] == "c"
    for mode in _modes(form):
        if scalar:
            c_pass = 11 if mode == "CONCAT" else None  # 11 scalar chunks beside G = 8 / 16
        else:
            c_pass = (17 if c // VEC[dt] <= 9 else 2) * VEC[dt] if mode == "CONCAT" else None
        call = Call(dt, order, mode, c, c_pass=c_pass)
        assert call.vec() != scalar
        launch(form, call)
        call.check(f"{form} {mode} {wd}")


@pytest.mark.parametrize("order,chunks", [("pool", 31), ("pool", 32), ("gbev", 32), ("trans", 32), ("gimg", 32),
                                          ("gbev", 35)])
@pytest.mark.parametrize("dt", DTS)
def test_once_switch(dt, order, chunks):
    """Matrix item 5: shpl_pull_once changes from a thread per (entry, chunk) to a wave per 64 entries
    (seg_window) at 32 chunks, cell-keyed only: 31 and 32 chunks cell-keyed, 32 chunks pixel-keyed with
    ent_col (the thread form), 31 / 35 chunks for the zero rows' division."""
    call = Call(dt, order, "POOL", chunks * VEC[dt])
    assert call.vec()
    launch("once", call)
    call.check(f"once {order} {chunks}")


@pytest.mark.parametrize("form", ["rows", "pair"])
@pytest.mark.parametrize("chunks", [3, 33])
@pytest.mark.parametrize("head_k", [1, 3, 8, 32])
@pytest.mark.parametrize("dt", DTS)
def test_run_heads(dt, head_k, chunks, form):
    """Matrix item 6: cell-keyed range CSRs with run heads filled on the host (head_k 1, 3, 8, 32), pulled
    row-keyed and paired at G = 8 and G = 64, both cell-keyed orders; head slots past a run's end carry a
    NaN weight, so using one shows."""
    for order, mode in (("pool", "POOL"), ("pool", "CONCAT"), ("gbev", "ADD")):
        call = Call(dt, order, mode, chunks * VEC[dt])
        launch(form, call, csr=_heads("main", order, head_k))
        call.check(f"{form} {order} {mode} head_k {head_k}")
    if form == "pair":  # both sides at once, the pixel side without heads
        cell, pix = Call(dt, "pool", "CONCAT", chunks * VEC[dt]), Call(dt, "trans", "CONCAT", chunks * VEC[dt])
        pair(cell, pix, cell_csr=_heads("main", "pool", head_k))
        cell.check("pair cell")
        pix.check("pair pixel")


@pytest.mark.parametrize("orders", [("pool", "trans"), ("gbev", "gimg")])
@pytest.mark.parametrize("mode", ["POOL", "CONCAT", "ADD"])
@pytest.mark.parametrize("dt", DTS)
def test_pair_same_mode(dt, mode, orders):
    """Matrix item 7: both sides of shpl_pull_pair in one launch with the mode at compile time."""
    cell, pix = Call(dt, orders[0], mode, 3 * VEC[dt]), Call(dt, orders[1], mode, 5 * VEC[dt])
    pair(cell, pix)
    cell.check("cell")
    pix.check("pixel")


@pytest.mark.parametrize("modes", [("POOL", "ADD"), ("ADD", "POOL"), ("CONCAT", "POOL"), ("ADD", "CONCAT")])
@pytest.mark.parametrize("dt", DTS)
def test_pair_mixed_modes(dt, modes):
    """POOL beside ADD (and the other mixtures): the run-time mode instance of k_rows2."""
    cell, pix = Call(dt, "gbev", modes[0], 3 * VEC[dt]), Call(dt, "gimg", modes[1], 3 * VEC[dt])
    pair(cell, pix)
    cell.check(f"cell {modes[0]}")
    pix.check(f"pixel {modes[1]}")


@pytest.mark.parametrize("cols", ["ent_col", "null"])
@pytest.mark.parametrize("dt", DTS)
def test_pair_identity_cols(dt, cols):
    """The pixel side over a map whose columns are the identity: with ent_col (per-column partials of one
    product each), and with ent_col = NULL plus SHPL_CSR_IDENTITY_COLS (the plain sum) -- alone and paired,
    row-keyed, flat and once."""
    for order in ("trans", "gimg"):
        c = _csr("ident", order, True)
        s = c if cols == "ent_col" else _with(c, ent_col=None, flags=L.CSR_IDENTITY_COLS)
        cell, pix = Call(dt, "pool", "CONCAT", 3 * VEC[dt], mname="ident"), \
            Call(dt, order, "CONCAT", 3 * VEC[dt], mname="ident")
        pair(cell, pix, pix_csr=s)
        cell.check("cell")
        pix.check(f"pixel {order}")
        for form in ("rows", "once", "flat"):
            call = Call(dt, order, "POOL", 9 * VEC[dt], mname="ident")
            f = _csr("ident", order, False)
            one = s if form != "flat" else f if cols == "ent_col" else _with(f, ent_col=None,
                                                                            flags=L.CSR_IDENTITY_COLS)
            launch(form, call, csr=one)
            call.check(f"{form} {order}")


@pytest.mark.parametrize("case", ["f32_bf16", "bf16_f32", "vec_scalar", "scalar_vec"])
def test_pair_two_launches(case):
    """f32 beside bf16, a vector side beside a scalar one: shpl_pull_pair falls back to two launches."""
    dc, dp = {"f32_bf16": (F32, BF16), "bf16_f32": (BF16, F32)}.get(case, (F32, F32))
    cc = 3 if case == "scalar_vec" else 3 * VEC[dc]
    cp = 3 if case == "vec_scalar" else 3 * VEC[dp]
    for mode in ("CONCAT", "ADD"):
        cell, pix = Call(dc, "pool", mode, cc), Call(dp, "trans", mode, cp)
        assert (cell.dt, cell.vec()) != (pix.dt, pix.vec())
        pair(cell, pix)
        cell.check(f"cell {mode}")
        pix.check(f"pixel {mode}")


@pytest.mark.parametrize("side", ["cell", "pixel"])
@pytest.mark.parametrize("how", ["null", "empty_map"])
@pytest.mark.parametrize("dt", DTS)
def test_pair_one_side(dt, how, side):
    """Either side NULL, either side the empty map (whose pull is the streaming pass alone)."""
    for mode in ("POOL", "CONCAT", "ADD"):
        cell = Call(dt, "pool", mode, 3 * VEC[dt], mname="empty" if (how, side) == ("empty_map", "cell") else "main")
        pix = Call(dt, "trans", mode, 3 * VEC[dt], mname="empty" if (how, side) == ("empty_map", "pixel") else "main")
        if how == "null":
            pair(None if side == "cell" else cell, None if side == "pixel" else pix)
            (pix if side == "cell" else cell).check(mode)
            assert (cell if side == "cell" else pix).untouched()
        else:
            pair(cell, pix)
            cell.check(f"cell {mode}")
            pix.check(f"pixel {mode}")


@pytest.mark.parametrize("wide", ["cell", "pixel"])
@pytest.mark.parametrize("dt", DTS)
def test_pair_narrow_beside_wide(dt, wide):
    """1 chunk beside 65: the lane group (G = 64) comes from the wider side, the narrow side runs in it."""
    for mode in ("CONCAT", "ADD"):
        cell = Call(dt, "pool", mode, (65 if wide == "cell" else 1) * VEC[dt])
        pix = Call(dt, "trans", mode, (65 if wide == "pixel" else 1) * VEC[dt])
        pair(cell, pix)
        cell.check(f"cell {mode}")
        pix.check(f"pixel {mode}")


@pytest.mark.parametrize("form", ["once", "pair"])
@pytest.mark.parametrize("dt", DTS)
def test_empty_map(dt, form):
    """Matrix item 8: the empty map through shpl_pull_once (both keys) and shpl_pull_pair (every mode):
    zeros, the pass-through copy, pass + 0 (-0 -> +0)."""
    for c in (3 * VEC[dt], 3):
        if form == "once":
            for order in ORD:
                call = Call(dt, order, "POOL", c, mname="empty")
                launch("once", call)
                call.check(f"once {order}")
        else:
            for mode in ("POOL", "CONCAT", "ADD"):
                cell, pix = Call(dt, "pool", mode, c, mname="empty"), Call(dt, "gimg", mode, c, mname="empty")
                pair(cell, pix)
                cell.check(f"cell {mode}")
                pix.check(f"pixel {mode}")


@pytest.mark.parametrize("order", ["pool", "trans"])
@pytest.mark.parametrize("dt", DTS)
def test_capacity_second_round(dt, order):
    """3000 live entries in 2048 * 320 capacity slots, flat form: every workgroup of k_sparse_long scans its
    320 slots in two rounds, and a run of 20 starts in the second (asserted from the CSR in _csr)."""
    for mode in ("POOL", "ADD"):
        call = Call(dt, order, mode, 3 * VEC[dt], mname="cap")
        launch("flat", call)
        call.check(f"flat {mode}")


@pytest.mark.parametrize("order", list(ORD))
@pytest.mark.parametrize("dt", DTS)
def test_tiny_capacity(dt, order):
    """A capacity of at most LONG_RUN slots: k_sparse takes every run itself (no k_sparse_long launch)."""
    for c in (2 * VEC[dt], 3 * VEC[dt], 3):
        for form in ("flat", "rows", "once"):
            call = Call(dt, order, "POOL" if form == "once" else "ADD", c, mname="tiny")
            launch(form, call)
            call.check(f"{form} c {c}")


def _status_cases():
    """(name, fields of the call to replace, fields of the CSR struct to replace, expected status) over a
    valid CONCAT call: every SHPL_ERR_ARG / SHPL_ERR_BAD_SHAPE branch of plan()."""
    big = 1 << 31
    return [
        ("null_csr", {}, None, L.ERR_ARG),
        ("direction", {"direction": 2}, {}, L.ERR_ARG),
        ("dtype", {"dtype": L.F64}, {}, L.ERR_ARG),
        ("mode_high", {"mode": 3}, {}, L.ERR_ARG),
        ("mode_low", {"mode": -1}, {}, L.ERR_ARG),
        ("n_keys_negative", {}, {"n_keys": -1}, L.ERR_BAD_SHAPE),
        ("c_pool_negative", {"c_pool": -1}, {}, L.ERR_BAD_SHAPE),
        ("c_pass_negative", {"c_pass": -1}, {}, L.ERR_BAD_SHAPE),
        ("null_out", {"out": None}, {}, L.ERR_ARG),
        ("null_src", {"src": None}, {}, L.ERR_ARG),
        ("null_pass_concat", {"pass_": None}, {}, L.ERR_ARG),
        ("null_pass_add", {"pass_": None, "mode": L.OUT_ADD, "c_pass": 12}, {}, L.ERR_ARG),
        ("null_ent_dst", {}, {"ent_dst": None}, L.ERR_ARG),
        ("null_ent_src", {}, {"ent_src": None}, L.ERR_ARG),
        ("null_ent_val", {}, {"ent_val": None}, L.ERR_ARG),
        ("pixel_without_columns", {"direction": L.BY_PIXEL}, {"ent_col": None}, L.ERR_ARG),
        ("add_widths_differ", {"mode": L.OUT_ADD}, {}, L.ERR_BAD_SHAPE),
        ("head_k_0", {}, {"heads": 256, "head_k": 0}, L.ERR_ARG),
        ("head_k_33", {}, {"heads": 256, "head_k": 33}, L.ERR_ARG),
        ("heads_without_key_range", {}, {"heads": 256, "head_k": 8, "key_range": None}, L.ERR_ARG),
        ("out_stride_small", {"out_stride": 19}, {}, L.ERR_BAD_SHAPE),
        ("src_stride_small", {"src_stride": 19}, {}, L.ERR_BAD_SHAPE),
        ("pass_stride_small", {"pass_stride": 23}, {}, L.ERR_BAD_SHAPE),
        ("out_stride_2_31", {"out_stride": big}, {}, L.ERR_BAD_SHAPE),
        ("src_stride_2_31", {"src_stride": big}, {}, L.ERR_BAD_SHAPE),
        ("pass_stride_2_31", {"pass_stride": big}, {}, L.ERR_BAD_SHAPE),
    ]


@pytest.mark.parametrize("case", _status_cases(), ids=[c[0] for c in _status_cases()])
def test_statuses(case):
    """Matrix item 9: every argument / shape error of plan() through each entry point that takes it, and
    the entry points' own checks; all return before any launch, so the sentinel output is unchanged."""
    name, argf, csrf, want = case
    lib = L.lib()
    # the valid call: CONCAT of 12 pooled f32 channels at src_off 8 after 8 pass-through channels at pass_off 16
    call = Call(F32, "pool", "CONCAT", 12)
    assert (call.src_stride, call.pass_stride, call.out_stride) == (28, 32, 28)
    base = _csr("main", "pool", True)
    a = dict(direction=L.BY_CELL, dtype=L.F32, src=call.src, src_stride=call.src_stride, src_off=call.src_off,
             c_pool=call.c_pool, pass_=call.pass_, pass_stride=call.pass_stride, pass_off=call.pass_off,
             c_pass=call.c_pass, mode=call.mode, out=call.out, out_stride=call.out_stride)
    ok = (a["direction"], a["dtype"], base.ref(), L.ptr(a["src"]), a["src_stride"], a["src_off"], a["c_pool"],
          L.ptr(a["pass_"]), a["pass_stride"], a["pass_off"], a["c_pass"], a["mode"], L.ptr(a["out"]),
          a["out_stride"], _stream())
    a.update(argf)
    s = None if csrf is None else _with(base, **csrf)
    sref = None if s is None else ctypes.byref(s)
    args = (a["direction"], a["dtype"], sref, L.ptr(a["src"]), a["src_stride"], a["src_off"], a["c_pool"],
            L.ptr(a["pass_"]), a["pass_stride"], a["pass_off"], a["c_pass"], a["mode"], L.ptr(a["out"]),
            a["out_stride"], _stream())
    for fn in (lib.shpl_pull, lib.shpl_pull_dense, lib.shpl_pull_sparse, lib.shpl_pull_once):
        assert fn(*args) == want, (name, fn.__name__)
    if a["direction"] in (L.BY_CELL, L.BY_PIXEL):
        d = L.pull_desc(a["dtype"], a["src"], a["src_stride"], a["src_off"], a["c_pool"], a["pass_"],
                        a["pass_stride"], a["pass_off"], a["c_pass"], a["mode"], a["out"], a["out_stride"])
        if a["direction"] == L.BY_CELL:
            assert lib.shpl_pull_pair(sref, ctypes.byref(d), None, None, _stream()) == want, name
        else:
            assert lib.shpl_pull_pair(None, None, sref, ctypes.byref(d), _stream()) == want, name
    if name == "null_csr":
        # the entry points' own checks: shpl_pull_once with another mode or without key_range, shpl_pull_pair
        # with a CSR without key_range (a descriptor without a CSR is the case above)
        assert lib.shpl_pull_once(*ok) == L.ERR_ARG  # CONCAT
        pool = list(ok)
        pool[11] = L.OUT_POOL
        for mode in (L.OUT_CONCAT, L.OUT_ADD):
            bad = list(pool)
            bad[11], bad[10] = mode, 12
            assert lib.shpl_pull_once(*bad) == L.ERR_ARG
        flat = _csr("main", "pool", False)
        pool[2] = flat.ref()
        assert lib.shpl_pull_once(*pool) == L.ERR_ARG
        d = call.desc()
        assert lib.shpl_pull_pair(flat.ref(), ctypes.byref(d), None, None, _stream()) == L.ERR_ARG
        pflat = _csr("main", "trans", False)
        assert lib.shpl_pull_pair(None, None, pflat.ref(), ctypes.byref(d), _stream()) == L.ERR_ARG
        assert lib.shpl_pull_pair(base.ref(), ctypes.byref(d), None, ctypes.byref(d), _stream()) == L.ERR_ARG
    torch.cuda.synchronize()
    assert call.untouched(), name
