"""The row-streaming bf16 conv kernels (k_conv_rows, k_wgrad_rows with k_wgrad_rows_sum / _final, and the prep
kernels k_occ_frame / k_pool_runs of shpl_conv_rows.hip), pinned in every dispatch form on MI355X.

Every case makes three kinds of assertion: the result is within the existing bound of the CPU oracle (the
tolerances and helpers of tests/test_gpu_conv.py, tests/test_gpu_conv_grad.py and tests/test_gpu_conv_tiled.py,
imported, not re-derived); the bitwise identities the code states hold where they apply (two sources on a chunk
boundary == their concatenation; pooled over a CSR == the dense form over the materialised map, which is itself
bitwise the oracle's pooled map rounded once; a two-map input gradient == the one map, split); and the SHA-256 of
the output's bytes equals the value recorded in tests/golden/conv_rows_bits.json
(tests/golden/make_conv_rows_bits.py, which runs these same case functions). The table is self-referential: a
pin for later refactors, the oracle bounds and identities carry the correctness claim.

Every forward case asserts ``fc.rows_form(...)``; tests/test_conv_rows_cases.py proves without a GPU that the
forward cases' keys are exactly KEYS, the 42 instantiations of rows::launch, and that the library's predicate
agrees. Pooled cases read the hand-made maps of tests/rows_map.py (2 x 61 x 70: bands of 31 and 30 rows, strips
of 32, 32 and 6 columns) and the planted map of tests/grouped_map.py.

Particulars named below (shpl_conv_rows.hip): m16 (even Q: 16x16x32 MFMAs, odd Q: 32x32x16), streg (statistics
summed from registers; otherwise through an LDS transpose), offsets_in_lds (the per-lane DMA offsets kept in LDS),
occ2_form (out2 stored at occupied cells only), rows_wpe_min (built at one wave per SIMD).

k_conv_rows<Q, QA, CMP, RELU, ST> -> case id (FWD_CASES; "p": B pooled)

    <1,1,0,0,0> fwd-16+0-32-raw         <1,1,0,1,0> fwd-8+0-32-relu          <1,1,0,0,1> fwd-16+0-32-stats
    <2,2,0,0,0> fwd-32+0-32-raw         <2,2,0,1,0> fwd-24+0-64-relu         <2,2,0,0,1> fwd-32+0-64-stats
    <3,3,0,0,0> fwd-48+0-32-raw         <3,3,0,1,0> fwd-40+0-32-relu         <3,3,0,0,1> fwd-48+0-32-stats
    <4,4,0,0,0> fwd-64+0-64-raw         <4,4,0,1,0> fwd-56+0-32-relu         <4,4,0,0,1> fwd-64+0-32-stats
    <2,1,0,0,0> fwd-8+8-32-raw          <2,1,0,1,0> fwd-16+16-32-relu        <2,1,0,0,1> fwd-16+16-32-stats
    <2,1,1,0,0> fwd-16+8p-32-raw        <2,1,1,1,0> fwd-16+16p-32-relu       <2,1,1,0,1> fwd-16+16p-32-stats
    <3,1,0,0,0> fwd-16+32-32-raw        <3,1,0,1,0> fwd-16+24-32-relu
    <3,1,1,0,0> fwd-16+32p-32-raw       <3,1,1,1,0> fwd-16+24p-32-relu
    <3,2,0,0,0> fwd-24+8-32-raw         <3,2,0,1,0> fwd-32+16-32-relu
    <3,2,1,0,0> fwd-32+16p-32-raw       <3,2,1,1,0> fwd-32+8p-32-relu
    <4,1,0,0,0> fwd-16+48-32-raw        <4,1,0,1,0> fwd-16+40-32-relu        <4,1,0,0,1> fwd-16+48-32-stats
    <4,1,1,0,0> fwd-16+48p-32-raw       <4,1,1,1,0> fwd-16+40p-32-relu
    <4,2,0,0,0> fwd-32+32-32-raw        <4,2,0,1,0> fwd-32+24-32-relu        <4,2,0,0,1> fwd-32+32-32-stats
    <4,2,1,0,0> fwd-32+32p-32-raw       <4,2,1,1,0> fwd-32+32p-64-relu       <4,2,1,0,1> fwd-32+32p-32-stats
    <4,3,0,0,0> fwd-48+16-32-raw        <4,3,0,1,0> fwd-40+8-32-relu         <4,3,0,0,1> fwd-48+16-32-stats
    <4,3,1,0,0> fwd-48+16p-32-raw       <4,3,1,1,0> fwd-48+16p-32-relu

  Further cases on forms of that table: nan-16+32-{raw,relu} (<3,1,0,*,0> against the tiled kernel, a NaN input
  pixel), fwd-empty0-32+32p-32-relu (frame 0 without entries), geom-HxW (<1,1,0,1,0>: H = 1, 2, 3, 58, 59, 60 --
  one band whose n_in = H + 2 covers every residue mod RING = 3, twice -- and 61, two uneven bands; W = 1, 32, 33,
  70), dgrad-C-from-G (<Q,Q,0,0,0> with out2 / c_split: G = 16 Q gradient channels, C = 64, 96, 128 in two, three
  and four output blocks, split at every multiple of 32) and dgrad-reuse-G (occ2: G = 32 is occ2_form, G = 64
  writes out2 whole). shpl_conv3x3_dgrad_reuse takes the pooled forward's plan, whose c_out = G must be whole
  32-channel blocks: Q = 1 and Q = 3 (G = 16, 48) are SHPL_ERR_ARG there (asserted without a GPU in
  tests/test_conv_rows_cases.py), so of the occ2 forms only Q = 2 is reachable, and of the whole ones only Q = 4.

k_pool_runs<NP, GROUP> (NP = c_b / 8) -> case id

    <1..6, false>  prep-fwd-cell-16+{8..48}       and prep-wgrad-cell-32+{8..48}
    <7..8, false>  prep-wgrad-cell-32+{56,64}
    <1..6, true>   prep-fwd-pixel-16+{8..48},   prep-fwd-planted-16+{8..48}   and the prep-wgrad ones below
    <1..8, true>   prep-wgrad-pixel-32+{8..64}, prep-wgrad-planted-32+{8..64}

  None is unreachable from the public API. NP = 7 and 8 are unreachable from the forward (c_b >= 56 is four B
  chunks, which leaves none of k_conv_rows' four for A); the weight gradient reaches them. The planted map's
  pooled sums differ between the per-column order (GROUP) and a plain sum in entry order at its planted pixels
  (asserted on the CPU against grouped_map.plain_sum), so GROUP taken for the plain form fails the map identity.

k_wgrad_rows<CMP, PAIR> -> case id (2 x 61 x 70)

    <false,false>  wgrad-32+0-32, wgrad-64+32-32      <false,true>  wgrad-32+32-32, wgrad-64+0-64
    <true,true>    wgrad-32+32p-32                    <true,false>  wgrad-64+32p-32

Group / chunk configurations of k_wgrad_rows and its reductions (WGRAD_GROUPS; n_items, n_groups asserted from
the formulas of wgrad_sizes and row_geom, rows_map.wgrad_geom)

    groups-1        1 x 3 x 20,    32 -> 32:  n_items = n_groups = 1
    groups-33       3 x 2 x 347,   32 -> 32:  33 groups: k_wgrad_rows_sum's second chunk holds 1 group
    groups-34       2 x 1 x 530,   32 -> 32:  34: a 2-group tail
    groups-35       5 x 1 x 200,   32 -> 32:  35: a 3-group tail
    groups-64       2 x 2 x 1024,  32 -> 32:  64: two whole chunks
    multi-pair      65 x 61 x 3,   32 + 32 -> 256:  130 items in 128 groups <false,true>; group 63 walks items
                    (31, 1, 0), (32, 0, 0) across a frame boundary, group 127 items (64, 0, 0), (64, 1, 0) across
                    a band boundary: the second item's prologue, the PAIR barrier between items, accumulators
                    carried across both kinds of boundary; four chunks in k_wgrad_rows_final
    multi-pooled    the same through rows_map.make("cell", (65, 61, 3)) <true,true>: s_occ / s_first per item

Statistics of two forms are bitwise equal only where both are streg or both are not. <4,1,0,0,1> is the one even-Q
form that is not streg, so fwd-16+48-32-stats and the one-source <4,4,0,0,1> over the concatenation are each held
to the oracle bound and their equality is recorded, not asserted (stats_41_equal_44 below): on MI355X they came out
different in the last bits, as two summation orders do.
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

import grouped_map as gm
import rows_map as rm
from oracle import shpl_oracle as orc
from sparse_pooling_amd import synth
from test_gpu_conv import ACC, DEV, TOL, _assert_within, _bf16, _bound, _np, _t, _weights
from test_gpu_conv_grad import ACC_W, _check
from test_gpu_conv_tiled import _epilogue, _rd, _vs_oracle, digest

pytestmark = pytest.mark.gpu

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_rows_bits.json")
SHAPE = (2, 61, 70)
CHUNK = 16  # bf16 channels per input chunk
# Whether fwd-16+48-32-stats' statistics came out bitwise the one-source <4,4,0,0,1> form's over the concatenation
# (set by the case; tests/golden/make_conv_rows_bits.py records it beside the table). On MI355X they did not: an
# LDS-transpose sum against a register sum, in different orders; equality is not promised and not asserted.
stats_41_equal_44 = None

# The 42 instantiations of rows::launch: (Q, QA, CMP, RELU, ST)
KEYS = [
    (1, 1, 0, 0, 0), (1, 1, 0, 1, 0), (1, 1, 0, 0, 1),
    (2, 2, 0, 0, 0), (2, 2, 0, 1, 0), (2, 2, 0, 0, 1),
    (3, 3, 0, 0, 0), (3, 3, 0, 1, 0), (3, 3, 0, 0, 1),
    (4, 4, 0, 0, 0), (4, 4, 0, 1, 0), (4, 4, 0, 0, 1),
    (2, 1, 0, 0, 0), (2, 1, 0, 1, 0), (2, 1, 1, 0, 0), (2, 1, 1, 1, 0),
    (3, 1, 0, 0, 0), (3, 1, 0, 1, 0), (3, 1, 1, 0, 0), (3, 1, 1, 1, 0),
    (3, 2, 0, 0, 0), (3, 2, 0, 1, 0), (3, 2, 1, 0, 0), (3, 2, 1, 1, 0),
    (4, 1, 0, 0, 0), (4, 1, 0, 1, 0), (4, 1, 1, 0, 0), (4, 1, 1, 1, 0),
    (4, 2, 0, 0, 0), (4, 2, 0, 1, 0), (4, 2, 1, 0, 0), (4, 2, 1, 1, 0),
    (4, 3, 0, 0, 0), (4, 3, 0, 1, 0), (4, 3, 1, 0, 0), (4, 3, 1, 1, 0),
    (2, 1, 0, 0, 1), (4, 1, 0, 0, 1), (4, 2, 0, 0, 1), (4, 3, 0, 0, 1),
    (2, 1, 1, 0, 1), (4, 2, 1, 0, 1),
]

# Forward cases (c_a, c_b, pooled, relu, stats, c_out), one per instantiation, all on 2 x 61 x 70
FWD_CASES = [
    # <1,1,0,*,*>: one chunk, 32x32x16 MFMAs, offsets in registers; NA = 2 DMAs, TA = 4 lanes in the last
    (16, 0, False, False, False, 32),
    (8, 0, False, True, False, 32),     # QA = 1 from 8 channels: A's only chunk half empty
    (16, 0, False, False, True, 32),    # statistics through the LDS transpose (odd Q: not streg)
    # <2,2,0,*,*>: m16; NA = 3, TA = 8
    (32, 0, False, False, False, 32),
    (24, 0, False, True, False, 64),    # the second chunk half empty; two output blocks
    (32, 0, False, False, True, 64),    # streg; two output blocks of partials
    # <3,3,0,*,*>: 32x32x16; NA = 4, TA = 12
    (48, 0, False, False, False, 32),
    (40, 0, False, True, False, 32),    # the third chunk half empty
    (48, 0, False, False, True, 32),    # statistics through the LDS transpose
    # <4,4,0,*,*>: m16, 144 weight registers, offsets in registers (dense, QA = 4); NA = 5, TA = 16
    (64, 0, False, False, False, 64),   # two output blocks
    (56, 0, False, True, False, 32),    # the fourth chunk half empty
    (64, 0, False, False, True, 32),    # streg
    # <2,1,*,*,*>: m16, one chunk each; NA = NB = 2, TA = TB = 4
    (8, 8, False, False, False, 32),    # QA = 1 from 8 channels, QB = 1 from 8: oracle bound only
    (16, 16, False, True, False, 32),
    (16, 8, True, False, False, 32),    # pooled, B's chunk half empty (k_pool_runs<1>)
    (16, 16, True, True, False, 32),
    # <3,1,*,*,0>: 32x32x16, B chunks skipped in rows without an occupied cell; NA = 2 / TA = 4, NB = 3 / TB = 8
    (16, 32, False, False, False, 32),
    (16, 24, False, True, False, 32),   # B's second chunk half empty
    (16, 32, True, False, False, 32),
    (16, 24, True, True, False, 32),
    # <3,2,*,*,0>: 32x32x16; NA = 3 / TA = 8, NB = 2 / TB = 4
    (24, 8, False, False, False, 32),   # A's second chunk half empty: oracle bound only
    (32, 16, False, True, False, 32),
    (32, 16, True, False, False, 32),
    (32, 8, True, True, False, 32),     # B's chunk half empty
    # <4,1,*,*,*>: m16, offsets_in_lds (QA = 1), a K-chunk of A and B pieces; NA = 2 / TA = 4, NB = 4 / TB = 12
    (16, 48, False, False, False, 32),
    (16, 40, False, True, False, 32),   # B's third chunk half empty
    (16, 48, True, False, False, 32),   # pooled K-chunk 0 holds A's pieces: never skipped; chunk 1 is
    (16, 40, True, True, False, 32),
    # <4,2,*,*,*>: m16; dense: offsets in registers; pooled: offsets_in_lds; NA = NB = 3, TA = TB = 8
    (32, 32, False, False, False, 32),
    (32, 24, False, True, False, 32),   # B's second chunk half empty
    (32, 32, True, False, False, 32),
    (32, 32, True, True, False, 64),    # two output blocks over one pooled operand
    # <4,3,*,*,*>: m16; pooled: offsets_in_lds; NA = 4 / TA = 12, NB = 2 / TB = 4
    (48, 16, False, False, False, 32),
    (40, 8, False, True, False, 32),    # A's third and B's chunk half empty: oracle bound only
    (48, 16, True, False, False, 32),   # rows_wpe_min: the one form built at one wave per SIMD
    (48, 16, True, True, False, 32),
    # the statistics forms of two sources
    (16, 16, False, False, True, 32),   # <2,1,0,0,1> streg
    (16, 48, False, False, True, 32),   # <4,1,0,0,1> the even-Q form that is not streg; offsets_in_lds
    (32, 32, False, False, True, 32),   # <4,2,0,0,1> streg
    (48, 16, False, False, True, 32),   # <4,3,0,0,1> streg
    (16, 16, True, False, True, 32),    # <2,1,1,0,1> streg, offsets_in_lds (pooled with statistics)
    (32, 32, True, False, True, 32),    # <4,2,1,0,1> streg, offsets_in_lds, one operand read ahead
]


def form_key(c_a, c_b, pooled, relu, stats):
    """(Q, QA, CMP, RELU, ST) of a forward call: 16-channel chunks of A, then of B."""
    qa, qb = (c_a + CHUNK - 1) // CHUNK, (c_b + CHUNK - 1) // CHUNK
    return (qa + qb, qa, int(pooled), int(relu), int(stats))


def streg(key):
    """shpl_conv_rows.hip's streg<Q, QA, CMP, ST>()."""
    q, qa, cmp_, _, st = key
    return bool(st) and q % 2 == 0 and not (q == 4 and qa == 1 and not cmp_)


def fwd_name(c_a, c_b, pooled, relu, stats, c_out):
    return "fwd-%d+%d%s-%d-%s" % (c_a, c_b, "p" if pooled else "", c_out,
                                  "stats" if stats else "relu" if relu else "raw")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from sparse_pooling_amd import _lib as L
    L.lib()
    assert torch.cuda.is_available()


def _same(u, v):
    """Bitwise equality (NaNs included)."""
    if u.dtype == torch.bfloat16:
        u, v = u.contiguous().view(torch.int16), v.contiguous().view(torch.int16)
    return u.shape == v.shape and torch.equal(u, v)


def _feat(shape, seed, shift=0.0):
    return _rd(synth.make_features(shape, seed) + shift)


# ------------------------------------------------------------------ pooled operands
def _smap(m):
    """The device map of rows_map.make(): packed as one frame, then its entry slots cut by frame."""
    from sparse_pooling_amd import shpl_map as sm
    p = sm.pack_map(_t(m["mij"]), _t(m["mval"]), m["m_size"], _t(m["idx"]), m["img_shape"])
    off = torch.tensor(np.concatenate([[0], np.cumsum(m["n_frame"])]), dtype=torch.int64, device=DEV)
    return sm.ShplMap(p.cell, p.col, p.val, p.pix, p.nnz_cap, p.n_cells, p.n_pix, p.n_cols, DEV, frame_off=off,
                      n_frames=len(m["n_frame"]), err=p.err)


@functools.lru_cache(maxsize=None)
def _pool_ref(variant, ca, cb, shape):
    """(map, a, b, the oracle's [a || pooled] rounded once to bf16) on the CPU; computed once per operand."""
    if variant == "planted":
        m = gm.make()
        a, b = gm.features(ca, cb)
    else:
        m = rm.make(variant, shape)
        a = _feat(shape + (ca,), 101)
        b = _feat(m["src_shape"] + (cb,), 102)
    W = a.shape[2]
    if variant in ("cell", "empty0"):
        ref, _ = orc.sparse_pool_layer(a.reshape(1, -1, W, ca), b, m["mij"], m["mval"], m["m_size"], m["idx"])
    else:
        _, ref = orc.sparse_pool_layer(b.reshape(1, -1, b.shape[2], cb), a, m["mij"], m["mval"], m["m_size"],
                                       m["idx"], dual=True)
    ref = ref.reshape(a.shape[:3] + (ca + cb,))
    if variant == "planted":  # the per-column order matters: a plain sum in entry order differs at the plants
        plain = gm.plain_sum(m, b)
        for y, x in m["planted"]:
            assert (plain[0, y, x] != ref[0, y, x, ca:]).any()
    return m, a, b, _rd(ref)


def _pooled(variant, ca, cb, shape=SHAPE):
    """Inputs of a pooled case: (a, b device tensors, pool CSR, frame_off, the materialised [a || pooled] device
    map, the oracle's [a || pooled] f32, the map). variant "cell" / "empty0": the cell-keyed CSR (a the target
    map, b the source map); "pixel": rows_map's swapped map through the pixel-keyed CSR with ent_col; "planted":
    tests/grouped_map.py (pixel-keyed, 1 x 9 x 40). The materialised map is bitwise the oracle's."""
    from sparse_pooling_amd import _lib as L, shpl_map as sm
    m, a, b, ref = _pool_ref(variant, ca, cb, shape)
    ta, tb = _bf16(a), _bf16(b)
    if variant == "planted":
        smap = sm.pack_map(_t(m["mij"]), _t(m["mval"]), m["m_size"], _t(m["idx"]), a.shape)
    else:
        smap = _smap(m)
    if variant in ("cell", "empty0"):
        pool = smap.csr(L.BY_CELL, L.ORDER_ENTRY)
        assert pool.ent_col is None
        mat = sm.pool_img_to_bev(smap, tb, ta.shape, bev=ta)
    else:
        pool = smap.csr(L.BY_PIXEL, L.ORDER_COL_ROW)
        assert pool.ent_col is not None
        mat = sm.pool_bev_to_img(smap, tb, ta.shape, img=ta)
    torch.cuda.synchronize()
    assert smap.error_bits() == 0
    np.testing.assert_array_equal(_np(mat.float()), ref)
    return ta, tb, pool, smap.frame_off, mat, ref, m


# ------------------------------------------------------------------ forward
def _conv(ta, tw, tb=None, pool=None, foff=None, epi=None, stats=False):
    """conv3x3 on k_conv_rows: with center, scale, shift + ReLU (epi) or raw, with statistics or not."""
    from sparse_pooling_amd import fusion_conv as fc
    kw = {} if epi is None else dict(center=_t(epi[0]), scale=_t(epi[1]), shift=_t(epi[2]))
    st = torch.empty((2, int(tw.shape[3])), dtype=torch.float64, device=DEV) if stats else None
    assert fc.rows_form(ta, tw, b=tb, pool=pool, frame_off=foff, relu=epi is not None, stats=stats)
    y = fc.conv3x3(ta, tw, b=tb, pool=pool, frame_off=foff, relu=epi is not None, stats=st, **kw)
    return y, st


def _outs(y, st=None):
    return {"y": y} if st is None else {"y": y, "stats": st}


def case_forward(ca, cb, pooled, relu, stats, cout, variant="cell"):
    global stats_41_equal_44
    key = form_key(ca, cb, pooled, relu, stats)
    assert key in KEYS
    w = _rd(_weights(ca + cb, cout, 4))
    tw = _bf16(w)
    epi = _epilogue(cout, 5) if relu else None
    if pooled:
        ta, tb, pool, foff, mat, x, _ = _pooled(variant, ca, cb)
        y, st = _conv(ta, tw, tb=tb, pool=pool, foff=foff, epi=epi, stats=stats)
        if ca % CHUNK == 0:  # == the dense two-source form over the materialised map (the same summation path)
            yu, su = _conv(mat[..., :ca].contiguous(), tw, tb=mat[..., ca:].contiguous(), epi=epi, stats=stats)
            assert _same(y, yu)
            if stats:
                assert streg(key) == streg(form_key(ca, cb, False, relu, stats)) and torch.equal(st, su)
    else:
        x = _feat(SHAPE + (ca + cb,), 3, 0.25 if stats else 0.0)
        if cb == 0:
            y, st = _conv(_bf16(x), tw, epi=epi, stats=stats)
        else:
            y, st = _conv(_bf16(x[..., :ca]), tw, tb=_bf16(x[..., ca:]), epi=epi, stats=stats)
            if ca % CHUNK == 0:  # A ends on a chunk: == the one-source conv of the concatenation
                y1, s1 = _conv(_bf16(x), tw, epi=epi, stats=stats)
                assert _same(y, y1)
                if stats:
                    one = form_key(ca + cb, 0, False, relu, stats)
                    _vs_oracle(y1, s1, x, w, epi, True)
                    if streg(key) == streg(one):
                        assert torch.equal(st, s1)
                    else:  # <4,1,0,0,1> against <4,4,0,0,1>: recorded, not asserted
                        assert key == (4, 1, 0, 0, 1)
                        stats_41_equal_44 = bool(torch.equal(st, s1))
    _vs_oracle(y, st, x, w, epi, True)
    return _outs(y, st)


def case_nan(relu):
    """<3,1,0,RELU,0> against the tiled kernel (an output view 2 bytes off 16-byte alignment) with center, scale
    and shift set and a NaN input pixel on the band and strip boundaries: small integers, so every accumulator
    is exact and only the epilogue can differ (test_bf16_rows_epilogue_equals_tiled's method)."""
    B, H, W = SHAPE
    ca, cb, cout = 16, 32, 32
    rng = np.random.default_rng(53)
    x = rng.integers(-3, 4, (B, H, W, ca + cb)).astype(np.float32)
    x[1, 31, 32, 3] = np.nan
    w = rng.integers(-2, 3, (3, 3, ca + cb, cout)).astype(np.float32)
    epi = _epilogue(cout, 54)
    n = B * H * W * cout
    flat = torch.empty(n + 16, dtype=torch.bfloat16, device=DEV)
    ta, tb, tw = _bf16(x[..., :ca]), _bf16(x[..., ca:]), _bf16(w)
    kw = dict(center=_t(epi[0]), scale=_t(epi[1]), shift=_t(epi[2]))
    from sparse_pooling_amd import fusion_conv as fc
    outs = []
    for off in (0, 1):  # 0: 16-byte aligned (the row kernel), 1: 2 bytes off (the tiled kernel)
        o = flat[off:off + n].view(B, H, W, cout)
        assert fc.rows_form(ta, tw, b=tb, relu=relu, out=o) == (off == 0)
        fc.conv3x3(ta, tw, b=tb, relu=relu, out=o, **kw)
        torch.cuda.synchronize()
        outs.append(o.clone())
    assert _same(outs[0], outs[1])
    bad = torch.isnan(outs[0].float())
    if not relu:  # the NaN reached the 3 x 3 pixels around it, and no other
        assert int(bad.sum()) == 9 * cout and bool(bad[1, 30:33, 31:34].all())
    xz = np.nan_to_num(x, nan=0.0)  # away from the NaN's 3 x 3 pixels the conv is that of a zero there
    ref = orc.conv3x3(xz, w, epi[0], epi[1], epi[2], relu)
    keep = np.ones((B, H, W, 1), bool)
    keep[1, 30:33, 31:34] = False
    got = np.where(keep, _np(outs[0].float()), 0.0)
    _assert_within(got, np.where(keep, ref, 0.0), _bound(xz, w, epi[1]) + np.abs(ref) * 2.0 ** -8)
    return {"y": outs[0]}


GEOM_H, GEOM_W = (1, 2, 3, 58, 59, 60, 61), (1, 32, 33, 70)


def case_geom(H, W):
    """<1,1,0,1,0> on 2 x H x W: one band of H + 2 staged rows (every residue mod RING at a full band), 61: two
    bands of 31 and 30; one partial strip, one whole, one whole + 1 column, two whole + 6."""
    strips, _, n_bands, band = rm.row_geom(H, W)
    assert (n_bands, band) == ((2, 31) if H == 61 else (1, H)) and strips == (W + 31) // 32
    x = _feat((2, H, W, 16), 41)
    w = _rd(_weights(16, 32, 42))
    epi = _epilogue(32, 43)
    y, _ = _conv(_bf16(x), _bf16(w), epi=epi)
    _vs_oracle(y, None, x, w, epi, True)
    return {"y": y}


# ------------------------------------------------------------------ input gradient
DGRAD_SHAPE = (2, 7, 70)


def case_dgrad(cg, cdx):
    """<Q,Q,0,0,0> with cdx / 32 output blocks, and out2 / c_split at every multiple of 32: the oracle bound of
    test_dgrad_bf16_two_maps; both maps bitwise the one-map form."""
    from sparse_pooling_amd import fusion_conv as fc
    g = _feat(DGRAD_SHAPE + (cg,), 21)
    w = _rd(_weights(cdx, cg, 22))
    tg, tw = _bf16(g), _bf16(w)
    assert fc.rows_form(tg, tw, relu=False, c_out=cdx) and form_key(cg, 0, False, False, False) in KEYS
    dx = fc.conv3x3_dgrad(tg, tw, cdx)
    ref = orc.conv3x3_dgrad(g, w)
    wt = np.ascontiguousarray(w[::-1, ::-1].transpose(0, 1, 3, 2))
    _, ab = orc.conv3x3(np.abs(g), np.abs(wt), raw=True)
    _check(dx.float(), ref, TOL + ACC * ab + 2.0 ** -8 * np.abs(ref), "dx")
    outs = {"dx": dx}
    for c in range(32, cdx, 32):
        da, db = fc.conv3x3_dgrad(tg, tw, cdx, split=c)
        assert da.shape[-1] == c and db.shape[-1] == cdx - c
        assert _same(torch.cat([da, db], -1), dx), c
        outs["da%d" % c], outs["db%d" % c] = da, db
    return outs


SENTINEL = -77.0  # exact in bf16


def case_dgrad_reuse(cg, stats, variant="cell"):
    """shpl_conv3x3_dgrad_reuse over the pooled forward [32 || 32 pooled] -> cg of rows_map: the first map and, at
    the occupied cells, the second are bitwise shpl_conv3x3_dgrad's. cg = 32 (Q = 2, occ2_form): every unoccupied
    cell of the second map keeps the sentinel it held; cg = 64 (Q = 4): the second map is written whole."""
    from sparse_pooling_amd import _lib as L, fusion_conv as fc
    F, H, W = SHAPE
    ta, tb, pool, foff, mat, x, m = _pooled(variant, 32, 32)
    tw = _bf16(_rd(_weights(64, cg, 61)))
    assert fc.rows_form(ta, tw, b=tb, pool=pool, frame_off=foff, relu=False, stats=stats)
    fws = L.workspace(fc.conv_ws_bytes(L.BF16, F, H, W, 32, 32, cg, pool.nnz_cap, stats), DEV)
    st = torch.empty((2, cg), dtype=torch.float64, device=DEV) if stats else None
    fc.conv3x3(ta, tw, b=tb, pool=pool, frame_off=foff, relu=False, stats=st, ws=fws)
    gy = _bf16(_feat(SHAPE + (cg,), 62))
    da, db = fc.conv3x3_dgrad(gy, tw, 64, split=32)
    ws = L.workspace(fc.conv_ws_bytes(L.BF16, F, H, W, cg, 0, 64, None, False), DEV)
    ra = torch.empty_like(da)
    rb = torch.full_like(db, SENTINEL)
    L.check(L.lib().shpl_conv3x3_dgrad_reuse(L.BF16, F, H, W, L.ptr(gy), cg, cg, L.ptr(tw), 64, L.ptr(ra), 32, 32,
                                             L.ptr(rb), 32, L.ptr(ws), ws.numel(), pool.ref(), L.ptr(fws),
                                             fws.numel(), int(stats), L.stream_of(DEV)), "shpl_conv3x3_dgrad_reuse")
    torch.cuda.synchronize()
    assert _same(ra, da)
    occ = torch.from_numpy(rm.occupied(m).reshape(-1)).to(DEV)
    assert 0 < int(occ.sum()) < occ.numel()
    flat_b, flat_r = db.reshape(-1, 32), rb.reshape(-1, 32)
    assert _same(flat_r[occ], flat_b[occ])
    if cg <= 32:
        assert bool((flat_r[~occ].float() == SENTINEL).all())
        assert bool((flat_b[~occ].float() != SENTINEL).any())
    else:
        assert _same(rb, db)
    return {"da": ra, "db": rb}


# ------------------------------------------------------------------ pooled operand prep
def case_prep_fwd(variant, cb):
    """k_occ_frame + k_pool_runs<cb / 8, GROUP> under the pooled forward [16 || cb pooled] -> 32, raw: bitwise the
    dense form over the shpl_pull map, which is bitwise the oracle's (_pooled)."""
    ta, tb, pool, foff, mat, x, _ = _pooled(variant, 16, cb)
    tw = _bf16(_rd(_weights(16 + cb, 32, 31)))
    assert form_key(16, cb, True, False, False) in KEYS
    y, _ = _conv(ta, tw, tb=tb, pool=pool, foff=foff)
    yu, _ = _conv(mat[..., :16].contiguous(), tw, tb=mat[..., 16:].contiguous())
    assert _same(y, yu)
    return {"y": y}


def case_prep_wgrad(variant, cb):
    """The same prep under the pooled weight gradient [32 || cb pooled] -> 32 (cb up to 64: NP = 1 .. 8)."""
    from sparse_pooling_amd import fusion_conv as fc
    ta, tb, pool, foff, mat, x, _ = _pooled(variant, 32, cb)
    g = _bf16(_feat(x.shape[:3] + (32,), 33))
    dw = fc.conv3x3_wgrad(ta, g, b=tb, pool=pool, frame_off=foff)
    dw_d = fc.conv3x3_wgrad(mat[..., :32].contiguous(), g, b=mat[..., 32:].contiguous())
    assert torch.equal(dw, dw_d) and bool(dw[:, :, 32:].any())
    return {"dw": dw}


# ------------------------------------------------------------------ weight gradient
def _wgrad_vs_oracle(dw, x, g):
    _check(dw, orc.conv3x3_wgrad(x, g), TOL + ACC_W * orc.conv3x3_wgrad(np.abs(x), np.abs(g)), "dw")


def case_wgrad(shape, ca, cb, cout, variant=None, expect=None):
    """k_wgrad_rows<CMP, PAIR> + k_wgrad_rows_sum / _final vs the oracle's double sums (TOL + ACC_W sum |x g|).
    Dense two sources == their concatenation bitwise (A ends on a 32-channel tile); pooled (variant) == the dense
    form over the materialised map bitwise. expect: the group geometry the case is there for."""
    from sparse_pooling_amd import fusion_conv as fc
    geo = rm.wgrad_geom(*shape, ca, cb, cout)
    if expect is not None:
        expect(geo)
    assert ca % 8 == 0 and cb % 8 == 0 and cout % 8 == 0 and (cb == 0 or ca % 32 == 0)  # rows::wgrad_supported
    g = _feat(shape + (cout,), 42)
    tg = _bf16(g)
    if variant is None:
        x = _feat(shape + (ca + cb,), 41)
        if cb == 0:
            dw = fc.conv3x3_wgrad(_bf16(x), tg)
        else:
            dw = fc.conv3x3_wgrad(_bf16(x[..., :ca]), tg, b=_bf16(x[..., ca:]))
            assert torch.equal(dw, fc.conv3x3_wgrad(_bf16(x), tg))
    else:
        ta, tb, pool, foff, mat, x, _ = _pooled(variant, ca, cb, shape)
        dw = fc.conv3x3_wgrad(ta, tg, b=tb, pool=pool, frame_off=foff)
        assert torch.equal(dw, fc.conv3x3_wgrad(mat[..., :ca].contiguous(), tg, b=mat[..., ca:].contiguous()))
    _wgrad_vs_oracle(dw, x, g)
    return {"dw": dw}


def _groups(n_items, n_groups, most=1):
    def check(geo):
        assert (geo["n_items"], geo["n_groups"]) == (n_items, n_groups), geo
        assert rm.straddles(geo)[2] == most
    return check


def _multi(geo):
    """130 items in 128 groups (n_cit n_cot = 2 x 8 = 16): groups 63 and 127 walk two items, group 63 across the
    frame boundary 31 | 32, group 127 across frame 64's band boundary."""
    assert (geo["n_items"], geo["n_groups"], geo["n_cit"], geo["n_cot"]) == (130, 128, 2, 8), geo
    assert geo["n_items"] % geo["n_groups"] != 0
    assert rm.straddles(geo) == ([63], [127], 2)
    assert rm.group_items(geo, 63) == [(31, 1, 0), (32, 0, 0)] and rm.group_items(geo, 127) == [(64, 0, 0), (64, 1, 0)]


MULTI_SHAPE = (65, 61, 3)
WGRAD_GROUPS = {  # shape, c_a, c_b, c_out, pooled variant, the geometry it is there for
    "groups-1": ((1, 3, 20), 32, 0, 32, None, _groups(1, 1)),
    "groups-33": ((3, 2, 347), 32, 0, 32, None, _groups(33, 33)),
    "groups-34": ((2, 1, 530), 32, 0, 32, None, _groups(34, 34)),
    "groups-35": ((5, 1, 200), 32, 0, 32, None, _groups(35, 35)),
    "groups-64": ((2, 2, 1024), 32, 0, 32, None, _groups(64, 64)),
    "multi-pair": (MULTI_SHAPE, 32, 32, 256, None, _multi),
    "multi-pooled": (MULTI_SHAPE, 32, 32, 256, "cell", _multi),
}
WGRAD_FORMS = [  # c_a, c_b, c_out, pooled, PAIR: k_wgrad_rows<CMP, PAIR> on 2 x 61 x 70
    (32, 0, 32, False, False), (64, 32, 32, False, False),  # <false,false>: one and three input tiles
    (32, 32, 32, False, True), (64, 0, 64, False, True),    # <false,true>: a pair from two sources, a pair inside A
    (32, 32, 32, True, True),                               # <true,true>: wave 1's tile pooled
    (64, 32, 32, True, False),                              # <true,false>: the third wave-alone tile pooled
]


def _pair(want_pair):
    def check(geo):
        assert (geo["n_cit"] % 2 == 0) == want_pair  # wgrad_launch's PAIR
        assert geo["n_items"] == 2 * 2 * 3 and geo["n_groups"] == 12  # every group one item
    return check


CASES = {}
for _c in FWD_CASES:
    CASES[fwd_name(*_c)] = (case_forward, _c)
CASES["fwd-empty0-32+32p-32-relu"] = (case_forward, (32, 32, True, True, False, 32, "empty0"))
for _relu in (False, True):
    CASES["nan-16+32-%s" % ("relu" if _relu else "raw")] = (case_nan, (_relu,))
for _h in GEOM_H:
    for _w in GEOM_W:
        CASES["geom-%dx%d" % (_h, _w)] = (case_geom, (_h, _w))
for _cg in (16, 32, 48, 64):
    for _cdx in (64, 96, 128):
        CASES["dgrad-%d-from-%d" % (_cdx, _cg)] = (case_dgrad, (_cg, _cdx))
for _cg, _st in ((32, False), (32, True), (64, False), (64, True)):
    CASES["dgrad-reuse-%d%s" % (_cg, "-stats" if _st else "")] = (case_dgrad_reuse, (_cg, _st))
CASES["dgrad-reuse-32-empty0"] = (case_dgrad_reuse, (32, False, "empty0"))
for _v in ("cell", "pixel", "planted"):
    for _cb in range(8, 49, 8):
        CASES["prep-fwd-%s-16+%d" % (_v, _cb)] = (case_prep_fwd, (_v, _cb))
    for _cb in range(8, 65, 8):
        CASES["prep-wgrad-%s-32+%d" % (_v, _cb)] = (case_prep_wgrad, (_v, _cb))
for _ca, _cb, _co, _p, _pr in WGRAD_FORMS:
    CASES["wgrad-%d+%d%s-%d" % (_ca, _cb, "p" if _p else "", _co)] = (
        case_wgrad, (SHAPE, _ca, _cb, _co, "cell" if _p else None, _pair(_pr)))
CASES["wgrad-empty0-32+32p-32"] = (case_wgrad, (SHAPE, 32, 32, 32, "empty0", None))
for _n, _a in WGRAD_GROUPS.items():
    CASES["wgrad-" + _n] = (case_wgrad, _a)


def run_case(name):
    """{output name: digest} of a case, after its oracle and identity assertions."""
    fn, args = CASES[name]
    outs = fn(*args)
    torch.cuda.synchronize()
    return {k: digest(v) for k, v in outs.items()}


@functools.lru_cache(maxsize=None)
def _table():
    with open(TABLE) as fh:
        return json.load(fh)


def test_table_lists_every_case():
    t = _table()
    assert t["pinned_to"].startswith("self")
    assert sorted(t["cases"]) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_rows_case(name):
    assert run_case(name) == _table()["cases"][name]
