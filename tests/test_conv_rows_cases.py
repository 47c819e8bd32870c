"""The case table of tests/test_gpu_conv_rows.py without a GPU: its forward cases reach exactly the 42
k_conv_rows instantiations of rows::launch, the library's own predicate (shpl_conv3x3_rows_form on fake,
never-dereferenced pointers, as tests/golden/make_conv_host_plan.py calls it) answers 1 for every case and 0 for
every (Q, QA, pooled, statistics) outside rows::supported / supported_st, the hand-made maps of tests/rows_map.py
hold the properties the kernels' paths hang on, and the weight gradient's group configurations are what the
formulas of wgrad_sizes and row_geom give."""
import importlib.util
import os

import numpy as np
import pytest

import rows_map as rm
import test_gpu_conv_rows as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_conv_host_plan", os.path.join(GOLDEN, "make_conv_host_plan.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

NF, H, W = R.SHAPE


def _rows_form(ca, cb, pooled, relu, stats, cout=32):
    from sparse_pooling_amd import _lib as L
    fn, args = gen.rows_form(gen.BF16, NF, H, W, ca, cb, cout, pool=gen.csr(NF * H * W) if pooled else None,
                             stats=int(stats), act=int(relu))
    rc, out = gen.replay(L.lib(), L, fn, args)
    assert rc == L.OK, (ca, cb, pooled, relu, stats, rc)
    return out


def test_cases_are_the_42_instantiations():
    assert len(R.KEYS) == 42 == len(set(R.KEYS)) == len(R.FWD_CASES)
    keys = [R.form_key(*c[:5]) for c in R.FWD_CASES]
    assert sorted(keys) == sorted(R.KEYS)  # none missing, none extra, none twice
    assert len({R.fwd_name(*c) for c in R.FWD_CASES}) == 42
    # the docstring's table names every instantiation beside its case
    for c, k in zip(R.FWD_CASES, keys):
        assert "<%d,%d,%d,%d,%d> %s " % (k + (R.fwd_name(*c),)) in R.__doc__.replace("\n", " \n"), (k, c)
    # channel tails inside a chunk: (3,2) with A's second chunk half empty, QA = 1 from 8 channels
    assert (24, 8) in {c[:2] for c in R.FWD_CASES} and any(c[0] == 8 for c in R.FWD_CASES)
    assert {c[5] for c in R.FWD_CASES} == {32, 64}


def test_the_literal_list_is_the_dispatch_table():
    """KEYS against rows::launch's rule, written out: supported(q, qa); pooled needs a B chunk; statistics only
    without ReLU and where supported_st allows."""
    want = set()
    for q in range(1, 5):
        for qa in range(1, q + 1):
            for cmp_ in (0, 1):
                if cmp_ and qa == q:
                    continue
                for relu in (0, 1):
                    want.add((q, qa, cmp_, relu, 0))
                st_ok = ((q, qa) in ((4, 2), (2, 1))) if cmp_ else not (q == 3 and qa < 3)
                if st_ok:
                    want.add((q, qa, cmp_, 0, 1))
    assert want == set(R.KEYS)


@pytest.mark.parametrize("case", R.FWD_CASES, ids=[R.fwd_name(*c) for c in R.FWD_CASES])
def test_library_takes_the_row_form(case):
    ca, cb, pooled, relu, stats, cout = case
    assert _rows_form(ca, cb, pooled, relu, stats, cout) == 1


def test_library_declines_what_the_list_leaves_out():
    """Every (q, qa, pooled, stats) from whole 16-channel chunks, up to five chunks: the library answers 1 exactly
    on KEYS. Among the refusals: (3,1) and (3,2) with statistics, pooled statistics at anything but (2,1) and
    (4,2), five chunks, a pooled call without a chunk of A."""
    declined = set()
    for qa in range(0, 6):
        for qb in range(0, 6 - qa):
            if qa + qb == 0:
                continue
            for pooled in (False, True):
                if pooled and qb == 0:
                    continue
                for relu, stats in ((False, False), (True, False), (False, True)):
                    key = (qa + qb, qa, int(pooled), int(relu), int(stats))
                    got = _rows_form(16 * qa, 16 * qb, pooled, relu, stats)
                    assert got == int(key in R.KEYS), key
                    if not got:
                        declined.add(key)
    for key in ((3, 1, 0, 0, 1), (3, 2, 0, 0, 1), (3, 1, 1, 0, 1), (3, 2, 1, 0, 1), (4, 1, 1, 0, 1), (4, 3, 1, 0, 1),
                (5, 4, 0, 0, 0), (4, 0, 1, 0, 0)):
        assert key in declined, key
    assert _rows_form(32, 32, False, True, True) == 0  # statistics beside a ReLU


def test_dgrad_reuse_declines_partial_output_blocks():
    """shpl_conv3x3_dgrad_reuse plans the pooled forward [c_split || c_dx - c_split pooled] -> c_gy: 16 and 48
    gradient channels (Q = 1, 3) are no whole output blocks of that forward, so of k_conv_rows' occ2 forms only
    Q = 2 and of the whole-out2 forms only Q = 4 are reachable; refused before any launch."""
    from sparse_pooling_amd import _lib as L
    one = gen.csr(176 * 200)
    for c_gy in (16, 48):
        fn, args = gen.dgrad(c_gy=c_gy, gy_stride=c_gy, reuse=(one, "P", 1 << 30, 0))
        assert gen.replay(L.lib(), L, fn, args)[0] == L.ERR_ARG


@pytest.mark.parametrize("variant", ["cell", "pixel", "empty0"])
def test_hand_made_map(variant):
    """rows_map.make asserts its properties where it builds the map; here the entries are checked against the
    counts they were drawn from, through the reference format alone."""
    m = rm.make(variant)
    F, Hm, Wm = m["shape"]
    assert (F, Hm, Wm) == R.SHAPE and rm.row_geom(Hm, Wm) == (3, 3, 2, 31)
    mij, idx = m["mij"], m["idx"]
    if variant == "pixel":
        tgt = (idx[:, 0] * Hm + idx[:, 1]) * Wm + idx[:, 2]
        tgt = tgt[mij[:, 1]]
        per_pixel_cols = np.bincount((idx[:, 0] * Hm + idx[:, 1]) * Wm + idx[:, 2], minlength=F * Hm * Wm)
        assert per_pixel_cols.max() > 1  # several columns per pixel
    else:
        tgt = mij[:, 0]
    got = np.bincount(tgt, minlength=F * Hm * Wm).reshape(F, Hm, Wm)
    np.testing.assert_array_equal(got, m["counts"])
    frame = tgt // (Hm * Wm)
    assert (np.diff(frame) >= 0).all()  # grouped by frame
    np.testing.assert_array_equal(np.bincount(frame, minlength=F), m["n_frame"])
    occ = rm.occupied(m)
    f1 = occ[1]
    assert f1[np.ix_(rm.EDGE_Y, rm.EDGE_X)].all() and not f1[rm.EMPTY_ROW].any() and f1[rm.FULL_ROW].all()
    assert f1[rm.OUTSIDE_ROW].any() and not f1[rm.OUTSIDE_ROW, 31:65].any()
    if variant == "empty0":
        assert not occ[0].any() and m["n_frame"][0] == 0
    else:
        assert m["n_frame"][0] > 0 and m["counts"][0][rm.LONG_CELL] == rm.LONG_RUN > 16
        assert set(range(1, 7)) <= set(np.unique(m["counts"]).tolist())
        assert (occ[0] != occ[1]).any()


def test_wgrad_group_configurations():
    """The group / chunk configurations of tests/test_gpu_conv_rows.py's weight gradient cases, from the item
    index arithmetic alone (WGC = 32 groups per chunk of k_wgrad_rows_sum, its loop unrolled by 4)."""
    tails = {}
    for name, (shape, ca, cb, cout, variant, expect) in R.WGRAD_GROUPS.items():
        geo = rm.wgrad_geom(*shape, ca, cb, cout)
        expect(geo)
        tails[name] = (-(-geo["n_groups"] // 32), geo["n_groups"] % 32 % 4, geo["n_groups"] % 32)
    assert tails["groups-1"] == (1, 1, 1)
    assert [tails["groups-%d" % n] for n in (33, 34, 35)] == [(2, 1, 1), (2, 2, 2), (2, 3, 3)]
    assert tails["groups-64"] == (2, 0, 0)
    assert tails["multi-pair"] == tails["multi-pooled"] == (4, 0, 0)
    geo = rm.wgrad_geom(*R.MULTI_SHAPE, 32, 32, 256)
    frame, band, most = rm.straddles(geo)
    assert frame and band and most == 2 and geo["n_items"] > geo["n_groups"]
    # every group of the forms on 2 x 61 x 70 walks one item
    for ca, cb, cout, _, _ in R.WGRAD_FORMS:
        assert rm.straddles(rm.wgrad_geom(*R.SHAPE, ca, cb, cout))[2] == 1
