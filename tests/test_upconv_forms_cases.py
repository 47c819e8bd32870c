"""The case table of tests/test_gpu_upconv_forms.py without a GPU: its cases reach each of the 12 k_upconv3x3, the
6 k_upconv3x3_wgrad and the 6 k_upconv3x3_dgrad (type x NB) instantiations, exactly as its docstring's table says;
its Python restatements of dg_plan and uw_plan / wgrad_groups agree with the library's workspace sizes for every
case; dense_map holds the properties the upconv instantiations of find_runs and stage_halo hang on; and the
multi-tile weight gradient case walks the groups it is there for."""
import numpy as np
import pytest

import rows_map as rm
import test_gpu_conv_rows as R
import test_gpu_conv_tiled as T
import test_gpu_upconv as base
import test_gpu_upconv_forms as U

TYPES = ("float", "bf16")
FWD = ["k_upconv3x3<%s,%d,%d,%d>" % ((t,) + k) for t in TYPES
       for k in ((0, 0, 0), (0, 1, 0), (1, 0, 0), (1, 1, 0), (1, 0, 1), (1, 1, 1))]
WGRAD = ["k_upconv3x3_wgrad<%s,%d,%d>" % ((t,) + k) for t in TYPES for k in ((0, 0), (1, 0), (1, 1))]
DGRAD = ["k_upconv3x3_dgrad<%s,%d>" % (t, nb) for t in TYPES for nb in (1, 2, 4)]
POOL_BATCH, SCAN, BALLOT = 4, 256, 64  # entries per load batch, per scan round, per ballot round


def _derived(name):
    """The instantiation of a case from its arguments (not from what the table declares)."""
    fn, a = U.CASES[name]
    if fn is U.case_fwd:
        bf, _, key, _, _, _, pooled, stats = a[:8]
        return "k_upconv3x3" + U.fwd_form(bf, key, pooled, stats)
    if fn is U.case_wgrad:
        bf, _, key, _, _, _, pooled = a[:7]
        return "k_upconv3x3_wgrad" + U.wgrad_form(bf, key, pooled)
    if fn is U.case_dgrad:
        return "k_upconv3x3_dgrad" + U.dgrad_form(a[0], a[2], a[3])
    return U.FORMS[name]  # the ABI cases name the form of the call they repeat through views


def test_cases_are_the_24_instantiations():
    assert len(FWD) == 12 and len(WGRAD) == 6 and len(DGRAD) == 6
    assert sorted(set(U.FORMS.values())) == sorted(FWD + WGRAD + DGRAD)  # none missing, none extra
    assert sorted(U.FORMS) == sorted(U.CASES)
    doc = U.__doc__.replace("\n", " \n")
    seen = set()
    for name in U.CASES:
        form = _derived(name)
        assert form == U.FORMS[name], name
        if "%s %s " % (form[form.index("<"):], name) in doc:  # named beside its instantiation in the table
            assert form not in seen, form
            seen.add(form)
    assert sorted(seen) == sorted(FWD + WGRAD + DGRAD)
    for kernel in ("k_upconv3x3<T, POOLED, STATS, GROUP>", "k_upconv3x3_dgrad<T, NB>",
                   "k_upconv3x3_wgrad<T, POOLED, GROUP>", "k_upwgrad_reduce"):
        assert kernel in U.__doc__
    # the channel counts the issue's paths hang on
    dg = {(a[2], a[3]) for fn, a in U.CASES.values() if fn is U.case_dgrad}
    assert {c for _, c in dg} == {32, 64, 96, 128, 160, 70, 250, 104} and {g for g, _ in dg} == {16, 24, 40, 64}
    assert {a[1] for fn, a in U.CASES.values() if fn is U.case_dgrad} == {U.DGRAD_SHAPE, U.TILE_SHAPE}
    assert U.DGRAD_CASES["dgrad-128-from-64"][3] == (32, 64, 96) and 20 in U.DGRAD_CASES["dgrad-64-from-24"][3]
    assert any(fn is U.case_fwd and a[5] == 40 and a[9] and a[8] for fn, a in U.CASES.values() if len(a) > 9)


def _shape(which, shape):
    return {"dense": (T.MAP_FRAMES,) + T.MAP_HW, "planted": None}.get(which, shape)


def test_plans_agree_with_the_library():
    """dg_plan and uw_plan, restated, against shpl_upconv3x3_dgrad_workspace_bytes and
    shpl_upconv3x3_wgrad_workspace_bytes: the packed weights n_cbg NB qa 288 32 bytes; the pooled row pointers
    F (h + 1) 4 and the partials n_groups n_cib n_cob 9 32 32 4, each region rounded up to 256."""
    from sparse_pooling_amd import _lib as L, fusion_upconv as fu
    n_d = n_w = 0
    for name, (fn, a) in U.CASES.items():
        if fn is U.case_dgrad:
            bf, (F, h, w), cg, cdx, _, plan = a
            got = U.dg_plan(bf, cg, cdx)
            assert got[:3] == plan, name
            n_cib, nb, n_cbg = plan
            assert nb == (n_cib if n_cib <= 2 else 4) and n_cbg == -(-n_cib // nb)
            assert fu.upconv_grad_ws_bytes("dgrad", L.BF16 if bf else L.F32, F, h, w, cg, 0, cdx) == got[3], name
            n_d += 1
        elif fn is U.case_wgrad:
            bf, which, _, ca, cb, cout, pooled, shape, expect = a
            F, h, w = _shape(which, shape)
            plan = U.uw_plan(bf, F, h, w, ca, cb, cout, pooled)
            assert (plan["n_tiles"], plan["tiles_per_group"], plan["n_groups"]) == expect, name
            assert plan["n_groups"] == min(1024 // (plan["n_cib"] * plan["n_cob"]), plan["n_tiles"]) \
                or plan["tiles_per_group"] > 1
            assert fu.upconv_grad_ws_bytes("wgrad", L.BF16 if bf else L.F32, F, h, w, ca, cb, cout,
                                           1000 if pooled else None) == plan["bytes"], name
            n_w += 1
    assert n_d == 20 and n_w == 24


def test_weight_gradient_groups():
    """multi: 21 tiles over 64 block pairs are 11 groups of 2 tiles, the last of 1; group 1 walks across the frame
    boundary; k_upwgrad_reduce's 4-way sum sees tails of 1, 2 and 3 past a whole round, and none on dense_map."""
    for bf in (False, True):
        p = U.uw_plan(bf, *U.MULTI_SHAPE, 256, 256, 128, True)
        assert (p["n_cib"], p["n_cob"], p["tiles_per_frame"]) == (16, 4, 3)
        assert (p["n_tiles"], p["tiles_per_group"], p["n_groups"]) == (21, 2, 11) == U.WGRAD_EXPECT["multi"]
        assert U.group_tiles(p, 0) == [(0, 0), (0, 1)]
        assert U.group_tiles(p, 1) == [(0, 2), (1, 0)]  # across a frame boundary
        assert U.group_tiles(p, 10) == [(6, 2)]  # the short last group (t1 clamped)
        assert sum(len(U.group_tiles(p, g)) for g in range(p["n_groups"])) == p["n_tiles"]
        assert p["n_groups"] // 4 == 2 and p["n_groups"] % 4 == 3
        for F, tail in ((5, 1), (6, 2), (7, 3)):
            q = U.uw_plan(bf, F, 4, 32, 256, 256, 128, False)
            assert (q["n_tiles"], q["tiles_per_group"], q["n_groups"]) == (F, 1, F) == U.WGRAD_EXPECT["groups-%d" % F]
            assert q["n_groups"] // 4 == 1 and q["n_groups"] % 4 == tail
        # 40 + 24 -> 40: the pooled chunks start mid-block; at bf16 the chunk layout is wider than c_a
        q = U.uw_plan(bf, 2, 10, 40, 40, 24, 40, True)
        ck = U.chunk(bf)
        assert -(-40 // ck) * ck % 32 != 0 and (q["n_cib"], q["n_cob"]) == ((3, 2) if bf else (2, 2))
        assert (-(-40 // ck) * ck != 40) == bf


def _runs(counts, f, rows, x_lo, x_hi):
    """Run lengths in find_runs' order over the given map rows and cells [x_lo, x_hi) (clipped to the map)."""
    H, W = counts.shape[1:]
    out = []
    for y in rows:
        if 0 <= y < H:
            out += [int(c) for c in counts[f, y, max(x_lo, 0):min(x_hi, W)] if c]
    return out


@pytest.mark.parametrize("what,rows,left,width", [("forward <9, 33>", range(-1, U.TH), -1, 33),
                                                  ("weight gradient <4, 32>", range(0, U.WTH), 0, 32)])
def test_dense_map_reaches_the_upconv_staging_paths(what, rows, left, width):
    """find_runs over the upconv halo (rows y0-1 .. y0+7, cells x0-1 .. x0+31) and over the weight gradient's tile
    (rows y0 .. y0+3, cells x0 .. x0+31): the second ballot round inside and before the window, several scan
    rounds with a run opening in one and closing in the next, stage_halo past 256 (run, piece) pairs, and runs
    longer than POOL_BATCH."""
    counts = T.dense_map(False)["counts"]
    np.testing.assert_array_equal(counts, T.dense_map(True)["counts"])  # the same targets under either key
    F, H, W = counts.shape
    th = len(rows) - (1 if left < 0 else 0)
    window = before = straddle = False
    for f in range(F):
        for y0 in range(0, H, th):
            for x0 in range(0, W, U.TW):
                ys = [y0 + r for r in rows if 0 <= y0 + r < H]
                lo, hi = max(x0 + left, 0), min(x0 + left + width, W)
                window |= any(counts[f, y, lo:hi].sum() > BALLOT for y in ys)
                if x0 == U.TW:  # tile column 1: the row's entries left of the window come first
                    before |= any(counts[f, y, :lo].sum() > BALLOT for y in ys)
                runs = _runs(counts, f, [y0 + r for r in rows], x0 + left, x0 + left + width)
                ends = set(np.cumsum(runs).tolist())
                straddle |= sum(runs) > SCAN and any(b not in ends for b in range(SCAN, sum(runs), SCAN))
    assert window, what + ": a window row range over 64 entries"
    assert before, what + ": a row with over 64 entries left of the window of tile column 1"
    assert straddle, what + ": a tile over 256 entries with a run straddling a multiple of 256"
    assert counts.max() > POOL_BATCH
    if left < 0:  # the forward's stage_halo: more than 256 (run, piece) pairs in one tile
        assert 2 * len(_runs(counts, 0, range(-1, U.TH), -1, 32)) > 256


def test_other_maps():
    m = rm.make("cell", (1, 1, 1))
    assert m["n_frame"] == [5] and m["counts"].max() > POOL_BATCH  # the one cell holds a run past a load batch
    for v in ("cell", "pixel"):
        m = rm.make(v, U.MULTI_SHAPE)
        assert min(m["n_frame"]) > 0 and m["counts"].shape == U.MULTI_SHAPE
        # every weight-gradient tile (4 x 32) of every frame holds runs: the pooled staging runs in each tile
        assert (m["counts"].reshape(7, 3, 4, 32).sum((2, 3)) > 0).all()
    # the planted map: the per-column order differs from a plain sum at the plants (asserted where it is made)
    R._pool_ref("planted", 16, 32, R.SHAPE)


def test_nine_matmuls_are_the_definition():
    rng = np.random.default_rng(3)
    x, g = rng.standard_normal((2, 5, 7, 6)), rng.standard_normal((2, 10, 14, 4))
    np.testing.assert_allclose(U.dw9(x, g), base.upconv_dw(x, g), rtol=1e-12, atol=1e-12)
