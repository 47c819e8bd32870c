"""The case table of tests/test_gpu_conv_wide.py without a GPU: the digest table lists every case under the
right label; the exact cases' digests are those of the CPU oracle's result; the library's own predicate
(shpl_conv3x3_wide_form on fake, never-dereferenced pointers, as tests/golden/make_conv_host_plan.py calls it)
answers for every case the form its row names; the hand-made maps hold the properties the kernel's paths hang
on; and the cases reach every (chunks, chunks of A, second operand, output blocks), tile shape, grid and
epilogue the kernel has."""
import importlib.util
import os

import numpy as np
import pytest

import test_gpu_conv_wide as Wd

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_conv_host_plan", os.path.join(GOLDEN, "make_conv_host_plan.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

EXACT = [n for n, c in Wd.CASES.items() if c.data == "x"]


def test_table_lists_every_case():
    t = Wd.table()
    assert sorted(t) == sorted(Wd.CASES)
    for name, c in Wd.CASES.items():
        assert t[name]["pinned_to"] == ("oracle" if c.data == "x" else "gpu"), name
        assert t[name]["digests"] and all(len(d) == 64 for d in t[name]["digests"].values()), name


@pytest.mark.parametrize("name", EXACT)
def test_exact_digests_are_the_oracles(name):
    """oracle_bits asserts the premise (whole halves, whole weights, twice sum |x| |w| < 2^24) as it goes."""
    got = {k: Wd.sha(v) for k, v in Wd.oracle_bits(Wd.CASES[name]).items()}
    assert got == Wd.table()[name]["digests"]


def test_exact_data_are_what_the_premise_names():
    for name in EXACT:
        c = Wd.CASES[name]
        a, b, w, (center, scale, shift) = Wd.inputs(c)
        if c.fn == "frame31":
            a = np.concatenate([v.reshape(-1) for v in Wd.big_blocks()])
        assert center is None and scale is None
        assert set(np.unique(a)) <= set(range(-3, 4)) and set(np.unique(w)) == set(range(-2, 3)), name
        assert b is None or set(np.unique(b)) <= set(range(-3, 4)), name
        assert shift is None or np.array_equal(shift, np.round(shift)), name
        if c.kind in ("cmp", "map") and c.fn != "empty_pool":
            m, _ = Wd.case_map(c)
            assert set(np.unique(m["mval"])) <= set(Wd.POOL_VALUES.tolist()) and m["counts"].max() <= 11, name


@pytest.mark.parametrize("name", list(Wd.CASES))
def test_library_answers_the_form_the_case_names(name):
    from sparse_pooling_amd import _lib as L
    c = Wd.CASES[name]
    shape, kw = Wd.abi_call(c)
    if "pool" in kw:
        kw["pool"] = gen.csr(int(np.prod(c.shape)), cap=kw["pool"])
    fn, args = gen.wide_form(gen.BF16, *shape, **kw)
    assert gen.replay(L.lib(), L, fn, args) == (L.OK, c.form), name


def test_hand_made_map():
    m = Wd.hand_map()
    F, H, W = Wd.HAND_SHAPE
    tgt = m["mij"][:, 0]
    np.testing.assert_array_equal(np.bincount(tgt, minlength=F * H * W).reshape(F, H, W), m["counts"])
    frame = tgt // (H * W)
    assert (np.diff(frame) >= 0).all() and list(np.bincount(frame, minlength=F)) == m["n_frame"]
    occ = m["counts"] > 0
    assert m["n_frame"][0] == 0 and m["n_frame"][1] > 0 and not occ[0].any()   # frame_off[1] == 0
    assert occ[1, Wd.HAND_ROW, 31] and occ[1, Wd.HAND_ROW, 32]                   # both sides of a word boundary
    assert occ[1, H - 1, W - 1]                                                  # the last pixel of the last frame
    assert occ[1, 0].all()                                                       # a fully occupied first row
    (y0, x0), (cy, cx) = Wd.HAND_TILE, Wd.HAND_CORNER
    assert y0 % Wd.TILE == 0 and x0 % Wd.TILE == 0 and (cy, cx) == (y0 - 1, x0 + Wd.TILE)
    halo = np.zeros((H, W), bool)
    halo[max(y0 - 1, 0):y0 + Wd.TILE + 1, max(x0 - 1, 0):x0 + Wd.TILE + 1] = True
    assert (occ[1] & halo).sum() == 1 and occ[1, cy, cx]                         # one run, on the halo's corner
    assert 1 < m["counts"].max() <= 10 and (m["idx"][:, 0] == frame).all()
    # the source pixels of an entry's column lie in the source map
    assert (m["idx"][:, 1] < Wd.SRC_HW[0]).all() and (m["idx"][:, 2] < Wd.SRC_HW[1]).all()


def test_tall_map_reaches_past_the_occupancy_table():
    H, W = Wd.TALL_HW
    assert H * ((W + 31) // 32) == 18432 + 1                                     # rows::OCC_MAX_WORDS + 1
    for exact in (True, False):
        m = Wd.tall_map(exact)
        assert m["counts"][0, 0].all() and m["counts"][0, -1].all()


def test_cases_reach_every_form():
    cases = list(Wd.CASES.values())
    by = lambda data: {Wd.reach(c)[:3] for c in cases if c.data == data and c.form}  # noqa: E731
    want = {(2, 2, "none"), (2, 1, "dense"), (3, 2, "dense"), (3, 1, "dense"), (8, 4, "dense"), (2, 1, "cmp"),
            (2, 1, "map")}
    assert want <= by("x") and want <= by("f")
    for data in "xf":
        assert {Wd.reach(c)[3] for c in cases if c.data == data and c.form} == {1, 2}
        dense = [c for c in cases if c.fn == "dense" and c.data == data]
        assert {(1, 1), (16, 16), (17, 17), (1, 40), (40, 1)} <= {c.shape[1:] for c in dense}
        tiles = {c.shape[0] * -(-c.shape[1] // Wd.TILE) * -(-c.shape[2] // Wd.TILE) for c in dense}
        assert 9 in tiles                                                        # no multiple of the 8 XCDs
        assert {c.form for c in cases if c.fn == "view" and c.data == data} >= {1}
        assert {c.extra["key"] for c in cases if c.fn == "pooled" and c.data == data} == {"cell", "pixel"}
        assert {c.extra["map"] for c in cases if c.fn == "pooled" and c.data == data} == {"dense", "hand"}
        assert any(c.fn == "empty_pool" and c.data == data for c in cases)
    assert 16 in {c.shape[0] * -(-c.shape[1] // Wd.TILE) * -(-c.shape[2] // Wd.TILE) for c in cases}  # two XCD rounds
    assert {(c.epi, c.relu) for c in cases if c.data == "f" and c.form == 1} >= {
        (e, r) for e in Wd.EPILOGUES for r in (False, True)}
    assert any(c.extra.get("zeros") for c in cases)
    assert {c.extra["off"]: c.form for c in cases if c.fn == "view"} == {8: 1, 3: 0}
    big = [c for c in cases if c.fn == "frame31"]
    assert len(big) == 1 and big[0].form == 0 and big[0].data == "x"
    (H, W), S = Wd.BIG_HW, Wd.BIG_STRIDE
    assert 2 ** 31 <= (H * W - 1) * S * 2 and H * W * S * 2 < 2 ** 32             # a wrapped offset is negative
