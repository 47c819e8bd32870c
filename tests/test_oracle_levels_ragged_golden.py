"""The CPU oracle, called once per frame and level with the frame's OWN image size and that level's (stride,
bv_size), against the reference run of tests/golden/levels_ragged.npz (written by
tests/golden/make_levels_ragged_golden.py): three frames at 1224x370, 1238x374 and 620x188, the AVOD pair and the
pyramid P2..P5. CPU only. The GPU tests of shpl_build_index_levels_ragged take their expectations from the same
oracle calls (tests/levels_ragged_cases.py)."""
import os

import numpy as np
import pytest

import levels_cases as lc
import levels_ragged_cases as lrc
import ragged_cases as rc


@pytest.mark.parametrize("name", ["pair", "pyramid"])
def test_oracle_per_frame_and_level_matches_reference(name):
    g = lrc.golden()
    levels = lc.golden_levels(g, name)
    assert levels == [((float(s[0]), float(s[1])), b) for s, b in lrc.SETS[name]]
    assert tuple(g["padded"]) == rc.PADDED and [tuple(s) for s in g["sizes"]] == lrc.GOLDEN_SIZES
    for f in range(3):
        refs = lrc.oracle_levels(g[f"points_{f}"], g[f"voxels_{f}"], g["P"], levels, g["sizes"][f])
        for lv, ref in enumerate(refs):
            np.testing.assert_array_equal(ref["Mij_pool"], g[f"{name}_mij_{lv}_{f}"].reshape(-1, 2))
            np.testing.assert_array_equal(ref["img_index_flip_pool"], g[f"{name}_flip_{lv}_{f}"].reshape(-1, 3))
            np.testing.assert_array_equal(ref["M_size"], g[f"{name}_msize_{lv}_{f}"])


def test_fixture_tells_levels_and_sizes_apart():
    """The pair's nnz differ in every frame, every hand-placed edge row is among the voxels, and at least two
    frames differ from the oracle at the padded size (here all three do, at the pair)."""
    g = lrc.golden()
    levels = lc.golden_levels(g, "pair")
    differ = 0
    for f in range(3):
        assert g[f"pair_msize_0_{f}"][1] != g[f"pair_msize_1_{f}"][1]
        assert g[f"pair_msize_0_{f}"][0] == 700 * 800 and g[f"pair_msize_1_{f}"][0] == 88 * 100
        assert set((699, 700, 703, 704)) <= set(g[f"voxels_{f}"][:, 1].tolist())
        pad = lrc.oracle_levels(g[f"points_{f}"], g[f"voxels_{f}"], g["P"], levels, rc.PADDED)
        differ += any(pad[lv]["Mij_pool"].shape[0] != g[f"pair_msize_{lv}_{f}"][1] or
                      not np.array_equal(pad[lv]["img_index_flip_pool"], g[f"pair_flip_{lv}_{f}"].reshape(-1, 3))
                      for lv in range(2))
    assert differ >= 2


def test_fixture_is_small_and_data_only():
    assert os.path.getsize(lrc.GOLDEN) < 100 * 1024
    g = np.load(lrc.GOLDEN, allow_pickle=False)  # plain arrays: no pickled objects
    assert all(g[k].dtype.kind in "fiu" for k in g.files)
    assert not os.path.basename(lrc.GOLDEN).startswith("index_")  # those are read as single-frame goldens


@pytest.mark.parametrize("name", ["pair", "pyramid"])
def test_base_batch_preconditions_hold(name):
    """The GPU tests' base batch, from the oracle alone (levels_ragged_cases.base_preconditions), and the clamp
    counts the frames' own strided sizes produce: frame 2 (620x188) 11 / 29 / 58 entries at strides 8 / 16 / 32,
    frame 0 (1224x370) some at strides 16 and 32."""
    refs, clamped = lrc.base_preconditions(name)
    by_stride = {int(s[0]): c for (s, _), c in zip(lrc.SETS[name], clamped)}
    assert by_stride[8][2] == 11
    if name == "pyramid":
        assert (by_stride[16][2], by_stride[32][2]) == (29, 58)
        assert by_stride[16][0] >= 1 and by_stride[32][0] >= 1 and by_stride[4] == [0, 0, 0, 0, 0]
