"""The CPU oracle, called once per frame and level with that level's (stride, bv_size), against the reference run
of tests/golden/levels_avod.npz (written by tests/golden/make_levels_golden.py): the AVOD pair -- stride 1 over
BEV 700 x 800, stride 8 over the BEV input padded to 704 rows -- and the pyramid P2..P5. CPU only. The GPU tests
of shpl_build_index_levels take their expectations from the same oracle calls (tests/levels_cases.py)."""
import os

import numpy as np
import pytest

import levels_cases as lc


@pytest.mark.parametrize("name", ["pair", "pyramid"])
def test_oracle_per_level_matches_reference(name):
    g = lc.golden()
    levels = lc.golden_levels(g, name)
    assert levels == [((float(s[0]), float(s[1])), b) for s, b in lc.SETS[name]]
    assert tuple(g["im_size"]) == lc.IM_SIZE
    for f in range(3):
        refs = lc.oracle_levels(g[f"points_{f}"], g[f"voxels_{f}"], g["P"], levels, g["im_size"])
        for lv, ref in enumerate(refs):
            np.testing.assert_array_equal(ref["Mij_pool"], g[f"{name}_mij_{lv}_{f}"].reshape(-1, 2))
            np.testing.assert_array_equal(ref["img_index_flip_pool"], g[f"{name}_flip_{lv}_{f}"].reshape(-1, 3))
            np.testing.assert_array_equal(ref["M_size"], g[f"{name}_msize_{lv}_{f}"])


def test_pair_keeps_different_points_in_every_frame():
    """The fixture can tell the levels apart: the pair's nnz differ in every frame, and every hand-placed edge row
    (z = 699, 700, 703, 704) is present among the voxels."""
    g = lc.golden()
    for f in range(3):
        assert g[f"pair_msize_0_{f}"][1] != g[f"pair_msize_1_{f}"][1]
        assert g[f"pair_msize_0_{f}"][0] == 700 * 800 and g[f"pair_msize_1_{f}"][0] == 88 * 100
        assert set((699, 700, 703, 704)) <= set(g[f"voxels_{f}"][:, 1].tolist())
        # a stride-1 row at or past 700 rows is never kept; the padded stride-8 grid keeps z up to 703
        assert g[f"pair_mij_0_{f}"].reshape(-1, 2)[:, 0].max() < 700 * 800
        assert g[f"pair_mij_1_{f}"].reshape(-1, 2)[:, 0].max() >= (703 // 8) * 100


def test_fixture_is_small_and_data_only():
    assert os.path.getsize(lc.GOLDEN) < 100 * 1024
    g = np.load(lc.GOLDEN, allow_pickle=False)  # plain arrays: no pickled objects
    assert all(g[k].dtype.kind in "fiu" for k in g.files)
    assert not os.path.basename(lc.GOLDEN).startswith("index_")  # those are read as single-frame goldens
