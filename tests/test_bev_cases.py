"""The BEV edge cases (tests/bev_cases.py) without a GPU: every case reaches the path it was planted for,
checked on its sorted words, and the C oracle equals the reference's goldens (tests/golden/bev_edges.npz,
written by tests/golden/make_golden.py) bitwise on every case the reference ran."""
import os

import numpy as np
import pytest

import bev_cases as bc
from oracle import shpl_oracle as orc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bev_edges.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLD)


def _words(name):
    a = bc.case(name)
    g = bc.geom(a[2], a[3], a[6])
    return a, g, bc.sorted_words(*a)


def _covers(start, length, word):
    """A run holds both word - 1 and word."""
    return bool(((start <= word - 1) & (start + length > word)).any())


@pytest.mark.parametrize("name", list(bc.CASES))
def test_cases_stay_inside_their_grid_and_size(name):
    a, g, w = _words(name)
    assert a[0].shape[1] <= 12000 and a[0].dtype == np.float64
    assert bc.in_grid(w, g)  # the reference does not raise
    assert g.log_tile == {"G0": 0, "G4": 4, "G0s1": 0, "G0s8": 0, "Gneg": 0}[bc.CASES[name][1]]
    if name in bc.GOLDEN:  # the reference voxelizes a slice only if it holds more than one point
        assert (np.bincount(w[:, 0], minlength=a[6] + 1) >= 2).all()


def test_grids():
    g = {n: bc.geom(G.ext, G.vs, G.S) for n, G in bc.GRIDS.items()}
    assert (g["G0"].n_keys, g["G4"].n_keys, g["G0s8"].n_keys) == (9600, 153600, 14400)
    assert (g["Gneg"].min_x, g["Gneg"].min_z) == (-30, -20)
    assert (g["Gover"].nx, g["Gover"].nz) == (6, 48)


@pytest.mark.parametrize("name", ["ties_G0", "ties_Gneg"])
def test_ties_winner_is_not_the_easy_one(name):
    a, g, w = _words(name)
    y = a[0][1]
    if name == "ties_Gneg":
        assert (w[:, 3] < 0).all()  # every discrete y is negative
    w = w[w[:, 0] < a[6]]
    _, start, length = bc.key_runs(w, g)
    multi = [(s, n) for s, n in zip(start, length) if n >= 2]
    assert 55 <= len(multi) <= 65 and min(n for _, n in multi) == 2 and max(n for _, n in multi) == 40
    not_min_y = later = middle = 0
    for s, n in multi:
        run = w[s:s + n]
        win, yd0 = run[0, 4], run[0, 3]
        tie = run[run[:, 3] == yd0, 4]
        assert tie.size >= 2 and np.unique(y[tie]).size == tie.size  # one discrete y, different exact y
        assert win == tie.min()
        if n >= 3:  # neither the first nor the last point of the cell in memory
            assert run[:, 4].min() < win < run[:, 4].max()
            middle += 1
        not_min_y += y[win] > y[run[:, 4]].min()
        later += bool((run[run[:, 3] != yd0, 4] < win).any())
    assert middle >= 50 and not_min_y >= 20 and later >= 10


def test_density_counts():
    (cloud, plane, ext, vs, hlo, hhi, S), cells = bc.density()
    g = bc.geom(ext, vs, S)
    w = bc.sorted_words(cloud, plane, ext, vs, hlo, hhi, S)
    key, _, length = bc.key_runs(w[w[:, 0] == S], g)
    count = dict(zip(key - S * g.n_cells, length))
    assert [count[c] for c in cells] == bc.DENSITY_COUNTS == list(range(1, 18)) + [40, 300]
    # points inside the extents, in those cells, in no slice
    x, y, z = cloud
    inside = (x > ext[0, 0]) & (x < ext[0, 1]) & (y > ext[1, 0]) & (y < ext[1, 1]) & (z > ext[2, 0]) & (z < ext[2, 1])
    assert inside.all()
    cell = (np.floor(x / vs).astype(int) - g.min_x) * g.nz + np.floor(z / vs).astype(int) - g.min_z
    silent = np.setdiff1d(np.arange(cloud.shape[1]), w[:, 4])
    h = plane[3] - y[silent]
    assert (h > hhi).sum() >= 20 and (h < hlo).sum() >= 10 and np.isin(cell[silent], cells).all()


@pytest.mark.parametrize("name", ["grid_lines_G0", "grid_lines_Gneg"])
def test_grid_lines_plants(name):
    (cloud, plane, ext, vs, hlo, hhi, S), g, w = _words(name)
    x, y, z = cloud
    kept = np.zeros(cloud.shape[1], bool)
    kept[w[:, 4]] = True
    for axis, c, first, n in ((0, x, g.min_x, g.nx), (2, z, g.min_z, g.nz)):
        for k in range(first + 1, first + n):  # every grid line inside, in both spellings, kept
            for v in {k * vs, round(k * vs, 9)}:
                assert kept[c == v].any(), (axis, k)
        assert np.floor(0.3 / 0.1) == 2 and np.floor(0.6 / 0.1) == 5  # a true division, as the issue says
    for axis in range(3):
        for side in range(2):
            e = ext[axis, side]
            assert (cloud[axis] == e).sum() >= 2 and not kept[cloud[axis] == e].any()  # strict bounds
            near = cloud[axis] == np.nextafter(e, ext[axis, 1 - side])
            assert near.sum() >= 2
            if axis != 1:
                assert kept[near].all()
    if name == "grid_lines_Gneg":  # the height range reaches past y = -0.1: only the bound drops that face
        assert kept[y == np.nextafter(-0.1, -1)].all()
    _, lo, hi = bc.slice_bounds(hlo, hhi, S)
    seen = 0
    for off in lo + hi:
        y0 = plane[3] - off
        for v in (np.nextafter(y0, -np.inf), y0, np.nextafter(y0, np.inf)):
            assert (y == v).any()
            seen += int(kept[y == v].any())
    assert seen >= 3 * S  # most of them lie inside the y extents and the height range


@pytest.mark.parametrize("name", ["tilted_kitti", "tilted_plane2"])
def test_tilted_is_tilted_and_clear_of_the_slice_planes(name):
    (cloud, plane, ext, vs, hlo, hhi, S), g, w = _words(name)
    assert cloud.shape[1] == 6000 and (plane[[0, 2]] != 0).all()
    _, lo, hi = bc.slice_bounds(hlo, hhi, S)
    t = plane[0] * cloud[0] + plane[1] * cloud[1] + plane[2] * cloud[2] + plane[3]
    assert min(np.abs(t - b).min() for b in lo + hi) > 1e-9
    _, _, length = bc.key_runs(w[w[:, 0] == S], g)
    assert (length >= 10).sum() >= 40  # the clustered cells
    assert np.setdiff1d(np.arange(6000), w[:, 4]).size > 100  # some points outside the height range


def test_window_paths():
    win, blk, stride = bc.TS_WIN, bc.BEV_BLOCK, bc.MAP_STRIDE
    # a: one tile (one key at log_tile 0) larger than the whole window
    a, g, w = _words("window_a")
    _, start, length = bc.key_runs(w, g)
    assert g.log_tile == 0 and length.max() == 11000 and (length > win).sum() == 2  # its slice and the density range
    # b: a run over word 10240
    for name in ("window_b", "window_b_G4"):
        a, g, w = _words(name)
        key, start, length = bc.key_runs(w, g)
        i = np.nonzero((start < win) & (start + length > win))[0]
        assert i.size == 1 and length[i[0]] >= 200
        tile = key >> g.log_tile
        in_tile = tile == tile[i[0]]
        assert (in_tile.sum() >= 2) == (name == "window_b_G4")  # G4: several keys in the straddling tile
    # c, d: n_ent exactly one window / one chunk
    assert _words("window_c")[2].shape[0] == win and np.unique(_words("window_c")[2][:, 4]).size == 5120
    assert _words("window_d")[2].shape[0] == blk
    # e, f: a run that begins on a chunk edge and one that crosses the next
    for name, edge in (("window_e", blk), ("window_f", stride)):
        a, g, w = _words(name)
        _, start, length = bc.key_runs(w, g)
        assert (start == edge).any() and _covers(start, length, 2 * edge)
        assert (w[:2 * edge + 1, 0] == 0).all()  # both in the slice words, which step 5 compacts
    # f holds e's conditions for the 1024-word chunks as well
    _, start, length = bc.key_runs(_words("window_f")[2], _words("window_f")[1])
    assert (start % blk == 0).sum() >= 2 and _covers(start, length, 8 * blk)


def test_sparse_frames():
    count = lambda name: np.bincount(_words(name)[2][:, 0], minlength=6).tolist()  # noqa: E731
    assert bc.case("sparse_empty")[0].shape == (3, 0)
    assert bc.case("sparse_one")[0].shape == (3, 1) and sum(count("sparse_one")) == 2
    for name in ("sparse_outside", "sparse_above"):
        assert bc.case(name)[0].shape == (3, 50) and sum(count(name)) == 0
    cloud, _, ext = bc.case("sparse_above")[:3]
    assert ((cloud > ext[:, :1]) & (cloud < ext[:, 1:])).all()
    cloud, _, ext = bc.case("sparse_outside")[:3]
    assert not ((cloud > ext[:, :1]) & (cloud < ext[:, 1:])).all(axis=0).any()
    c = count("sparse_one_in_slice")
    assert c[2] == 0 and c[4] == 1 and min(c[0], c[1], c[3]) >= 2


def test_slices_cases_cut_the_ties_cloud():
    for name, S in (("slices_s1", 1), ("slices_s8", 8)):
        a, g, w = _words(name)
        np.testing.assert_array_equal(a[0], bc.case("ties_G0")[0])
        assert a[6] == S and w.shape[0] == 2 * a[0].shape[1]
        _, _, length = bc.key_runs(w[w[:, 0] < S], g)
        assert (length >= 2).sum() >= 55


def test_overflow_points_are_inside_the_extents_and_outside_the_grid():
    cloud, plane, ext, vs, hlo, hhi, S = bc.case("overflow")
    g = bc.geom(ext, vs, S)
    w = bc.sorted_words(cloud, plane, ext, vs, hlo, hhi, S)
    assert w.shape[0] == 2 * cloud.shape[1]  # every point inside the extents and the height range
    out = w[(w[:, 1] >= g.nx) | (w[:, 2] >= g.nz)]
    assert sorted(set(out[:, 4])) == list(bc.OVERFLOW_POINTS)
    assert set(out[out[:, 4] == 100, 1]) == {g.nx} and set(out[out[:, 4] == 200, 2]) == {g.nz}
    # voxel sizes whose round extents do this, and some that do not
    assert np.floor(np.nextafter(0.9, 0) / 0.3) == 3.0 and np.ceil(0.9 / 0.3 - 1) == 2
    assert np.floor(np.nextafter(14.4, 0) / 0.3) == 48.0 and np.ceil(14.4 / 0.3 - 1) == 47


# ---- the oracle against the reference -----------------------------------------------------------------

@pytest.mark.parametrize("name", bc.GOLDEN)
def test_oracle_matches_reference_on_edges(golden, name):
    args = bc.case(name)
    for k, v in zip(("point_cloud", "ground_plane", "area_extents", "voxel_size", "height_lo", "height_hi",
                     "num_slices"), args):
        np.testing.assert_array_equal(golden[f"{name}/{k}"], v)  # the fixture is of this case table
    hm, dm, vox, upts = orc.bev_slices(*args)
    np.testing.assert_array_equal(vox, golden[f"{name}/voxel_indices"])
    np.testing.assert_array_equal(upts, golden[f"{name}/pts_in_voxel"])
    np.testing.assert_array_equal(hm, golden[f"{name}/height_maps"])
    np.testing.assert_array_equal(dm, golden[f"{name}/density_map"])
    assert vox.shape[0] > 0 and (dm > 0).any()


def test_overflow_reference_raised_and_oracle_reports(golden):
    args = bc.case("overflow")
    np.testing.assert_array_equal(golden["overflow/point_cloud"], args[0])
    assert str(golden["overflow/raised"]) == "ValueError"
    assert str(golden["overflow/message"]) == "Extents are smaller than max_voxel_coord"
    with pytest.raises(ValueError, match="Extents are smaller than max_voxel_coord"):
        orc.bev_slices(*args)
    # either point alone is reported; without both the oracle runs
    keep = np.ones(args[0].shape[1], bool)
    for p in bc.OVERFLOW_POINTS:
        keep[:] = True
        keep[[q for q in bc.OVERFLOW_POINTS if q != p]] = False
        with pytest.raises(ValueError):
            orc.bev_slices(args[0][:, keep], *args[1:])
    keep[list(bc.OVERFLOW_POINTS)] = False
    hm, dm, vox, _ = orc.bev_slices(args[0][:, keep], *args[1:])
    assert vox.shape[0] > 100 and hm.shape == (2, 48, 6)
