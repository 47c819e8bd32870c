"""The BEV slice voxelizer (shpl_bev_slices, shpl_bev_maps, shpl_bev_input) and the one-workgroup tile sort it
shares with the MV3D producer, on the planted clouds of tests/bev_cases.py: every case alone and in one ragged
batch per grid, against the reference's goldens (tests/golden/bev_edges.npz) where the reference ran and the C
oracle elsewhere. Every comparison is bitwise.

What each case is there for is asserted on the CPU (tests/test_bev_cases.py); here the device runs them.
"""
import os
import types

import numpy as np
import pytest
import torch

import bev_cases as bc
from oracle import shpl_oracle as orc

pytestmark = pytest.mark.gpu

DEV = "cuda"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bev_edges.npz")
EQ = np.testing.assert_array_equal


def _np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def golden():
    from sparse_pooling_amd import _lib as L
    L.lib()
    assert torch.cuda.is_available()
    return np.load(GOLD)


def _run(frames, grid_args, maps=True, counts=None):
    """bev_slices_batch over frames [(cloud (3, n), plane)]; counts: live points of each frame."""
    from sparse_pooling_amd import bev
    off = np.concatenate([[0], np.cumsum([c.shape[1] for c, _ in frames])]).astype(np.int64)
    pts = np.ascontiguousarray(np.concatenate([c.T for c, _ in frames]))
    pl = np.stack([p for _, p in frames])
    b = bev.bev_slices_batch(torch.from_numpy(pts).to(DEV), torch.from_numpy(off).to(DEV),
                             torch.from_numpy(pl).to(DEV), *grid_args, maps=maps,
                             point_counts=None if counts is None else torch.tensor(counts, device=DEV))
    torch.cuda.synchronize()
    return b, off


def _check_frame(b, off, f, want, maps=True):
    hm, dm, vox, upts = want
    n = int(b.frame_nvox[f].item())
    assert n == vox.shape[0]
    EQ(_np(b.voxel_indices[off[f]:off[f] + n]), vox)
    EQ(_np(b.pts_in_voxel[off[f]:off[f] + n]), upts)
    if maps:
        EQ(_np(b.height_maps[f]), hm)
        EQ(_np(b.density_map[f]), dm)


def _occupied(want, plane, grid_args):
    """The occupied (slice, row, column) elements of the height maps: the expected maps' non-zeros and, because
    a height of exactly 0.0 is possible, the expected voxel rows -- a row's slice is the first one whose expected
    map holds the row's point's height (dist_to_plane's sum, left to right) at its cell."""
    ehm, _, vox, upts = want
    occ = ehm != 0
    if occ.sum() != vox.shape[0]:
        _, _, hlo, hhi, S = grid_args
        hpd, lo, _ = bc.slice_bounds(hlo, hhi, S)
        a, b, c, d = plane
        dist = (a * upts[:, 0] + b * upts[:, 1] + c * upts[:, 2] + d) / np.sqrt(a * a + b * b + c * c)
        row, col = vox[:, 1] - 1, vox[:, 0]  # pixel row nz - 1 - z = (nz - z) - 1
        hit = np.stack([ehm[s, row, col] == (dist - lo[s]) / hpd for s in range(S)])
        # a point on the lower plane of the next slice also "hits" that slice's empty cell (0.0 == 0.0), and where
        # hi[s - 1] and lo[s] differ by an ulp one point is the row of one cell in both slices: the rows are
        # slice-major with ascending cells, so a row's slice is the first hit that keeps that order
        cell = col.astype(np.int64) * ehm.shape[1] - row
        cur, prev = 0, -1 << 40
        for r in range(vox.shape[0]):
            s = next(s for s in range(cur, S) if hit[s, r] and (s > cur or cell[r] > prev))
            cur, prev = s, cell[r]
            occ[s, row[r], col[r]] = True
        assert occ.sum() == vox.shape[0]
    return occ


def _check_map_forms(frames, grid_args, wants):
    """The deferred maps (into NaN), the network input and the non-zeroing maps (into a sentinel) of a
    maps=False call, against the expected maps of every frame."""
    b, off = _run(frames, grid_args, maps=False)
    assert b.height_maps is None and b.density_map is None and int(b.err.item()) == 0
    F, (S, nz, nx) = len(frames), wants[0][0].shape
    f64 = dict(dtype=torch.float64, device=DEV)
    hm, dm = b.write_maps(torch.full((F, S, nz, nx), float("nan"), **f64), torch.full((F, nz, nx), float("nan"), **f64))
    bin_ = b.write_bev_input(torch.full((F, nz, nx, S + 1), float("nan"), dtype=torch.float32, device=DEV))
    sent = 7.5
    shm, sdm = b.write_maps(torch.full((F, S, nz, nx), sent, **f64), torch.full((F, nz, nx), sent, **f64), zero=False)
    torch.cuda.synchronize()
    for f, (ehm, edm, vox, _) in enumerate(wants):
        _check_frame(b, off, f, wants[f], maps=False)
        EQ(_np(hm[f]), ehm)
        EQ(_np(dm[f]), edm)
        EQ(_np(bin_[f]).view(np.uint32), np.dstack((*ehm, edm)).astype(np.float32).view(np.uint32))
        occ = _occupied(wants[f], frames[f][1], grid_args)
        EQ(_np(shm[f]), np.where(occ, ehm, sent))
        EQ(_np(sdm[f]), np.where(edm != 0, edm, sent))
        assert (occ.any(axis=0) <= (edm != 0)).all()


def _grid_args(name):
    return bc.case(name)[2:]


ALONE = list(bc.CASES)


@pytest.mark.parametrize("name", ALONE)
def test_case_alone(golden, name):
    cloud, plane = bc.case(name)[:2]
    want = bc.expected(name, golden)
    b, off = _run([(cloud, plane)], _grid_args(name))
    _check_frame(b, off, 0, want)
    assert int(b.err.item()) == 0
    _check_map_forms([(cloud, plane)], _grid_args(name), [want])


# one ragged batch per grid: every case of the grid, the frame without points in the middle, and frames under
# other planes (their expected outputs from the oracle)
BATCHES = {
    "G0": ["ties_G0", "density", "grid_lines_G0", "window_a", "window_b", "sparse_one", "sparse_empty", "window_c",
           "window_d", "window_e", "window_f", "sparse_outside", "sparse_above", "sparse_one_in_slice"],
    "G4": ["tilted_kitti", "sparse_empty", "tilted_plane2", "window_b_G4"],
    "Gneg": ["ties_Gneg", "sparse_empty", "grid_lines_Gneg"],
    "G0s1": ["slices_s1", "sparse_empty", "slices_s1"],
    "G0s8": ["slices_s8", "sparse_empty", "slices_s8"],
}
OTHER_PLANES = {"G0": ("density", bc.KITTI_PLANE), "G4": ("tilted_kitti", bc.PLANE2),
                "Gneg": ("ties_Gneg", np.array([0.004, -1.0, -0.003, 1.66])),
                "G0s1": ("slices_s1", bc.KITTI_PLANE), "G0s8": ("slices_s8", bc.KITTI_PLANE)}


@pytest.mark.parametrize("grid", list(BATCHES))
def test_ragged_batch_per_grid(golden, grid):
    names = BATCHES[grid]
    grid_args = _grid_args(names[0])
    frames = [tuple(bc.case(n)[:2]) for n in names]
    wants = [bc.expected(n, golden) if n != "sparse_empty" else orc.bev_slices(bc.case(n)[0], frames[0][1], *grid_args)
             for n in names]
    name, plane = OTHER_PLANES[grid]  # the same cloud under another plane: the planes are per frame
    if grid in ("G0s1", "G0s8"):
        frames[2] = (frames[2][0], plane)
        wants[2] = orc.bev_slices(frames[2][0], plane, *grid_args)
    else:
        frames.append((bc.case(name)[0], plane))
        wants.append(orc.bev_slices(bc.case(name)[0], plane, *grid_args))
    assert not np.array_equal(wants[-1][0], bc.expected(name, golden)[0])
    b, off = _run(frames, grid_args)
    assert int(b.err.item()) == 0
    for f in range(len(frames)):
        _check_frame(b, off, f, wants[f])
    _check_map_forms(frames, grid_args, wants)


@pytest.mark.parametrize("name", ["ties_G0", "density"])
def test_point_counts_hide_valid_looking_rows(golden, name):
    """The capacity layout shpl_velo_to_cam hands over: behind each frame's live points lie rows that are valid
    points of the same grid (another seed's cloud), which only the counts keep out."""
    live, plane = bc.case(name)[:2]
    grid_args = _grid_args(name)
    other = bc.ties("G0", seed=99)[0]
    assert bc.sorted_words(other, plane, *grid_args).shape[0] == 2 * other.shape[1]  # all of them would count
    n, m = live.shape[1], other.shape[1]
    full = np.concatenate([live, other], axis=1)
    # frame 0: live + padding; 1: count 0 over valid rows; 2: count beyond the capacity (clamped to it); 3: as 0
    frames = [(full, plane), (other, plane), (live, plane), (full[:, ::-1].copy(), plane)]
    counts = [n, 0, n + 1000, m]
    b, off = _run(frames, grid_args, counts=counts)
    assert int(b.err.item()) == 0
    want = bc.expected(name, golden)
    empty = orc.bev_slices(np.zeros((3, 0)), plane, *grid_args)
    rev = orc.bev_slices(full[:, ::-1][:, :m], plane, *grid_args)
    for f, w in enumerate([want, empty, want, rev]):
        _check_frame(b, off, f, w)
    assert int(b.frame_nvox[0].item()) < orc.bev_slices(full, plane, *grid_args)[2].shape[0]  # the rows would add voxels


def test_generate_bev_like_the_reference(golden):
    from sparse_pooling_amd import bev
    cloud, plane, ext, vs, hlo, hhi, S = bc.case("ties_G0")
    hm, dm, vox, upts = bc.expected("ties_G0", golden)
    gen = bev.BevSlices(types.SimpleNamespace(height_lo=hlo, height_hi=hhi, num_slices=S))
    maps, gvox, gpts = gen.generate_bev("lidar", cloud.copy(), plane, ext, vs, output_indices=True)
    assert gvox.dtype == torch.int64 and gpts.dtype == torch.float64
    EQ(_np(gvox), vox)
    EQ(_np(gpts), upts)
    EQ(np.stack([_np(m) for m in maps["height_maps"]]), hm)
    EQ(_np(maps["density_map"]), dm)
    only = gen.generate_bev("lidar", cloud.copy(), plane, ext, vs)
    EQ(_np(only["density_map"]), dm)


# ---- a point inside the extents whose cell lies past the grid --------------------------------------------

def _overflow():
    args = bc.case("overflow")
    keep = np.ones(args[0].shape[1], bool)
    keep[list(bc.OVERFLOW_POINTS)] = False
    return args, np.ascontiguousarray(args[0][:, keep])


def test_overflow_point_forms_no_voxel_and_sets_the_row_bit():
    from sparse_pooling_amd import _lib as L
    from sparse_pooling_amd import bev
    args, rest = _overflow()
    want = orc.bev_slices(rest, *args[1:])
    b, off = _run([(args[0], args[1])], args[2:])
    assert int(b.err.item()) & L.EBIT_ROW
    _check_frame(b, off, 0, want)
    b, off = _run([(rest, args[1])], args[2:])
    assert int(b.err.item()) == 0
    _check_frame(b, off, 0, want)
    gen = bev.BevSlices(types.SimpleNamespace(height_lo=args[4], height_hi=args[5], num_slices=args[6]))
    with pytest.raises(ValueError, match="Extents are smaller than max_voxel_coord"):
        gen.generate_bev("lidar", args[0].copy(), args[1], args[2], args[3], output_indices=True)
    maps, vox, _ = gen.generate_bev("lidar", rest, args[1], args[2], args[3], output_indices=True)
    EQ(_np(vox), want[2])


def test_overflow_frame_leaves_its_neighbours_alone():
    from sparse_pooling_amd import _lib as L
    args, rest = _overflow()
    rng = np.random.default_rng(8)
    G = bc.GRIDS["Gover"]
    g = bc.geom(G.ext, G.vs, G.S)
    a, c = (bc._scatter(G, g, rng, rng.integers(0, g.n_cells, n)) for n in (500, 150))
    frames = [(a, args[1]), (args[0], args[1]), (c, bc.KITTI_PLANE)]
    wants = [orc.bev_slices(a, args[1], *args[2:]), orc.bev_slices(rest, *args[1:]),
             orc.bev_slices(c, bc.KITTI_PLANE, *args[2:])]
    b, off = _run(frames, args[2:])
    assert int(b.err.item()) == L.EBIT_ROW
    for f in range(3):
        _check_frame(b, off, f, wants[f])
    # the slots behind each frame's voxels were not written
    for f in range(3):
        n = int(b.frame_nvox[f].item())
        assert wants[f][2].shape[0] == n < off[f + 1] - off[f]


# ---- the shared sort through the MV3D producer ------------------------------------------------------------

def _mv3d_cloud(which):
    """480 000 keys, 32 per tile. big: 11 000 points in one voxel; straddle: a voxel of 300 points over word
    10240; exact: 10 240 points in range."""
    rng = np.random.default_rng(40 + len(which))

    def uniform(n, side=(-19.9, 19.9)):
        return np.stack([rng.uniform(*side, n), rng.uniform(-0.9, 2.9, n), rng.uniform(0.1, 47.9, n)], axis=1)

    def voxel(n, corner=(0.0, 0.2, 24.0)):  # side index 100, height index 3, forward index 120
        return np.asarray(corner) + rng.uniform(0.02, 0.18, (n, 3))

    if which == "big":
        pts = np.concatenate([voxel(11000), uniform(800)])
    elif which == "straddle":
        pts = np.concatenate([uniform(10100, (-19.9, -0.1)), voxel(300), uniform(1000, (0.3, 19.9))])
    else:
        out = uniform(400)
        out[:, 1] += 5.0
        pts = np.concatenate([uniform(10240), out])
    pts = pts[rng.permutation(len(pts))]
    pts = np.concatenate([pts, rng.uniform(0, 1, (len(pts), 1))], axis=1)
    img2 = np.stack([rng.integers(0, 1242, len(pts)), rng.integers(0, 375, len(pts))])
    return pts, img2


@pytest.mark.parametrize("which", ["big", "straddle", "exact"])
def test_mv3d_producer_sort_windows(which):
    from sparse_pooling_amd import mv3d
    pts, img2 = _mv3d_cloud(which)
    e_img, e_bv, e_mv, nb = orc.mv3d_voxels(pts, img2, **orc.MV3D_PED)
    if which == "big":
        assert nb.max() == 45 and (e_mv == 1 / 45).sum() == 45 and e_bv.shape[0] < 1000
    elif which == "straddle":
        assert e_bv.shape[0] > 11000
        voxel = (e_bv == [120, 100]).all(axis=1)
        assert voxel.sum() == 45  # the 300-point voxel, capped; 10 100 words sort before it
        assert (pts[:, 0] < -0.05).sum() == 10100
    else:
        assert nb.sum() == e_bv.shape[0] and (pts[:, 1] < 2.99).sum() == 10240
    img, bv, mv = mv3d.mv3d_sparse_pooling_input(pts, img_index2=img2)
    EQ(_np(img), e_img)
    EQ(_np(bv), e_bv)
    EQ(_np(mv), e_mv)
