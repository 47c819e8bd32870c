"""Several fusion levels over a batch of mixed image sizes, for the tests of shpl_build_index_levels_ragged: the
reference fixture, each level's padded image feature map, and what the reference computes per frame and level --
the oracle called with the frame's OWN image size and that level's (stride, bv_size) on a fresh gen
(tests/test_oracle_levels_ragged_golden.py pins these calls to a reference run)."""
import os

import numpy as np

import levels_cases as lc
import ragged_cases as rc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "levels_ragged.npz")
GOLDEN_SIZES = [(1224, 370), (1238, 374), (620, 188)]
SETS = lc.SETS


def golden():
    return np.load(GOLDEN, allow_pickle=False)


def level_maps(levels, padded=rc.PADDED):
    """Each level's padded image feature map (rows, cols): the padded size's strided size at that level."""
    return [rc.strided(padded, stride[0]) for stride, _ in levels]


def oracle_levels(points, voxels, P, levels, size):
    """Per level the oracle's gen + produce of one frame at its own image size (W, H)."""
    return lc.oracle_levels(points, voxels, P, levels, im_size=size)


def differs(a, b):
    """Two oracle results of one frame and level are not the same M."""
    return (a["Mij_pool"].shape != b["Mij_pool"].shape or
            not np.array_equal(a["img_index_flip_pool"], b["img_index_flip_pool"]) or
            not np.array_equal(a["Mij_pool"], b["Mij_pool"]))


def clamped_by_own_size(points, voxels, P, size, level):
    """How many entries of one frame at one level the frame's OWN strided size clamps: the unclamped strided index
    floor(rounded / s) lies at or past floor(own size / s). The rounded index comes from the oracle at image stride 1 with the level's BEV stride and size -- the same
    kept set in the same order, and stride 1 never clamps (the clip keeps u < W - 1)."""
    (s_img, s_bv), bv_size = level
    one = rc.oracle_index(points, voxels, P, size, bv_size, (1, s_bv))
    ref = rc.oracle_index(points, voxels, P, size, bv_size, (s_img, s_bv))
    assert one["Mij_pool"].shape == ref["Mij_pool"].shape
    hq, wq = rc.strided(size, s_img)
    v = np.floor(one["img_index_flip_pool"][:, 1] / float(s_img)).astype(np.int64)
    u = np.floor(one["img_index_flip_pool"][:, 2] / float(s_img)).astype(np.int64)
    hit = (v >= hq) | (u >= wq)
    # what the clamp does to them: the frame's own last row / column
    flip = ref["img_index_flip_pool"]
    assert (flip[v >= hq, 1] == hq - 1).all() and (flip[u >= wq, 2] == wq - 1).all()
    return int(hit.sum())


# ------------------------------------------------------------------ the GPU tests' base batch

BASE_COUNTS = [2100, 1023, 300, 0, 300]  # + 7 outside each: 2107 / 1030 / 307 / 7 / 307 points
BASE_SIZES = [(1224, 370), (1238, 374), (620, 188), (1241, 376), (1242, 375)]
# the oracle's nnz at the AVOD pair per frame: at the frame's own size, and at the padded size (f64 points)
BASE_PAIR_NNZ = [(2081, 2092), (1013, 1019), (106, 107), (0, 0), (300, 300)]
BASE_PAIR_NNZ_PADDED = [(2087, 2098), (1013, 1019), (296, 300), (0, 0), (300, 300)]


def base_frames():
    """Five frames across the 1024-point chunk edge (2107 and 1030 points), one of them empty of points inside
    any image."""
    return rc.make_frames(BASE_COUNTS, (1, 1), 3000)


def base_refs(name, points_dtype=np.float64, sizes=None):
    """refs[f][l]: the oracle for frame f of the base batch at level l of the set, at the frame's own size (or
    `sizes`), the points as the device reads them."""
    sizes = BASE_SIZES if sizes is None else sizes
    return [oracle_levels(fr.points.astype(points_dtype).astype(np.float64), fr.voxel_indices, fr.P, SETS[name], size)
            for fr, size in zip(base_frames(), sizes)]


def base_preconditions(name, points_dtype=np.float64):
    """What makes the base batch a test of per-frame sizes AND per-level compaction, from the oracle alone: at
    every level at least two frames differ from the padded-size result; the pair's nnz differ in at least three
    frames; at every level of stride >= 8 at least one entry is clamped by its frame's own strided size. Returns
    (refs, the clamped counts per level and frame)."""
    frames, levels = base_frames(), SETS[name]
    refs = base_refs(name, points_dtype)
    pads = base_refs(name, points_dtype, [rc.PADDED] * len(frames))
    for l in range(len(levels)):
        assert sum(differs(refs[f][l], pads[f][l]) for f in range(len(frames))) >= 2, (name, l)
    if name == "pair":
        assert sum(refs[f][0]["M_size"][1] != refs[f][1]["M_size"][1] for f in range(len(frames))) >= 3
        if points_dtype == np.float64:
            assert [tuple(int(r["M_size"][1]) for r in refs[f]) for f in range(5)] == BASE_PAIR_NNZ
            assert [tuple(int(r["M_size"][1]) for r in pads[f]) for f in range(5)] == BASE_PAIR_NNZ_PADDED
    clamped = [[clamped_by_own_size(fr.points.astype(points_dtype).astype(np.float64), fr.voxel_indices, fr.P, size,
                                    level) for fr, size in zip(frames, BASE_SIZES)] for level in levels]
    for l, (stride, _) in enumerate(levels):
        if stride[0] >= 8:
            assert sum(clamped[l]) >= 1, (name, l, clamped[l])
    return refs, clamped
