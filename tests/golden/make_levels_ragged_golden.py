"""Generate ``levels_ragged.npz`` by RUNNING the reference's own numpy index builders once per frame AND level,
every frame with its OWN image shape (make_golden.py's rules: the reference checkout is needed here and nowhere
else; the fixture is data only).

Reference functions executed (file:line, relative to the reference checkout):

* ``gen_sparse_pooling_input_avod``   avod/avod/utils/sparse_pool_utils.py:6-20
* ``produce_sparse_pooling_input``    avod/avod/utils/sparse_pool_utils.py:22-58

The dataset hands every sample's own ``image_shape`` to gen (avod/avod/datasets/kitti/kitti_dataset.py:376-377) and
builds one entry per fusion level over the same points, voxel indices and calibration (kitti_dataset.py:381-389).
The fixture holds three frames of 300 points drawn inside the padded image (1242, 376) plus 7 outside it, at the
sizes 1224x370, 1238x374 and 620x188, each with a few hand-placed voxels whose z lies at the edges of the two
BEV grids (699, 700, 703, 704) on points that survive the frame's OWN clip, and the reference's outputs per frame
for two sets of levels:

    pair     [((1, 1), (700, 800)), ((8, 8), (704, 800))]                       the AVOD pair
    pyramid  [((4, 4), (704, 800)), ((8, 8), ...), ((16, 16), ...), ((32, 32), ...)]   P2..P5

    padded [2] (W, H), sizes [3,2] (W_f, H_f), P [3,4], points_<f> [307,3], voxels_<f> [307,2],
    <set>_strides [L,2], <set>_bv_sizes [L,2],
    <set>_mij_<l>_<f> / <set>_flip_<l>_<f> / <set>_msize_<l>_<f>   (Mij_pool, img_index_flip_pool, M_size)

``gen`` is called afresh for every (frame, level): ``produce`` mutates its input. The generator asserts that the
pair's nnz differ in every frame and that at least two frames differ from the run at the padded size. The name
does not match ``index_*.npz``: those are also read as single-frame goldens.

Run:  python tests/golden/make_levels_ragged_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import _install_stubs, _ref_avod  # noqa: E402

from sparse_pooling_amd import synth  # noqa: E402

PADDED = (1242, 376)
SIZES = [(1224, 370), (1238, 374), (620, 188)]
SETS = {"pair": [((1, 1), (700, 800)), ((8, 8), (704, 800))],
        "pyramid": [((s, s), (704, 800)) for s in (4, 8, 16, 32)]}
N_POINTS, N_OUTSIDE, SEED = 300, 7, 2600
EDGE_Z = (699, 700, 703, 704)  # the last row of the stride-1 grid, the first past it; likewise of the padded grid


def frames():
    """The fixture's frames (the tests regenerate nothing: they read the arrays from the fixture)."""
    spec = synth.FrameSpec(N_POINTS, PADDED, (704, 800), (1, 1))
    out = []
    for f, size in enumerate(SIZES):
        fr = synth.make_frame(spec, SEED + f, n_outside=N_OUTSIDE)
        inside = np.flatnonzero(synth._clip_mask(fr.points, fr.P, size))  # survivors of the frame's own clip
        assert inside.size >= 4 * len(EDGE_Z)
        for k, z in enumerate(EDGE_Z):  # hand-placed (spread over the frame)
            fr.voxel_indices[inside[(37 * f + 71 * k) % inside.size]] = (13 + 100 * k + f, z)
        out.append(fr)
    return out


def main():
    _install_stubs()
    spu = _ref_avod()

    def run(fr, size, stride, bv_size):
        g = spu.gen_sparse_pooling_input_avod(fr.points.copy(), fr.voxel_indices.copy(), synth.StereoCalib(fr.P),
                                              [float(size[0]), float(size[1])], bv_size)
        return spu.produce_sparse_pooling_input(g, stride=list(stride))

    rec = dict(padded=np.array(PADDED, np.float64), sizes=np.array(SIZES, np.float64), P=synth.KITTI_P2)
    for name, levels in SETS.items():
        rec[f"{name}_strides"] = np.array([s for s, _ in levels], np.float64)
        rec[f"{name}_bv_sizes"] = np.array([b for _, b in levels], np.int64)
    differs = 0
    for f, (fr, size) in enumerate(zip(frames(), SIZES)):
        rec[f"points_{f}"], rec[f"voxels_{f}"] = fr.points, fr.voxel_indices
        frame_differs = False
        for name, levels in SETS.items():
            nnz = []
            for lv, (stride, bv_size) in enumerate(levels):
                out = run(fr, size, stride, bv_size)
                rec[f"{name}_mij_{lv}_{f}"] = np.asarray(out["Mij_pool"], np.int64)
                rec[f"{name}_flip_{lv}_{f}"] = np.asarray(out["img_index_flip_pool"], np.int64)
                rec[f"{name}_msize_{lv}_{f}"] = np.asarray(out["M_size"], np.int64)
                nnz.append(rec[f"{name}_mij_{lv}_{f}"].shape[0])
                pad = run(fr, PADDED, stride, bv_size)
                frame_differs |= (np.asarray(pad["Mij_pool"]).shape != rec[f"{name}_mij_{lv}_{f}"].shape or
                                  not np.array_equal(pad["img_index_flip_pool"], rec[f"{name}_flip_{lv}_{f}"]))
            print(f"frame {f} {size} {name}: nnz={nnz}")
            if name == "pair":
                assert nnz[0] != nnz[1], "the pair's kept sets must differ in every frame"
        differs += frame_differs
    assert differs >= 2, "at least two frames must differ from the run at the padded size"
    path = os.path.join(HERE, "levels_ragged.npz")
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
