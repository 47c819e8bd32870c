"""Generate ``index_ragged.npz`` by RUNNING the reference's own numpy index builders once per frame, each
frame with its OWN image size (make_golden.py's rules: the reference checkout is needed here and nowhere
else; the fixture is data only).

Reference functions executed (file:line, relative to the reference checkout):

* ``gen_sparse_pooling_input_avod``   avod/avod/utils/sparse_pool_utils.py:6-20
* ``produce_sparse_pooling_input``    avod/avod/utils/sparse_pool_utils.py:22-58

KittiDataset.load_samples reads every sample's image_shape from its PNG and hands it to
gen_sparse_pooling_input_avod (avod/avod/datasets/kitti/kitti_dataset.py:376-377); KITTI's left colour images
come in four sizes. The fixture holds a batch of five frames -- those four sizes and one half-size frame -- of
300 points inside the PADDED image (1242, 376) plus 7 outside it, so that every frame's own clip drops points
the padded clip keeps, and the reference's outputs per frame for strides (4, 4) and (8, 8):

    sizes [5,2] (W, H), padded [2], bv_size [2], P [3,4], strides [2,2],
    points_<f> [307,3], voxels_<f> [307,2],
    mij_<s>_<f> / flip_<s>_<f> / msize_<s>_<f>   (s = 4, 8: Mij_pool, img_index_flip_pool, M_size)

``gen`` is called afresh for every (frame, stride): ``produce`` mutates its input.

Every ``index_*.npz`` here is also read as a single-frame golden (make_golden.py's ``_index_case`` keys) by the
tests over that pattern, so the file carries those keys too: frame 1 (1224 x 370) at stride (4, 4).

Run:  python tests/golden/make_ragged_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import _install_stubs, _ref_avod  # noqa: E402

from sparse_pooling_amd import synth  # noqa: E402

SIZES = [(1242, 375), (1224, 370), (1238, 374), (1241, 376), (620, 188)]  # (W, H): KITTI's four + a half-size frame
PADDED = (1242, 376)
BV_SIZE = (704, 800)
STRIDES = [(4, 4), (8, 8)]
N_POINTS, N_OUTSIDE, SEED = 300, 7, 1055
SINGLE = (1, 4)  # (frame, stride) also stored in the single-frame layout of make_golden.py's index_<case>.npz


def frames():
    """The batch's frames (the tests regenerate nothing: they read the arrays from the fixture)."""
    spec = synth.FrameSpec(N_POINTS, PADDED, BV_SIZE, (1, 1))
    return [synth.make_frame(spec, SEED + f, n_outside=N_OUTSIDE) for f in range(len(SIZES))]


def main():
    _install_stubs()
    spu = _ref_avod()
    rec = dict(sizes=np.array(SIZES, np.float64), padded=np.array(PADDED, np.float64), bv_size=np.array(BV_SIZE),
               P=synth.KITTI_P2, strides=np.array(STRIDES, np.float64))
    for f, (fr, size) in enumerate(zip(frames(), SIZES)):
        rec[f"points_{f}"], rec[f"voxels_{f}"] = fr.points, fr.voxel_indices
        for stride in STRIDES:
            g = spu.gen_sparse_pooling_input_avod(fr.points.copy(), fr.voxel_indices.copy(),
                                                  synth.StereoCalib(fr.P), list(size), BV_SIZE)
            gen = {k: np.array(v, copy=True) for k, v in g.items()}
            out = spu.produce_sparse_pooling_input(g, stride=list(stride))
            s = int(stride[0])
            if (f, s) == SINGLE:  # the file is also a single-frame index golden (every index_*.npz is read as one)
                rec.update(points=fr.points, voxel_indices=fr.voxel_indices, im_size=np.array(size),
                           stride=np.array(stride, dtype=np.float64), gen_bv_index=gen["bv_index"],
                           gen_img_index=gen["img_index"], gen_bv_size=gen["bv_size"], gen_img_size=gen["img_size"],
                           mutated_img_index=np.asarray(g["img_index"]), Mij_pool=np.asarray(out["Mij_pool"]),
                           M_val=np.asarray(out["M_val"]), M_size=np.asarray(out["M_size"]),
                           img_index_flip_pool=np.asarray(out["img_index_flip_pool"]),
                           bev_index_flip_pool=np.asarray(out["bev_index_flip_pool"]))
            rec[f"mij_{s}_{f}"] = np.asarray(out["Mij_pool"], np.int64)
            rec[f"flip_{s}_{f}"] = np.asarray(out["img_index_flip_pool"], np.int64)
            rec[f"msize_{s}_{f}"] = np.asarray(out["M_size"], np.int64)
            print(f"frame {f} size {size} stride {stride}: nnz={rec[f'mij_{s}_{f}'].shape[0]}")
    path = os.path.join(HERE, "index_ragged.npz")
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
