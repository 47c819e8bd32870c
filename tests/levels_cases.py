"""Several fusion levels over one batch of frames, for the tests of shpl_build_index_levels: the two sets of
levels, the reference fixture, and what the reference computes per frame and level -- the oracle called with that
level's (stride, bv_size) on a fresh gen (oracle/shpl_oracle.py restates the reference's numpy builders;
tests/test_oracle_levels_golden.py pins these calls to a reference run)."""
import os

import numpy as np

import ragged_cases as rc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "levels_avod.npz")
IM_SIZE = (1242, 375)
# the AVOD pair: the full-resolution SHPL at stride 1, the after-VGG SHPL at stride 8 over the BEV input padded by 4
PAIR = [((1, 1), (700, 800)), ((8, 8), (704, 800))]
# RetinaNet's P2..P5 (stride 2**k)
PYRAMID = [((s, s), (704, 800)) for s in (4, 8, 16, 32)]
SETS = {"pair": PAIR, "pyramid": PYRAMID}


def golden():
    return np.load(GOLDEN, allow_pickle=False)


def golden_levels(g, name):
    return [((float(s[0]), float(s[1])), (int(b[0]), int(b[1])))
            for s, b in zip(g[f"{name}_strides"], g[f"{name}_bv_sizes"])]


def oracle_levels(points, voxels, P, levels, im_size=IM_SIZE):
    """Per level the oracle's gen + produce of one frame (gen afresh per level: produce strides it in place)."""
    return [rc.oracle_index(points, voxels, P, im_size, bv_size, stride) for stride, bv_size in levels]
