"""Batches of mixed image sizes for the ragged index builder's tests: the frames, and what the reference computes
for them -- the oracle called PER FRAME with the frame's OWN image size (oracle/shpl_oracle.py restates the
reference's numpy builders; tests/test_oracle_ragged_golden.py pins these calls to a reference run).

The frames share one padded image feature map [B, Hp, Wp, C]. What the layer computes on it (the window rule):
  bv_fused[f]                = the oracle's layer over img[f, :hq_f, :wq_f]
  img_fused[f, :hq_f, :wq_f] = the oracle's img_fused (dual)
  outside that window          the pass-through half is the input's padding copied, the pooled half zero
and the gradients likewise (outside the window d_img is g_img's pass-through columns alone).
"""
import os

import numpy as np

from oracle import shpl_oracle as orc
from sparse_pooling_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "index_ragged.npz")
KITTI_SIZES = [(1242, 375), (1224, 370), (1238, 374), (1241, 376)]  # (W, H) of KITTI's left colour images
HALF = (620, 188)
PADDED = (1242, 376)  # (max W, max H)
BV_SIZE = (704, 800)


def golden():
    return np.load(GOLDEN, allow_pickle=False)


def oracle_index(points, voxels, P, size, bv_size, stride):
    """gen_sparse_pooling_input_avod + produce_sparse_pooling_input of one frame at image size `size` (W, H): gen
    afresh on every call, because produce strides its img_index in place."""
    gen = orc.gen_sparse_pooling_input_avod(points, voxels, P, [float(size[0]), float(size[1])], tuple(bv_size))
    return orc.produce_sparse_pooling_input(gen, stride=tuple(stride))


def make_frames(counts, stride, seed, padded=PADDED):
    """Frames of counts[f] points inside the PADDED image and 7 that every clip drops, as the issue draws them."""
    return [synth.make_frame(synth.FrameSpec(int(n), padded, BV_SIZE, tuple(stride)), seed + f, n_outside=7)
            for f, n in enumerate(counts)]


def strided(size, s):
    """(hq, wq) = floor((H, W) / s) of an image size (W, H): make_geometry's IEEE division."""
    return int(np.floor(size[1] / float(s))), int(np.floor(size[0] / float(s)))


def frame_refs(frames, sizes, stride, points_dtype=np.float64):
    """Per frame, the oracle's outputs at the frame's own size (the points as the device reads them)."""
    return [oracle_index(fr.points.astype(points_dtype).astype(np.float64), fr.voxel_indices, fr.P, size, BV_SIZE,
                         stride) for fr, size in zip(frames, sizes)]


def pix_ids(flip, f, hp, wp):
    """f * Hp * Wp + v' * Wp + u' of img_index_flip_pool rows, -1 where (v', u') lies outside the padded map."""
    v, u = flip[:, 1], flip[:, 2]
    ok = (v >= 0) & (u >= 0) & (v < hp) & (u < wp)
    return np.where(ok, f * hp * wp + v * wp + u, -1)


def padded_features(B, hp, wp, c, sizes, s, seed):
    """[B, Hp, Wp, c] f32 features; outside every frame's own window a non-zero pattern no kernel may pool."""
    x = synth.make_features((B, hp, wp, c), seed)
    for f, size in enumerate(sizes):
        hq, wq = strided(size, s)
        pad = np.ones((hp, wp), bool)
        pad[:hq, :wq] = False
        x[f][pad] = 1000.0 + f + np.arange(c, dtype=np.float32)
    return x


def layer_oracle(refs, sizes, s, bev, img, g_bv=None, g_img=None):
    """Per frame (bv_fused, img_fused, d_bev, d_img) on the padded maps under the window rule (module docstring);
    the gradients None without g_bv / g_img. bev [B,Hb,Wb,Cb], img [B,Hp,Wp,Ci] f32."""
    B, hp, wp, Ci = img.shape
    Hb, Wb, Cb = bev.shape[1:]
    out = []
    for f, (ref, size) in enumerate(zip(refs, sizes)):
        hq, wq = strided(size, s)
        assert hq <= hp and wq <= wp
        mij, mval, msize, idx = ref["Mij_pool"], ref["M_val"], ref["M_size"], ref["img_index_flip_pool"]
        win = np.ascontiguousarray(img[f:f + 1, :hq, :wq])
        eb, ei_win = orc.sparse_pool_layer(bev[f:f + 1], win, mij, mval, msize, idx, dual=True)
        ei = np.zeros((1, hp, wp, Ci + Cb), np.float32)
        ei[..., :Ci] = img[f]
        ei[:, :hq, :wq] = ei_win
        d_bev = d_img = None
        if g_bv is not None:
            d_img = g_img[f:f + 1, ..., :Ci].copy()
            d_img[:, :hq, :wq] += orc.sparse_pool_grad_img(mij, mval, msize, g_bv[f, ..., Cb:].reshape(-1, Ci), idx,
                                                           (1, hq, wq, Ci))
            d_bev = g_bv[f:f + 1, ..., :Cb] + orc.sparse_pool_trans_grad_bev(
                mij, mval, msize, np.ascontiguousarray(g_img[f:f + 1, :hq, :wq, Ci:]), idx).reshape(1, Hb, Wb, Cb)
        out.append((eb, ei, d_bev, d_img))
    return out
