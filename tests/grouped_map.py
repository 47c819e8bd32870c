"""A seeded, hand-made single-frame correspondence matrix in the reference format
(Mij [nnz, 2] of (BEV row, column k), M_val, M_size, img_index_flip [ncols, 3]) whose
BEV->image pooling depends on TF's summation order: _sparse_pool_trans_op sums each
column of M first (Q[k] = sum of column k's entries, the SparseTensorDenseMatMul of the
transposed M) and then adds the columns' partials per pixel (ScatterNd). A helper for
tests/test_grouped_map_oracle.py and tests/test_gpu_conv_img.py; it needs no GPU.

Geometry: image 9 x 40 (two occupancy words per row, the second partial; two 32-pixel
strips, the second 8 wide), BEV 11 x 13. About 60 columns holding 0, 1, 2 or 3 entries
each (about 150 entries), duplicate (row, column) pairs, several columns per pixel,
pixels occupied at x in {0, 31, 32, 39} and y in {0, 8}, values in [0.25, 2).

Planted on three pixels (x = 0, 32, 39) is a cancellation triple of columns
k1 < k2 < k3 that no other column shares a pixel with:

    k1: one entry   4096 * bev = 4096 * 4096 s    = 2^24 s
    k2: two entries    1 * bev =    1 *    1 s    (twice)
    k3: one entry   4096 * bev = 4096 * -4096 s   = -2^24 s

(s: a power of two per channel). Per column first: 0 + 2^24 s + (s + s) - 2^24 s = 2 s.
One product after the other in (column, row) order: ((2^24 s + s) + s) - 2^24 s = 0, since
2^24 + 1 rounds back to 2^24 in f32. Every operand is exact in bf16, and so is 2 s.
"""
import numpy as np

IMG_HW = (9, 40)
BEV_HW = (11, 13)
N_COLS = 60
# (y, x) of the planted pixels, and the columns k1 < k2 < k3 of each (random columns lie between them)
PLANTED = [(0, 0), (8, 32), (4, 39)]
PLANT_COLS = [(3, 17, 40), (8, 9, 55), (21, 30, 31)]
# BEV rows kept for the plants: (the 4096 s row, the two s rows, the -4096 s row); the first plant's k2 holds a
# duplicate (row, column) pair
PLANT_ROWS = [(5, (6, 6), 7), (70, (71, 72), 73), (140, (141, 142), 139)]
# pixels the other columns are drawn from: the strip and word edges, first and last row, and a few shared ones
FORCED = [(0, 31), (0, 32), (0, 39), (8, 0), (8, 31), (8, 39), (3, 31), (3, 32)]


def channel_scale(c):
    """The planted rows' power of two per channel: 1/4, 1/2, 1, 2, repeating."""
    return np.ldexp(1.0, (np.arange(c) % 4) - 2).astype(np.float32)


def _bf16_round(a):
    """f32 -> the nearest bf16-representable f32 (round to nearest even)."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)


def make(seed=0):
    """{mij, mval, m_size, idx, img_shape (1, H, W), bev_hw, planted}: the map."""
    rng = np.random.default_rng(seed)
    H, W = IMG_HW
    R = BEV_HW[0] * BEV_HW[1]
    plant_cols = {k for ks in PLANT_COLS for k in ks}
    reserved = {r for a, (b1, b2), c in PLANT_ROWS for r in (a, b1, b2, c)}
    free_rows = np.array([r for r in range(R) if r not in reserved])
    pool = list(FORCED) + [(int(y), int(x)) for y, x in zip(rng.integers(0, H, 14), rng.integers(0, W, 14))]
    pool = [p for p in pool if p not in PLANTED]
    pix = np.zeros((N_COLS, 2), np.int64)
    other = [k for k in range(N_COLS) if k not in plant_cols]
    for n, k in enumerate(other):  # every pool pixel at least once, then shared ones
        pix[k] = pool[n] if n < len(pool) else pool[int(rng.integers(0, len(pool)))]
    rows, cols, vals = [], [], []
    for k in other:
        n = int(rng.choice(4, p=[0.05, 0.10, 0.15, 0.70]))
        r = rng.choice(free_rows, size=n, replace=False) if n else np.zeros(0, np.int64)
        if n >= 2 and rng.random() < 0.3:
            r[1] = r[0]  # a duplicate (row, column) pair
        rows += [int(v) for v in r]
        cols += [k] * n
        vals += [float(v) for v in rng.uniform(0.25, 2.0, n)]
    for (y, x), (k1, k2, k3), (ra, (rb1, rb2), rc) in zip(PLANTED, PLANT_COLS, PLANT_ROWS):
        pix[[k1, k2, k3]] = (y, x)
        rows += [ra, rb1, rb2, rc]
        cols += [k1, k2, k2, k3]
        vals += [4096.0, 1.0, 1.0, 4096.0]
    order = rng.permutation(len(rows))  # M's entries in no particular order
    mij = np.stack([np.array(rows, np.int64), np.array(cols, np.int64)], 1)[order]
    mval = np.array(vals, np.float32)[order]
    idx = np.concatenate([np.zeros((N_COLS, 1), np.int64), pix], 1)
    return {"mij": np.ascontiguousarray(mij), "mval": mval, "m_size": np.array([R, N_COLS], np.int64), "idx": idx,
            "img_shape": (1, H, W), "bev_hw": BEV_HW, "planted": list(PLANTED)}


def features(c_img, c_bev, seed=1):
    """(img [1, 9, 40, c_img], bev [1, 11, 13, c_bev]) f32, bf16-representable, the planted BEV rows set."""
    rng = np.random.default_rng(seed)
    img = _bf16_round(rng.standard_normal((1,) + IMG_HW + (c_img,)).astype(np.float32))
    bev = _bf16_round(rng.standard_normal((1,) + BEV_HW + (c_bev,)).astype(np.float32))
    flat = bev.reshape(-1, c_bev)
    s = channel_scale(c_bev)
    for ra, (rb1, rb2), rc in PLANT_ROWS:
        flat[ra] = 4096.0 * s
        flat[rb1] = s
        flat[rb2] = s
        flat[rc] = -4096.0 * s
    return img, bev


def plain_sum(m, bev):
    """The BEV->image pooling with one f32 product after the other per pixel in (column, row) order -- what a
    pixel-keyed CSR summed without the per-column partials gives: [1, H, W, C]."""
    _, H, W = m["img_shape"]
    flat = np.ascontiguousarray(bev, np.float32).reshape(-1, bev.shape[-1])
    out = np.zeros((H * W, flat.shape[1]), np.float32)
    order = np.lexsort((m["mij"][:, 0], m["mij"][:, 1]))  # by column, then row; stable
    for e in order:
        r, k = m["mij"][e]
        p = int(m["idx"][k, 1]) * W + int(m["idx"][k, 2])
        out[p] = out[p] + np.float32(m["mval"][e]) * flat[r]
    return out.reshape(1, H, W, -1)
