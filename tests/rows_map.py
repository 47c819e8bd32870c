"""A seeded, hand-made two-frame correspondence in the reference format (Mij [nnz, 2] of (row, column),
M_val, M_size, img_index_flip [ncols, 3]) for the row-streaming conv kernels (k_conv_rows, k_wgrad_rows and
their prep kernels k_occ_frame / k_pool_runs of shpl_conv_rows.hip). A helper of tests/test_gpu_conv_rows.py
and tests/test_conv_rows_cases.py; it needs no GPU, and the properties the kernels' paths hang on are asserted
here, where the map is made.

The row kernels cut an h x w map into bands of ceil(h / ceil(h / 60)) rows and strips of 32 columns
(row_geom below, as shpl_conv.hip's), with ceil(w / 32) occupancy words per row. The default target map is
2 x 61 x 70: bands of 31 and 30 rows, three strips (the last 6 wide), three words per row. The source map is
2 x 6 x 7. In both frames

  * cells at x = 0, 31, 32, 63, 64, 69 (both ends of every word and strip) and y = 0, 30, 31, 60 (both ends of
    both bands) are occupied;
  * row 5 has no entry: the pooled chunk is skipped in every strip;
  * row 7 has entries only outside strip 1's 34-cell window (cells 31 .. 64): skipped there, not in strips 0, 2;
  * row 9 has all 70 cells occupied;
  * cells hold 1 .. 6 entries (each count occurs); cell (12, 40) of frame 0 holds 20 (a run past 16).

Frame 1's occupancy differs from frame 0's, and its entry slots start past 0. Variants: "cell" (M's rows are
the target cells, one column per entry on a source pixel: the cell-keyed use, a plain sum per cell); "pixel"
(swapped: M's rows are the source cells and a target pixel's n entries lie in 1 .. n columns on that pixel:
the pixel-keyed use with ent_col, per-column partials); "empty0" (cell-keyed, frame 0 without entries: frame
1's slots start at 0 and its run ranks count from the frame's own first word). Other shapes (make(shape=...))
get the same construction without the default shape's special rows.
"""
import functools

import numpy as np

FRAMES, MAP_HW, SRC_HW = 2, (61, 70), (6, 7)
TW, HALO = 32, 34  # strip width, halo row window (cells x0 - 1 .. x0 + 32)
EDGE_X, EDGE_Y = (0, 31, 32, 63, 64, 69), (0, 30, 31, 60)
EMPTY_ROW, OUTSIDE_ROW, FULL_ROW = 5, 7, 9
LONG_CELL, LONG_RUN = (12, 40), 20
DENSITY = 0.3


def row_geom(h, w):
    """(strips, words per row, bands, rows per band) as shpl_conv.hip's row_geom cuts an h x w map."""
    n_bands = (h + 59) // 60
    return (w + TW - 1) // TW, (w + 31) // 32, n_bands, (h + n_bands - 1) // n_bands


def _counts(rng, variant, shape):
    F, H, W = shape
    c = np.where(rng.random(shape) < DENSITY, rng.integers(1, 7, shape), 0)
    if shape == (FRAMES,) + MAP_HW:
        strips, wpr, n_bands, band = row_geom(H, W)
        assert (strips, wpr, n_bands, band) == (3, 3, 2, 31) and W % TW == 6
        for y in EDGE_Y:
            for x in EDGE_X:
                c[:, y, x] = np.maximum(c[:, y, x], 1)
        c[:, EMPTY_ROW] = 0
        c[:, OUTSIDE_ROW, TW - 1:2 * TW + 1] = 0  # strip 1's window: cells 31 .. 64
        c[:, OUTSIDE_ROW, 3], c[:, OUTSIDE_ROW, 66] = 2, 1
        c[:, FULL_ROW] = np.maximum(c[:, FULL_ROW], 1)
        c[0][LONG_CELL] = LONG_RUN
        # the properties the kernels' paths hang on
        occ = c > 0
        assert occ[:, EDGE_Y][:, :, EDGE_X].all()
        assert not occ[:, EMPTY_ROW].any()
        for s in range(strips):  # the 34-cell window of strip s in the row of entries outside strip 1
            lo, hi = max(s * TW - 1, 0), min(s * TW + TW + 1, W)
            inside = occ[:, OUTSIDE_ROW, lo:hi]
            assert hi - lo <= HALO and (not inside.any() if s == 1 else inside.any(1).all())
        assert occ[:, FULL_ROW].all() and occ[:, FULL_ROW].shape[1] == 70
        assert set(range(1, 7)) <= set(np.unique(c).tolist()) and c.max() == LONG_RUN > 16
        assert (occ[0] != occ[1]).any()
    if variant == "empty0":
        c[0] = 0
    return c


@functools.lru_cache(maxsize=None)
def make(variant="cell", shape=(FRAMES,) + MAP_HW, seed=11):
    """{mij, mval, m_size, idx, img_shape, counts [F, H, W], n_frame (entries per frame)}: the map. Entries are
    grouped by frame and shuffled inside; values in [-2, 2)."""
    assert variant in ("cell", "pixel", "empty0")
    rng = np.random.default_rng(seed)
    F, H, W = shape
    hs, ws = SRC_HW
    swapped = variant == "pixel"
    counts = _counts(rng, variant, shape)
    n_src = hs * ws
    rows, cols, col_pix, n_frame, several = [], [], [], [], 0
    for f in range(F):
        r_f, c_f = [], []
        for t in np.flatnonzero(counts[f].reshape(-1)):
            n = int(counts[f].reshape(-1)[t])
            src = rng.choice(n_src, n, replace=False) + f * n_src
            m = int(rng.integers(1, n + 1)) if swapped else n  # columns of this target
            several += swapped and 1 < m < n
            c_f += [len(col_pix) + i % m for i in range(n)]
            r_f += [int(s) for s in src] if swapped else [f * H * W + int(t)] * n
            col_pix += [f * H * W + int(t)] * m if swapped else [int(s) for s in src]
        order = rng.permutation(len(r_f))
        rows += [r_f[i] for i in order]
        cols += [c_f[i] for i in order]
        n_frame.append(len(r_f))
    if swapped:
        assert several > 0  # pixels whose entries share columns: per-column partials differ from a plain sum
    if variant == "empty0":
        assert n_frame[0] == 0 and n_frame[1] > 0
    else:
        assert n_frame[0] > 0  # frame 1's entry slots start past 0
    col_pix = np.asarray(col_pix, np.int64)
    ih, iw = (H, W) if swapped else (hs, ws)
    idx = np.stack([col_pix // (ih * iw), col_pix % (ih * iw) // iw, col_pix % iw], 1)
    mij = np.stack([np.asarray(rows, np.int64), np.asarray(cols, np.int64)], 1)
    mval = rng.uniform(-2, 2, len(mij)).astype(np.float32)
    return {"mij": np.ascontiguousarray(mij), "mval": mval, "idx": np.ascontiguousarray(idx), "counts": counts,
            "m_size": np.array([F * (n_src if swapped else H * W), len(col_pix)], np.int64),
            "img_shape": (F, ih, iw), "n_frame": n_frame, "shape": shape, "src_shape": (F, hs, ws)}


def occupied(m):
    """[F, H, W] bool: the target cells with entries."""
    return m["counts"] > 0


def wgrad_geom(n_frames, h, w, c_a, c_b, c_out):
    """{n_items, n_groups, n_cit, n_cot, strips, n_bands} of the row-streaming weight gradient, by the formulas
    of shpl_conv_rows.hip: items are (frame, band, strip) with strips fastest; 32-channel input tiles of A then
    of B, 32-channel output tiles; wgrad_sizes' n_groups = min(2048 / (n_cit n_cot), n_items)."""
    strips, _, n_bands, _ = row_geom(h, w)
    n_items = n_frames * n_bands * strips
    n_cit, n_cot = (c_a + 31) // 32 + (c_b + 31) // 32, (c_out + 31) // 32
    return {"n_items": n_items, "n_groups": min(max(2048 // (n_cit * n_cot), 1), max(n_items, 1)), "n_cit": n_cit,
            "n_cot": n_cot, "strips": strips, "n_bands": n_bands}


def group_items(g, grp):
    """The items group grp walks: [grp n_items / n_groups, (grp + 1) n_items / n_groups), as (frame, band, strip)."""
    out = []
    for item in range(grp * g["n_items"] // g["n_groups"], (grp + 1) * g["n_items"] // g["n_groups"]):
        strip, fb = item % g["strips"], item // g["strips"]
        out.append((fb // g["n_bands"], fb % g["n_bands"], strip))
    return out


def straddles(g):
    """(groups whose consecutive items cross a frame boundary, groups whose items cross a band boundary inside a
    frame, the largest number of items of a group)."""
    frame, band, most = [], [], 0
    for grp in range(g["n_groups"]):
        it = group_items(g, grp)
        most = max(most, len(it))
        for (f0, b0, _), (f1, b1, _) in zip(it, it[1:]):
            if f0 != f1:
                frame.append(grp)
            elif b0 != b1:
                band.append(grp)
    return frame, band, most
