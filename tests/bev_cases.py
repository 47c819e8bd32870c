"""Planted clouds for the BEV slice voxelizer (shpl_bev.hip) and its one-workgroup tile sort
(shpl_tilesort.h), small enough for small grids, plus a plain numpy listing of a cloud's sorted words.

Every builder is seeded and returns the voxelizer's arguments

    (cloud (3, n) f64, plane (4,), area_extents (3, 2), voxel_size, height_lo, height_hi, num_slices)

``sorted_words`` follows the description at the top of shpl_bev.hip: one word (v, xi, zi, yd, point) per
(point, slice) membership, v = slice or num_slices for the density range, in (v, xi, zi, yd, point) order. It is
there to check that a case reaches the path it was planted for (tests/test_bev_cases.py) -- expected outputs
come from the reference's goldens (tests/golden/bev_edges.npz) and from the C oracle, never from it. Its plane
test is a plain left-to-right sum: exact for planes (0, -1, 0, d), and no case plants a height within an ulp of
a slice plane of a tilted one.
"""
import collections

import numpy as np

TS_TILES, TS_WIN, BEV_BLOCK, MAP_STRIDE = 16384, 10240, 1024, 4096  # shpl_tilesort.h, shpl_bev.hip

PLANE = np.array([0.0, -1.0, 0.0, 1.65])
KITTI_PLANE = np.array([-1.851372e-02, -9.998285e-01, -5.362401e-04, 1.678541e+00])  # synth.KITTI_PLANE
PLANE2 = np.array([0.03, -2.0, -0.011, 3.4])  # not normalised

Grid = collections.namedtuple("Grid", "ext vs S hlo hhi")


def _grid(x, z, vs=0.1, S=5, y=(-5.0, 3.0), hlo=-0.2, hhi=2.3):
    return Grid(np.array([x, y, z], dtype=np.float64), vs, S, hlo, hhi)


GRIDS = {
    "G0": _grid([-2, 2], [0, 4]),                      # 40 x 40 x 6 = 9600 keys: one key per tile
    "G4": _grid([-8, 8], [0, 16]),                     # 153 600 keys: 16 keys per tile
    "G0s1": _grid([-2, 2], [0, 4], S=1),
    "G0s8": _grid([-2, 2], [0, 4], S=8),               # BEV_MAX_SLICES, 14 400 keys
    # min_x = -30, min_z = -20, every discrete y negative; the height range reaches past the upper y extent,
    # so a point on y = -0.1 is dropped by the strict bound alone
    "Gneg": _grid([-3, 1], [-2, 2], y=(-5.0, -0.1), hlo=1.5, hhi=6.0),
    "Gover": _grid([-0.9, 0.9], [0, 14.4], vs=0.3, S=2),  # 0.9 / 0.3 and 14.4 / 0.3 round to integers
}

Geom = collections.namedtuple("Geom", "min_x min_y min_z nx nz n_cells n_keys log_tile")


def geom(ext, vs, S):
    """bev_geom of shpl_bev.hip (voxel_grid_2d.py:127-149)."""
    ext = np.asarray(ext, dtype=np.float64).reshape(3, 2)
    min_x, min_y, min_z = (int(np.floor(ext[i, 0] / vs)) for i in range(3))
    nx = int(np.ceil(ext[0, 1] / vs - 1) - min_x + 1)
    nz = int(np.ceil(ext[2, 1] / vs - 1) - min_z + 1)
    n_keys = nx * nz * (S + 1)
    log_tile = 0
    while ((n_keys - 1) >> log_tile) + 1 > TS_TILES:
        log_tile += 1
    return Geom(min_x, min_y, min_z, nx, nz, nx * nz, n_keys, log_tile)


def slice_bounds(hlo, hhi, S):
    """bev_slices.py:30-31, :66-67."""
    hpd = (hhi - hlo) / S
    lo = [hlo + s * hpd for s in range(S)]
    return hpd, lo, [v + hpd for v in lo]


def sorted_words(cloud, plane, ext, vs, hlo, hhi, S):
    """The frame's sorted words, int64 [n_ent, 5]: columns (v, xi, zi, yd, point)."""
    cloud = np.asarray(cloud, dtype=np.float64).reshape(3, -1)
    ext = np.asarray(ext, dtype=np.float64).reshape(3, 2)
    g = geom(ext, vs, S)
    x, y, z = cloud
    inside = ((x > ext[0, 0]) & (x < ext[0, 1]) & (y > ext[1, 0]) & (y < ext[1, 1]) &
              (z > ext[2, 0]) & (z < ext[2, 1]))
    xd, yd, zd = (np.floor(c / vs).astype(np.int64) for c in (x, y, z))
    _, lo, hi = slice_bounds(hlo, hhi, S)
    lo, hi = lo + [hlo], hi + [hhi]

    def below(off):
        return plane[0] * x + plane[1] * y + plane[2] * z + (plane[3] - off) < 0

    rows = []
    for v in range(S + 1):
        i = np.nonzero(inside & (below(hi[v]) != below(lo[v])))[0]
        rows.append(np.stack([np.full(i.size, v), xd[i] - g.min_x, zd[i] - g.min_z, yd[i], i], axis=1))
    w = np.concatenate(rows).astype(np.int64).reshape(-1, 5)
    return w[np.lexsort((w[:, 4], w[:, 3], w[:, 2], w[:, 1], w[:, 0]))]


def key_runs(words, g):
    """(key of each run, first word of each run, length of each run) of sorted words."""
    key = words[:, 0] * g.n_cells + words[:, 1] * g.nz + words[:, 2]
    start = np.nonzero(np.r_[True, key[1:] != key[:-1]])[0] if key.size else np.zeros(0, np.int64)
    return key[start], start, np.diff(np.r_[start, key.size])


def in_grid(words, g):
    return bool(((words[:, 1] >= 0) & (words[:, 1] < g.nx) & (words[:, 2] >= 0) & (words[:, 2] < g.nz)).all())


# ---- planting ------------------------------------------------------------------------------------------

def _args(cloud, plane, G):
    return (np.ascontiguousarray(cloud, dtype=np.float64).reshape(3, -1), np.array(plane, dtype=np.float64),
            G.ext.copy(), G.vs, G.hlo, G.hhi, G.S)


def _in_cell(G, g, rng, cell, n):
    """n (x, z) pairs well inside cell = xi * nz + zi."""
    xi, zi = np.divmod(np.asarray(cell), g.nz)
    return ((g.min_x + xi + rng.uniform(0.15, 0.85, n)) * G.vs, (g.min_z + zi + rng.uniform(0.15, 0.85, n)) * G.vs)


def _y_of_height(G, rng, s, n, d=PLANE[3]):
    """y of n points of slice s (s = array or scalar) under the plane (0, -1, 0, d), away from the slice planes
    and inside the y extents."""
    hpd, lo, _ = slice_bounds(G.hlo, G.hhi, G.S)
    y = d - (np.asarray(lo)[s] + rng.uniform(0.05, 0.95, n) * hpd)
    assert (y > G.ext[1, 0] + 0.01).all()
    hi_ok = y < G.ext[1, 1] - 0.01  # Gneg's lowest slice reaches past the y extent: fold those back inside
    return np.where(hi_ok, y, G.ext[1, 1] - 0.01 - rng.uniform(0, 0.3, n))


def _scatter(G, g, rng, cells, slices=None):
    """One in-range point per entry of cells, in the given (or random) slices."""
    n = len(cells)
    x, z = _in_cell(G, g, rng, cells, n)
    s = rng.integers(0, G.S, n) if slices is None else np.broadcast_to(slices, (n,))
    return np.stack([x, _y_of_height(G, rng, s, n), z])


def _bands(G, s):
    """Discrete y values whose whole band [b, b + 1) * vs lies inside slice s and the y extents."""
    _, lo, hi = slice_bounds(G.hlo, G.hhi, G.S)
    y0 = max(PLANE[3] - hi[s], G.ext[1, 0]) + 0.02
    y1 = min(PLANE[3] - lo[s], G.ext[1, 1]) - 0.02
    return [b for b in range(int(np.floor(y0 / G.vs)) - 1, int(np.ceil(y1 / G.vs)) + 1)
            if b * G.vs >= y0 and (b + 1) * G.vs <= y1]


def _interleave(rng, groups):
    """Concatenate point groups [(3, n_i)] at random positions, each group keeping its own order."""
    total = sum(p.shape[1] for p in groups)
    out = np.empty((3, total))
    slots = rng.permutation(total)
    at = 0
    for p in groups:
        out[:, np.sort(slots[at:at + p.shape[1]])] = p
        at += p.shape[1]
    return out


def ties(grid="G0", seed=1):
    """60 cells of 2..40 points, each inside one slice. Memory order inside a cell of >= 3 points: a point of a
    larger discrete y, then the winner (smallest discrete y, earliest), then in random order the points that
    share the winner's discrete y (at other exact y, in every other cell a smaller one) and more points of
    larger discrete y. A 2-point cell holds two points of one discrete y. 240 one-point cells around them."""
    G = GRIDS[grid]
    g = geom(G.ext, G.vs, G.S)
    rng = np.random.default_rng(seed)
    cells = rng.choice(g.n_cells, 300, replace=False)
    counts = np.r_[[2, 2, 2, 3, 3, 3, 4, 5, 39, 40], rng.integers(2, 41, 50)]
    groups = [_scatter(G, g, rng, cells[60:])[:, [i]] for i in range(240)]
    for j, (c, n) in enumerate(zip(cells[:60], counts)):
        bands = _bands(G, j % G.S)
        b0 = bands[rng.integers(0, len(bands) - 1)]
        higher = [b for b in bands if b > b0]
        if n == 2:
            kinds = ["W", "T"]
        else:
            k = int(rng.integers(2, n))  # points of the smallest discrete y
            rest = ["T"] * (k - 1) + ["H"] * (n - 1 - k)
            kinds = ["H", "W"] + [rest[i] for i in rng.permutation(len(rest))]
        u_w = 0.5 if j % 2 == 0 else 0.1
        x, z = _in_cell(G, g, rng, c, n)
        y = np.empty(n)
        for i, kind in enumerate(kinds):
            if kind == "W":
                y[i] = (b0 + u_w) * G.vs
            elif kind == "T":
                y[i] = (b0 + (rng.uniform(0.12, 0.45) if j % 2 == 0 and i % 2 == 0 else rng.uniform(0.55, 0.9))) * G.vs
            else:
                y[i] = (higher[rng.integers(0, len(higher))] + rng.uniform(0.1, 0.9)) * G.vs
        if j % 2 == 0 and n > 2:  # one tie point surely above the winner's exact y... and one surely below
            y[kinds.index("T")] = (b0 + 0.2) * G.vs
        groups.append(np.stack([x, y, z]))
    return _args(_interleave(rng, groups), PLANE, G)


DENSITY_COUNTS = list(range(1, 18)) + [40, 300]


def density(seed=2):
    """Cells of exactly 1..17, 40 and 300 points inside the height range; every other one of them also holds
    3 points above height_hi and 2 below height_lo (inside the extents, in no slice). 100 one-point cells."""
    G = GRIDS["G0"]
    g = geom(G.ext, G.vs, G.S)
    rng = np.random.default_rng(seed)
    cells = rng.choice(g.n_cells, len(DENSITY_COUNTS) + 100, replace=False)
    parts = [_scatter(G, g, rng, cells[len(DENSITY_COUNTS):])]
    for j, (c, n) in enumerate(zip(cells, DENSITY_COUNTS)):
        parts.append(_scatter(G, g, rng, np.full(n, c)))
        if j % 2 == 0:
            x, z = _in_cell(G, g, rng, c, 5)
            h = np.r_[G.hhi + rng.uniform(0.05, 0.3, 3), G.hlo - rng.uniform(0.05, 0.3, 2)]
            parts.append(np.stack([x, PLANE[3] - h, z]))
    cloud = np.concatenate(parts, axis=1)
    return _args(cloud[:, rng.permutation(cloud.shape[1])], PLANE, G), cells[:len(DENSITY_COUNTS)]


def grid_lines(grid="G0", seed=3):
    """Points at exact multiples of the voxel size (as k * vs and as the nearest double of the decimal), on the
    six extent faces (dropped), one ulp inside each (kept where the height is in range) and on, just above and
    just below every slice plane of the plane (0, -1, 0, 1.65)."""
    G = GRIDS[grid]
    g = geom(G.ext, G.vs, G.S)
    rng = np.random.default_rng(seed)
    _, lo, hi = slice_bounds(G.hlo, G.hhi, G.S)

    def rand(n):  # in-range points in random cells
        return _scatter(G, g, rng, rng.integers(0, g.n_cells, n))

    pts = [rand(40)]
    for axis, first, count in ((0, g.min_x, g.nx), (2, g.min_z, g.nz)):
        vals = sorted({v for k in range(first, first + count + 1) for v in (k * G.vs, round(k * G.vs, 9))})
        p = rand(len(vals))
        p[axis] = vals
        pts.append(p)
    for axis in range(3):
        for side in range(2):
            e = G.ext[axis, side]
            p = rand(4)
            p[axis, :2] = e                                            # on the face
            p[axis, 2:] = np.nextafter(e, G.ext[axis, 1 - side])       # one ulp inside
            pts.append(p)
    for off in lo + hi:
        y0 = PLANE[3] - off
        p = rand(3)
        p[1] = [np.nextafter(y0, -np.inf), y0, np.nextafter(y0, np.inf)]
        pts.append(p)
    cloud = np.concatenate(pts, axis=1)
    return _args(cloud[:, rng.permutation(cloud.shape[1])], PLANE, G)


def tilted(plane=KITTI_PLANE, seed=4):
    """6000 points on G4, uniform in x, z and plane offset (some outside the height range), 1500 of them in 50
    cells; y solved from the plane."""
    G = GRIDS["G4"]
    g = geom(G.ext, G.vs, G.S)
    rng = np.random.default_rng(seed)
    x, z = rng.uniform(-7.99, 7.99, 6000), rng.uniform(0.01, 15.99, 6000)
    cx, cz = _in_cell(G, g, rng, np.repeat(rng.choice(g.n_cells, 50, replace=False), 30), 1500)
    x[:1500], z[:1500] = cx, cz
    x, z = _coarse(x), _coarse(z)  # the plane's coefficients keep every product inexact
    t = rng.uniform(G.hlo - 0.2, G.hhi + 0.2, 6000)
    y = (t - plane[0] * x - plane[2] * z - plane[3]) / plane[1]
    cloud = np.stack([x, y, z])
    return _args(cloud[:, rng.permutation(6000)], plane, G)


def _coarse(v):
    """Coordinates on a 2^-16 lattice, far finer than any margin the plants keep: they compress well in the
    committed fixture. Only where the case is about the order of the words, not about the arithmetic."""
    return np.round(np.asarray(v) * 65536.0) / 65536.0


def _planted(G, g, rng, spec, extra=None):
    """spec: [(slice, cell, count)] -> shuffled in-range points; extra: more columns."""
    sl, ce, n = (np.array([t[i] for t in spec], dtype=np.int64) for i in range(3))
    parts = [_scatter(G, g, rng, np.repeat(ce, n), np.repeat(sl, n))]
    if extra is not None:
        parts.append(extra)
    cloud = _coarse(np.concatenate(parts, axis=1))
    return cloud[:, rng.permutation(cloud.shape[1])]


def _out_of_range(G, g, rng, n):
    """Points that form no word: above / below the height range inside the extents, or outside the extents."""
    p = _scatter(G, g, rng, rng.integers(0, g.n_cells, n))
    k = np.arange(n) % 4
    p[1, k == 0] = PLANE[3] - (G.hhi + rng.uniform(0.05, 0.5, (k == 0).sum()))
    p[1, k == 1] = PLANE[3] - (G.hlo - rng.uniform(0.05, 0.5, (k == 1).sum()))
    p[0, k == 2] = G.ext[0, 1] + rng.uniform(0, 1, (k == 2).sum())
    p[2, k == 3] = G.ext[2, 0] - rng.uniform(0, 1, (k == 3).sum())
    return p


def window(which, grid="G0", seed=5):
    """The sort's LDS window (TS_WIN words), k_bev_frame's 1024-word chunks and k_bev_maps' 4096-word stride:
    a: 11 000 points of one slice in one cell (a tile larger than the window);
    b: a density run of 300 words over word 10240 (on G4: inside a tile of several keys);
    c: 5120 points in range, n_ent = 10240;   d: 512 points in range, n_ent = 1024;
    e: slice-0 runs [1024, 1074) and [2040, 2060);   f: slice-0 runs [4096, 4146) and [8190, 8200)."""
    G = GRIDS[grid]
    g = geom(G.ext, G.vs, G.S)
    rng = np.random.default_rng(seed + ord(which))
    mid = (g.nx // 2) * g.nz + g.nz // 2
    some = [(s, int(c), 1) for s in range(G.S) for c in rng.integers(0, g.n_cells, 6)]
    if which == "a":
        cloud = _planted(G, g, rng, [(2, mid, 11000)] + some)
    elif which == "b":
        spec = [(int(s), int(c), 1) for s, c in zip(rng.integers(0, G.S, 4100), rng.integers(0, mid, 4100))]
        spec += [(int(s), mid, 1) for s in rng.integers(0, G.S, 300)]
        near = 0 if g.log_tile == 0 else 80  # G4: 40 points in each of the next two cells of the same tile
        spec += [(int(s), mid + 1 + i % 2, 1) for i, s in enumerate(rng.integers(0, G.S, near))]
        spec += [(int(s), int(c), 1) for s, c in zip(rng.integers(0, G.S, 1600 - near),
                                                     rng.integers(mid + 16, g.n_cells, 1600 - near))]
        cloud = _planted(G, g, rng, spec)
    elif which in "cd":
        n = 5120 if which == "c" else 512
        cloud = _planted(G, g, rng, [(int(s), int(c), 1) for s, c in zip(rng.integers(0, G.S, n),
                                                                         rng.integers(0, g.n_cells, n))],
                         _out_of_range(G, g, rng, 300 if which == "c" else 100))
    else:
        counts = [1000, 24, 50, 966, 20] if which == "e" else [3000, 1096, 50, 4044, 10]
        cells = np.sort(rng.choice(g.n_cells, len(counts), replace=False))
        cloud = _planted(G, g, rng, [(0, int(c), n) for c, n in zip(cells, counts)] + [t for t in some if t[0] > 0])
    return _args(cloud, PLANE, G)


def sparse(which, seed=6):
    """empty: no point; one: one point in range; outside: 50 points outside the extents; above: 50 points inside
    the extents above height_hi; one_in_slice: slice 2 empty, slice 4 with exactly one point."""
    G = GRIDS["G0"]
    g = geom(G.ext, G.vs, G.S)
    rng = np.random.default_rng(seed)
    if which == "empty":
        cloud = np.zeros((3, 0))
    elif which == "one":
        cloud = _scatter(G, g, rng, [777], 3)
    elif which == "outside":
        cloud = _scatter(G, g, rng, rng.integers(0, g.n_cells, 50))
        k = np.arange(50) % 5
        cloud[0, k == 0], cloud[0, k == 1] = -2.0 - rng.uniform(0, 2, 10), 2.0 + rng.uniform(0, 2, 10)
        cloud[2, k == 2], cloud[2, k == 3] = -rng.uniform(0, 2, 10), 4.0 + rng.uniform(0, 2, 10)
        cloud[1, k == 4] = 3.0 + rng.uniform(0, 1, 10)
    elif which == "above":
        cloud = _scatter(G, g, rng, rng.integers(0, g.n_cells, 50))
        cloud[1] = PLANE[3] - (G.hhi + rng.uniform(0.01, 2.0, 50))
    else:
        s = np.r_[rng.choice([0, 1, 3], 200), 4]
        cloud = _scatter(G, g, rng, rng.integers(0, g.n_cells, 201), s)
        cloud = cloud[:, rng.permutation(201)]
    return _args(cloud, PLANE, G)


def slices(grid, seed=1):
    """The ties cloud cut into 1 or 8 slices."""
    G = GRIDS[grid]
    return _args(ties("G0", seed)[0], PLANE, G)


OVERFLOW_POINTS = (100, 200)  # columns of overflow()'s cloud


def overflow(seed=7):
    """300 ordinary points on Gover; point 100 has x = nextafter(0.9, 0) and point 200 z = nextafter(14.4, 0),
    both inside the extents and the height range: floor(x / 0.3) = 3 = min_x + nx, floor(z / 0.3) = 48 = nz."""
    G = GRIDS["Gover"]
    g = geom(G.ext, G.vs, G.S)
    rng = np.random.default_rng(seed)
    cloud = _scatter(G, g, rng, rng.integers(0, g.n_cells, 300))
    cloud[0, OVERFLOW_POINTS[0]] = np.nextafter(0.9, 0)
    cloud[2, OVERFLOW_POINTS[1]] = np.nextafter(14.4, 0)
    return _args(cloud, PLANE, G)


# name -> (builder, grid). GOLDEN: the cases the reference ran (tests/golden/bev_edges.npz).
CASES = {
    "ties_G0": (lambda: ties("G0"), "G0"),
    "ties_Gneg": (lambda: ties("Gneg", seed=11), "Gneg"),
    "density": (lambda: density()[0], "G0"),
    "grid_lines_G0": (lambda: grid_lines("G0"), "G0"),
    "grid_lines_Gneg": (lambda: grid_lines("Gneg", seed=13), "Gneg"),
    "tilted_kitti": (lambda: tilted(KITTI_PLANE), "G4"),
    "tilted_plane2": (lambda: tilted(PLANE2, seed=14), "G4"),
    "window_a": (lambda: window("a"), "G0"),
    "window_b": (lambda: window("b"), "G0"),
    "window_b_G4": (lambda: window("b", "G4"), "G4"),
    "window_c": (lambda: window("c"), "G0"),
    "window_d": (lambda: window("d"), "G0"),
    "window_e": (lambda: window("e"), "G0"),
    "window_f": (lambda: window("f"), "G0"),
    "sparse_empty": (lambda: sparse("empty"), "G0"),
    "sparse_one": (lambda: sparse("one"), "G0"),
    "sparse_outside": (lambda: sparse("outside"), "G0"),
    "sparse_above": (lambda: sparse("above"), "G0"),
    "sparse_one_in_slice": (lambda: sparse("one_in_slice"), "G0"),
    "slices_s1": (lambda: slices("G0s1"), "G0s1"),
    "slices_s8": (lambda: slices("G0s8"), "G0s8"),
}
GOLDEN = ["ties_G0", "ties_Gneg", "density", "grid_lines_G0", "grid_lines_Gneg", "tilted_kitti", "tilted_plane2",
          "window_b", "window_e", "slices_s1", "slices_s8"]

_built = {}


def case(name):
    """The arguments of a case, built once (the arrays are shared: do not write to them)."""
    if name not in _built:
        _built[name] = overflow() if name == "overflow" else CASES[name][0]()
        _built[name][0].setflags(write=False)
    return _built[name]


_expected = {}


def expected(name, golden):
    """(height_maps, density_map, voxel_indices, pts_in_voxel) of a case: the reference's where it ran
    (golden: the loaded bev_edges.npz), the oracle's otherwise. Computed once."""
    if name not in _expected:
        if name in GOLDEN:
            _expected[name] = tuple(golden[f"{name}/{k}"] for k in ("height_maps", "density_map", "voxel_indices",
                                                                    "pts_in_voxel"))
        else:
            from oracle import shpl_oracle as orc
            _expected[name] = orc.bev_slices(*case(name))
    return _expected[name]
