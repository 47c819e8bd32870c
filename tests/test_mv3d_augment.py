"""MV3D's augment_voxel, the host half (no GPU): the seeded draws and the
ground-truth boxes against the reference-generated fixtures
(tests/golden/mv3d_augment_*.npz, make_mv3d_augment_golden.py), and the host
checks of the two augmented C-ABI entry points."""
import ctypes
import glob
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(glob.glob(os.path.join(GOLD, "mv3d_augment_*.npz")))
IDS = [os.path.basename(p)[len("mv3d_augment_"):-len(".npz")] for p in CASES]


def test_the_fixture_cases_are_all_there():
    assert set(IDS) == {"f64", "f64_pc", "f32", "f32_pc", "dense", "one_f64", "one_f32", "none", "planted"}


@pytest.mark.parametrize("path", CASES, ids=IDS)
def test_seeded_draws_equal_the_reference(path):
    """np.random.seed(s); draw_voxel_aug(...) draws what the reference's augment_voxel drew after the same seed:
    shift, ratio, angle, the rotation it forms from the angle and AUGMENT_PC's remain_index."""
    from sparse_pooling_amd import mv3d
    g = np.load(path)
    np.random.seed(int(g["seed"]))
    q = mv3d.draw_voxel_aug(float(g["scale"]), g["points"].shape[0], bool(g["augment_pc"]))
    np.testing.assert_array_equal(np.array([q["sx"], q["sz"], q["ratio"][0], q["angle"][0]]), g["params"])
    np.testing.assert_array_equal(q["rot"], g["rot"])
    if g["augment_pc"]:
        assert q["remain_index"].dtype == np.int64
        np.testing.assert_array_equal(q["remain_index"], g["remain_index"])
    else:
        assert q["remain_index"] is None
    row = mv3d.vox_aug_rows([q])
    assert row.shape == (1, 8) and row.dtype == np.float64
    np.testing.assert_array_equal(row[0], [*g["params"][:3], *g["rot"].reshape(4), 0.0])


@pytest.mark.parametrize("path", CASES, ids=IDS)
def test_boxes_equal_the_reference_bit_for_bit(path):
    from sparse_pooling_amd import mv3d
    g = np.load(path)
    np.random.seed(int(g["seed"]))
    q = mv3d.draw_voxel_aug(float(g["scale"]), g["points"].shape[0], bool(g["augment_pc"]))
    blobs = {"gt_boxes_3d": g["boxes_before"].copy(), "gt_rys": g["rys_before"].copy()}
    assert mv3d.augment_voxel_boxes(blobs, q) is blobs
    assert blobs["gt_boxes_3d"].dtype == g["boxes_after"].dtype
    np.testing.assert_array_equal(blobs["gt_boxes_3d"], g["boxes_after"])
    np.testing.assert_array_equal(blobs["gt_rys"], g["rys_after"])
    assert not np.array_equal(g["boxes_after"], g["boxes_before"])


def test_augment_voxel_without_a_cloud_returns_the_blobs():
    """The reference's lidar_pc=None branch: draws, boxes, and blobs alone come back (no device needed)."""
    from sparse_pooling_amd import mv3d
    g = np.load(os.path.join(GOLD, "mv3d_augment_f64.npz"))
    blobs = {"gt_boxes_3d": g["boxes_before"].copy(), "gt_rys": g["rys_before"].copy()}
    np.random.seed(int(g["seed"]))
    out = mv3d.augment_voxel(blobs, scale=float(g["scale"]))
    assert out is blobs
    np.testing.assert_array_equal(blobs["gt_boxes_3d"], g["boxes_after"])


def test_planted_fixture_has_the_rounding_cases():
    """The planted cloud: per coordinate at least 8 points whose augmented value, rounded to f32 as the reference
    rounds it, lands in another voxel or on the other side of a strict bound than the unrounded f64 value."""
    g = np.load(os.path.join(GOLD, "mv3d_augment_planted.npz"))
    p, a = g["points"], g["aug_points"]
    assert p.dtype == np.float32 and a.dtype == np.float32
    sx, sz, ratio = g["params"][:3]
    u = p.astype(np.float64)
    u[:, 0] += sx
    u[:, 2] += sz
    u[:, 0:3] *= ratio
    xz = g["rot"] @ u[:, [0, 2]].T
    u[:, 0], u[:, 2] = xz[0], xz[1]
    for col, (lo, hi, res) in enumerate(((-20.0, 20 - 0.01, 0.2), (-1.0, 3 - 0.01, 0.4), (0.0, 48 - 0.01, 0.2))):
        f32 = np.float32
        in_a = (a[:, col] > f32(lo)) & (a[:, col] < f32(hi))
        in_u = (u[:, col] > lo) & (u[:, col] < hi)
        c_a = ((a[:, col] - f32(lo)) / f32(res)).astype(np.int32)
        c_u = ((u[:, col] - lo) / res).astype(np.int32)
        assert int(((in_a != in_u) | (in_a & (c_a != c_u))).sum()) >= 8, col


# ---------------------------------------------------------------- C ABI, host side

P = ctypes.c_void_p(256)  # a fake, aligned, non-null device pointer: never dereferenced by the host checks
N = None
RNG = (ctypes.c_double * 6)(0, 48 - 0.01, -20, 20 - 0.01, -1, 3 - 0.01)


def _lib():
    from sparse_pooling_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        from sparse_pooling_amd import build
        build.build()
    return L, L.lib()


def _voxels_aug(lib, **kw):
    a = dict(n_frames=1, off=P, n=10, pts=P, dtype=0, stride=4, img2=N, Pm=P, fv=N, aug=P, remain=N, roff=N, n_out=10,
             rng=RNG, res=0.2, zres=0.4, cap=45, img=P, ld=10, bv=P, mv=P, fn=P, nb=N, nvox=N, err=N, ws=P,
             ws_bytes=1 << 20, stream=N)
    a.update(kw)
    return lib.shpl_mv3d_voxels_aug(*a.values())


def _augment_points(lib, **kw):
    a = dict(n_frames=1, off=P, n=10, pts=P, dtype=0, stride=4, Pm=P, aug=P, remain=N, roff=N, n_out=10, cloud=P,
             img2=P, ld=10, err=N, stream=N)
    a.update(kw)
    return lib.shpl_mv3d_augment_points(*a.values())


def test_abi_exports_and_error_bit():
    L, lib = _lib()
    hdr = open(os.path.join(os.path.dirname(GOLD), "..", "include", "shpl.h")).read()
    for name in ("shpl_mv3d_augment_points", "shpl_mv3d_voxels_aug"):
        assert hasattr(lib, name) and name in L.EXPORTED and name in hdr
    assert L.EBIT_GATHER == 64 and "#define SHPL_EBIT_GATHER 64u" in hdr


@pytest.mark.parametrize("call", [_voxels_aug, _augment_points], ids=["voxels_aug", "augment_points"])
def test_abi_host_checks(call):
    """Null or inconsistent pointers: SHPL_ERR_ARG. A cloud type other than f32 / f64, negative totals, or out
    points that differ from the points without a gather: SHPL_ERR_BAD_SHAPE. All before any launch."""
    L, lib = _lib()
    for k in ("off", "pts", "aug"):
        assert call(lib, **{k: N}) == L.ERR_ARG, k
    assert call(lib, n_frames=0) == L.ERR_ARG
    assert call(lib, remain=P) == L.ERR_ARG  # remain_index without its offsets
    assert call(lib, roff=P) == L.ERR_ARG
    for dt in (L.BF16, 3, -1):
        assert call(lib, dtype=dt) == L.ERR_BAD_SHAPE, dt
    assert call(lib, n=-1, n_out=-1) == L.ERR_BAD_SHAPE
    assert call(lib, n_out=-1, remain=P, roff=P) == L.ERR_BAD_SHAPE
    assert call(lib, n_out=9) == L.ERR_BAD_SHAPE  # no gather: every point is an out point
    assert call(lib, ld=9) == L.ERR_BAD_SHAPE
    assert call(lib, n=1 << 31, n_out=1 << 31, ld=1 << 31) == L.ERR_BAD_SHAPE


def test_abi_voxels_aug_workspace_and_outputs():
    L, lib = _lib()
    need = ctypes.c_size_t()
    assert lib.shpl_mv3d_workspace_bytes(1000, ctypes.byref(need)) == L.OK
    # the workspace is sized for the OUT points: 10 points gathered into 1000
    assert _voxels_aug(lib, remain=P, roff=P, n_out=1000, ld=1000, ws_bytes=need.value - 1) == L.ERR_WORKSPACE
    assert _voxels_aug(lib, ws_bytes=16) == L.ERR_WORKSPACE
    assert _voxels_aug(lib, ws=N) == L.ERR_ARG
    assert _voxels_aug(lib, Pm=N) == L.ERR_ARG  # neither img_index2 nor P
    assert _voxels_aug(lib, nb=P) == L.ERR_ARG  # number_buffer without frame_nvox
    for k in ("img", "bv", "mv", "fn", "rng"):
        assert _voxels_aug(lib, **{k: N}) == L.ERR_ARG, k
    assert _voxels_aug(lib, stride=2) == L.ERR_BAD_SHAPE
    assert _voxels_aug(lib, res=0.0) == L.ERR_BAD_SHAPE
    assert _voxels_aug(lib, cap=0) == L.ERR_BAD_SHAPE


def test_abi_augment_points_outputs():
    L, lib = _lib()
    assert _augment_points(lib, Pm=N) == L.ERR_ARG  # the materialised form always projects
    assert _augment_points(lib, cloud=N) == L.ERR_ARG
    assert _augment_points(lib, img2=N) == L.ERR_ARG
    assert _augment_points(lib, stride=3) == L.ERR_BAD_SHAPE  # it copies r
    assert _augment_points(lib, cloud=ctypes.c_void_p(264)) == L.ERR_BAD_SHAPE  # rows are stored 16 bytes at a time
    assert _augment_points(lib, n=0, n_out=0, pts=N, cloud=N, img2=N, ld=0) == L.OK  # nothing to do, nothing launched


def test_existing_producer_keeps_its_signature():
    """shpl_mv3d_voxels is called positionally by its callers: same 22 arguments, same statuses."""
    L, lib = _lib()
    assert len(lib.shpl_mv3d_voxels.argtypes) == 22
    assert lib.shpl_mv3d_voxels(1, P, 10, P, 4, N, N, N, RNG, 0.2, 0.4, 45, P, 10, P, P, P, N, N, P, 1 << 20,
                                N) == L.ERR_ARG
    assert lib.shpl_mv3d_voxels(1, P, 10, P, 4, N, P, N, RNG, 0.2, 0.4, 45, P, 10, P, P, P, N, N, P, 16,
                                N) == L.ERR_WORKSPACE
