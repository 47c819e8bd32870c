"""The ragged levels index entry point of the C ABI (CPU only: no compute calls, no GPU needed): it is exported
and declared, and bad arguments are rejected on the host in shpl_build_index_levels' order -- pointers (d_im_sizes
and level_img_hw among them), the level count, every level's arrays, then shapes (a level's padded map among its
strides and BEV size), then the 2^31 bound per level (on the padded map's pixels and on the cells), then the
workspace, then the type codes."""
import ctypes
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from sparse_pooling_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        from sparse_pooling_amd import build
        build.build()
    return L, L.lib()


def test_levels_ragged_symbol_is_declared_and_exported():
    L, lib = _lib()
    header = open(os.path.join(ROOT, "include", "shpl.h")).read()
    name = "shpl_build_index_levels_ragged"
    assert name + "(" in header and hasattr(lib, name) and name in L.EXPORTED
    decl = header[header.index("int " + name + "("):]
    decl = decl[:decl.index(";")]
    assert "const double *d_im_sizes" in decl and "const int64_t *level_img_hw" in decl
    assert "im_w" not in decl and "im_h" not in decl
    # the levels entry's comment no longer says that there is no ragged form, and points at this one
    assert "no ragged form" not in header
    assert header.count(name) >= 2
    assert "#define SHPL_MAX_INDEX_LEVELS 4" in header  # shpl_index_level is shared, unchanged
    assert ctypes.sizeof(L.ShplIndexLevel) == 4 * 8 + 6 * ctypes.sizeof(ctypes.c_void_p)


P = 256  # a fake, aligned, non-null device pointer: never dereferenced
N = None
AVOD = [dict(s=(1., 1.), bv=(700., 800.), hw=(376, 1242)), dict(s=(8., 8.), bv=(704., 800.), hw=(47, 155))]
HW_DEFAULT = object()


def _levels(L, specs):
    arr = (L.ShplIndexLevel * max(len(specs), 1))()
    for a, sp in zip(arr, specs):
        a.s_img, a.s_bv = sp["s"]
        a.bv_h, a.bv_w = sp["bv"]
        for k in ("cell", "pix", "val", "frame_nnz"):
            setattr(a, k, sp.get(k, P))
        a.mij, a.flip = sp.get("mij"), sp.get("flip")
    return arr


def _call(L, lib, specs=AVOD, n_levels=None, levels="array", hws=HW_DEFAULT, n_frames=1, off=P, maxp=10, pts=P, vox=P,
          vstride=2, Pm=P, sizes=P, ws=P, ws_bytes=1 << 20, pdt=2, vit=1):
    arr = _levels(L, specs) if levels == "array" else levels
    maps = L.index_level_maps([sp["hw"] for sp in specs]) if hws is HW_DEFAULT else hws
    v = ctypes.c_void_p
    return lib.shpl_build_index_levels_ragged(n_frames, v(off), N, maxp, v(pts), pdt, v(vox), vit, vstride, v(Pm),
                                              v(sizes), N, len(specs) if n_levels is None else n_levels, arr, maps,
                                              v(P), N, v(ws), ws_bytes, N)


def _with(i, **kw):
    """AVOD with level i's fields replaced."""
    return [dict(sp, **kw) if k == i else sp for k, sp in enumerate(AVOD)]


def test_levels_ragged_rejections_in_the_listed_order():
    L, lib = _lib()
    assert L.F64 == 2 and L.I64 == 1
    # a good call gets as far as the workspace check
    assert _call(L, lib, ws_bytes=16) == L.ERR_WORKSPACE
    # 1. NULL d_im_sizes, NULL level_img_hw: with the pointers, SHPL_ERR_ARG -- ahead of every shape
    assert _call(L, lib, sizes=None) == L.ERR_ARG
    assert _call(L, lib, hws=None) == L.ERR_ARG
    assert _call(L, lib, sizes=None, n_levels=9) == L.ERR_ARG
    assert _call(L, lib, hws=None, n_levels=0) == L.ERR_ARG
    assert _call(L, lib, sizes=None, vstride=1) == L.ERR_ARG
    assert _call(L, lib, _with(0, s=(0., 1.)), hws=None) == L.ERR_ARG
    assert _call(L, lib, _with(1, hw=(0, 155)), sizes=None) == L.ERR_ARG
    # the levels entry's own pointers and their order
    for kw in (dict(n_frames=0), dict(off=None), dict(Pm=None), dict(ws=None), dict(pts=None), dict(vox=None),
               dict(levels=None, n_levels=2)):
        assert _call(L, lib, **kw) == L.ERR_ARG, kw
    for n in (0, -1, L.MAX_INDEX_LEVELS + 1, 1 << 20):  # the count, before levels[] and level_img_hw[] are read
        assert _call(L, lib, n_levels=n) == L.ERR_BAD_SHAPE, n
    for lv in (0, 1):
        for k in ("cell", "pix", "val", "frame_nnz"):
            assert _call(L, lib, _with(lv, **{k: None})) == L.ERR_ARG, (lv, k)
            assert _call(L, lib, _with(lv, **{k: None, "hw": (0, 0)})) == L.ERR_ARG, (lv, k)  # arrays before shapes
    # 2. a level's map size < 1: with that level's shapes, SHPL_ERR_BAD_SHAPE
    for lv in (0, 1):
        for hw in ((0, 155), (47, 0), (-1, 155), (47, -(1 << 40)), (0, 0)):
            assert _call(L, lib, _with(lv, hw=hw)) == L.ERR_BAD_SHAPE, (lv, hw)
            assert _call(L, lib, _with(lv, hw=hw), ws_bytes=16) == L.ERR_BAD_SHAPE, (lv, hw)  # before the workspace
        for s in ((0., 8.), (8., 0.), (float("nan"), 1.)):
            assert _call(L, lib, _with(lv, s=s)) == L.ERR_BAD_SHAPE, (lv, s)
        for bv in ((-1., 800.), (704., float("inf"))):
            assert _call(L, lib, _with(lv, bv=bv)) == L.ERR_BAD_SHAPE, (lv, bv)
    assert _call(L, lib, vstride=1) == L.ERR_BAD_SHAPE
    # 3. the 2^31 bound per level on n_frames * img_rows * img_cols: 376 x 1242 pixels, 4598 frames pass, 4599 do
    # not (4599 * 466992 = 2147696208 >= 2^31 - 1); the map decides, not a size of the frames
    px = [dict(s=(1., 8.), bv=(704., 800.), hw=(376, 1242))]  # 8800 cells
    assert 4598 * 376 * 1242 < 2147483647 <= 4599 * 376 * 1242
    assert _call(L, lib, px, n_frames=4598, ws_bytes=16) == L.ERR_WORKSPACE  # in bounds: the next check
    assert _call(L, lib, px, n_frames=4599, ws_bytes=16) == L.ERR_BAD_SHAPE
    small = [dict(px[0], hw=(47, 155))]
    assert _call(L, lib, small, n_frames=4599, ws_bytes=16) == L.ERR_WORKSPACE
    assert _call(L, lib, small + px, n_frames=4599, ws_bytes=16) == L.ERR_BAD_SHAPE  # whichever level
    assert _call(L, lib, px + small, n_frames=4599, ws_bytes=16) == L.ERR_BAD_SHAPE
    # a product past 2^63 is saturated, not wrapped
    for hw in ((1 << 62, 4), (1 << 32, 1 << 32), ((1 << 63) - 1, (1 << 63) - 1)):
        assert _call(L, lib, [dict(px[0], hw=hw)], ws_bytes=16) == L.ERR_BAD_SHAPE, hw
    # and on the cells: 3834 frames x 700 x 800 pass, 3835 do not
    tiny = [dict(sp, hw=(10, 10)) for sp in AVOD]
    assert _call(L, lib, tiny, n_frames=3834, ws_bytes=16) == L.ERR_WORKSPACE
    assert _call(L, lib, tiny, n_frames=3835, ws_bytes=16) == L.ERR_BAD_SHAPE
    assert _call(L, lib, tiny[1:], n_frames=3835, ws_bytes=16) == L.ERR_WORKSPACE
    # 4. then the workspace (the levels entry's query), then the type codes
    need = L.index_levels_ws_bytes(64, 100000, 2)
    assert _call(L, lib, n_frames=64, maxp=100000, ws_bytes=need - 1) == L.ERR_WORKSPACE
    assert _call(L, lib, pdt=7, ws_bytes=16) == L.ERR_WORKSPACE
    assert _call(L, lib, pdt=7) == L.ERR_ARG and _call(L, lib, vit=7) == L.ERR_ARG


def test_index_level_maps_helper_layout():
    """_lib.index_level_maps: the host array [n_levels][2] i64 of (img_rows, img_cols)."""
    L, _ = _lib()
    arr = L.index_level_maps([(376, 1242), (47, 155), (1 << 40, 3)])
    assert ctypes.sizeof(arr) == 3 * 2 * 8 and arr._type_ is ctypes.c_int64
    assert list(arr) == [376, 1242, 47, 155, 1 << 40, 3]
    assert len(L.index_level_maps([])) == 0
    import numpy as np
    assert list(L.index_level_maps([np.array([5, 7]), (np.int64(2), 3.0)])) == [5, 7, 2, 3]


def test_build_index_levels_keywords():
    """shpl_map.build_index_levels takes im_sizes and img_hws (checked by signature: no GPU here)."""
    import inspect
    from sparse_pooling_amd import shpl_map as sm
    params = inspect.signature(sm.build_index_levels).parameters
    assert params["im_sizes"].default is None and params["img_hws"].default is None
