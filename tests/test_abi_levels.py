"""The levels index entry points of the C ABI (CPU only: no compute calls, no GPU needed): both are exported, bad
arguments are rejected on the host in shpl_build_index's order -- pointers (levels and, once the level count is
known to be in range, every level's arrays among them), then shapes (the level count and every level's strides and BEV size among them), then the 2^31 bound per
level, then the workspace -- and config.fusion_levels gives the levels the reference's configs imply."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from sparse_pooling_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        from sparse_pooling_amd import build
        build.build()
    return L, L.lib()


def test_levels_symbols_are_declared_and_exported():
    L, lib = _lib()
    header = open(os.path.join(ROOT, "include", "shpl.h")).read()
    for name in ("shpl_build_index_levels", "shpl_build_index_levels_workspace_bytes"):
        assert name + "(" in header
        assert hasattr(lib, name)
        assert name in L.EXPORTED
    assert "#define SHPL_MAX_INDEX_LEVELS 4" in header and L.MAX_INDEX_LEVELS == 4
    assert "} shpl_index_level;" in header
    # the header says where the reference builds and reads the list
    assert "kitti_dataset.py:374-389" in header and "rpn_model.py:841-862" in header
    # struct shpl_index_level: four doubles, six pointers
    assert ctypes.sizeof(L.ShplIndexLevel) == 4 * 8 + 6 * ctypes.sizeof(ctypes.c_void_p)
    assert [n for n, _ in L.ShplIndexLevel._fields_] == ["s_img", "s_bv", "bv_h", "bv_w", "cell", "pix", "val", "mij",
                                                         "flip", "frame_nnz"]


P = 256  # a fake, aligned, non-null device pointer: never dereferenced
N = None
AVOD = [dict(s=(1., 1.), bv=(700., 800.)), dict(s=(8., 8.), bv=(704., 800.))]


def _levels(L, specs):
    arr = (L.ShplIndexLevel * max(len(specs), 1))()
    for a, sp in zip(arr, specs):
        a.s_img, a.s_bv = sp["s"]
        a.bv_h, a.bv_w = sp["bv"]
        for k in ("cell", "pix", "val", "frame_nnz"):
            setattr(a, k, sp.get(k, P))
        a.mij, a.flip = sp.get("mij"), sp.get("flip")
    return arr


def _call(L, lib, specs=AVOD, n_levels=None, levels="array", n_frames=1, off=P, maxp=10, pts=P, vox=P, vstride=2, Pm=P,
          im=(1242., 375.), ws=P, ws_bytes=1 << 20, pdt=2, vit=1):
    arr = _levels(L, specs) if levels == "array" else levels
    v = ctypes.c_void_p
    return lib.shpl_build_index_levels(n_frames, v(off), N, maxp, v(pts), pdt, v(vox), vit, vstride, v(Pm), im[0],
                                       im[1], N, len(specs) if n_levels is None else n_levels, arr, v(P), N, v(ws),
                                       ws_bytes, N)


def _with(i, **kw):
    """AVOD with level i's fields replaced."""
    return [dict(sp, **kw) if k == i else sp for k, sp in enumerate(AVOD)]


def test_levels_rejections_in_the_listed_order():
    L, lib = _lib()
    assert L.F64 == 2 and L.I64 == 1
    # 1. the level count, and a level's bad stride or size: SHPL_ERR_BAD_SHAPE
    for n in (0, -1, L.MAX_INDEX_LEVELS + 1, 1 << 20):
        assert _call(L, lib, n_levels=n) == L.ERR_BAD_SHAPE, n
    for lv in (0, 1):
        for s in ((0., 8.), (8., 0.), (-1., 1.), (float("nan"), 1.), (1., float("nan"))):
            assert _call(L, lib, _with(lv, s=s)) == L.ERR_BAD_SHAPE, (lv, s)
        for bv in ((-1., 800.), (704., -800.), (float("nan"), 800.), (704., float("inf"))):
            assert _call(L, lib, _with(lv, bv=bv)) == L.ERR_BAD_SHAPE, (lv, bv)
    assert _call(L, lib, vstride=1) == L.ERR_BAD_SHAPE
    # 2. a NULL levels, a level's NULL cell / pix / val / frame_nnz: SHPL_ERR_ARG
    assert _call(L, lib, levels=None, n_levels=2) == L.ERR_ARG
    for lv in (0, 1):
        for k in ("cell", "pix", "val", "frame_nnz"):
            assert _call(L, lib, _with(lv, **{k: None})) == L.ERR_ARG, (lv, k)
    # mij / flip are optional: the call gets as far as the workspace check
    assert _call(L, lib, ws_bytes=16) == L.ERR_WORKSPACE
    # a frame that can hold no point needs no entry arrays, but its count
    assert _call(L, lib, _with(1, cell=None, pix=None, val=None), maxp=0, pts=None, vox=None,
                 ws_bytes=16) == L.ERR_WORKSPACE
    assert _call(L, lib, _with(1, frame_nnz=None), maxp=0) == L.ERR_ARG
    # shpl_build_index's own pointers, and its order: pointers before shapes
    assert _call(L, lib, n_frames=0) == L.ERR_ARG
    assert _call(L, lib, off=None) == L.ERR_ARG
    assert _call(L, lib, Pm=None) == L.ERR_ARG
    assert _call(L, lib, ws=None) == L.ERR_ARG
    assert _call(L, lib, pts=None) == L.ERR_ARG
    assert _call(L, lib, vox=None) == L.ERR_ARG
    assert _call(L, lib, levels=None, n_levels=9) == L.ERR_ARG
    assert _call(L, lib, _with(0, cell=None, s=(0., 0.))) == L.ERR_ARG
    assert _call(L, lib, _with(1, val=None), vstride=1) == L.ERR_ARG
    assert _call(L, lib, _with(0, pix=None), n_levels=7) == L.ERR_BAD_SHAPE  # the count, before levels[] is read
    # 3. the 2^31 bound on global ids, per level: 3834 frames x 700 x 800 cells pass, 3835 do not (stride 1);
    # the stride-8 level alone would pass either (8800 cells, 155 x 46 pixels)
    small_img = (100., 100.)
    assert _call(L, lib, n_frames=3834, im=small_img, ws_bytes=16) == L.ERR_WORKSPACE  # in bounds: the next check
    assert _call(L, lib, n_frames=3835, im=small_img, ws_bytes=16) == L.ERR_BAD_SHAPE
    assert _call(L, lib, AVOD[1:], n_frames=3835, im=small_img, ws_bytes=16) == L.ERR_WORKSPACE
    assert _call(L, lib, AVOD[::-1], n_frames=3835, im=small_img, ws_bytes=16) == L.ERR_BAD_SHAPE  # whichever level
    px = [dict(s=(1., 8.), bv=(704., 800.))]  # 8800 cells, 1242 x 375 pixels: 4611 frames are past 2^31 pixel ids
    assert _call(L, lib, px, n_frames=4610, ws_bytes=16) == L.ERR_WORKSPACE
    assert _call(L, lib, px, n_frames=4611, ws_bytes=16) == L.ERR_BAD_SHAPE
    # 4. then the workspace, then the type codes
    need = L.index_levels_ws_bytes(64, 100000, 2)
    assert _call(L, lib, n_frames=64, maxp=100000, ws_bytes=need - 1) == L.ERR_WORKSPACE
    assert _call(L, lib, pdt=7) == L.ERR_ARG and _call(L, lib, vit=7) == L.ERR_ARG


def test_levels_workspace_query():
    L, lib = _lib()
    nb = ctypes.c_size_t()
    q = lib.shpl_build_index_levels_workspace_bytes
    # one level: shpl_build_index's workspace
    for frames, maxp in ((1, 0), (1, 20000), (64, 20000), (4, 1025)):
        assert L.index_levels_ws_bytes(frames, maxp, 1) == L.index_ws_bytes(frames, maxp)
    # four levels: the head, then 1 + 4 count planes of frames x chunks i32 (256-byte granules)
    chunks = (20000 + 1023) // 1024
    assert L.index_levels_ws_bytes(64, 20000, 4) == 256 + -(-(5 * 4 * 64 * chunks) // 256) * 256
    assert L.index_levels_ws_bytes(64, 20000, 4) > L.index_levels_ws_bytes(64, 20000, 1)
    assert L.index_levels_ws_bytes(64, 20000, 2) == L.index_ws_bytes(64, 20000)  # 1 + 2 planes: the flat builder's 3
    assert q(1, 10, 0, ctypes.byref(nb)) == L.ERR_BAD_SHAPE
    assert q(1, 10, L.MAX_INDEX_LEVELS + 1, ctypes.byref(nb)) == L.ERR_BAD_SHAPE
    assert q(0, 10, 2, ctypes.byref(nb)) == L.ERR_ARG
    assert q(1, -1, 2, ctypes.byref(nb)) == L.ERR_ARG
    assert q(1, 10, 2, None) == L.ERR_ARG


def test_index_levels_helper_layout():
    """_lib.index_levels: the host array of shpl_index_level from (stride, bv_size, tensors...)."""
    import torch
    L, _ = _lib()
    cell, pix = torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    val, nnz = torch.zeros(4), torch.zeros(1, dtype=torch.int64)
    arr = L.index_levels([((1, 1), (700, 800), cell, pix, val, None, None, nnz),
                          ((8, 4), (704, 800), cell, pix, val, nnz, nnz, nnz)])
    assert len(arr) == 2
    assert (arr[0].s_img, arr[0].s_bv, arr[0].bv_h, arr[0].bv_w) == (1., 1., 700., 800.)
    assert (arr[1].s_img, arr[1].s_bv, arr[1].bv_h, arr[1].bv_w) == (8., 4., 704., 800.)
    assert arr[0].cell == cell.data_ptr() and arr[0].pix == pix.data_ptr() and arr[0].val == val.data_ptr()
    assert arr[0].mij is None and arr[0].flip is None and arr[1].mij == nnz.data_ptr()
    assert arr[0].frame_nnz == nnz.data_ptr()


# The SHPL switches of the reference's configs (avod/avod/configs), restated: what each implies for the dataset's
# sparse_pooling_input list.
def _rpn(full, vgg, indices=True):
    return f"""
model_config {{ model_name: 'avod_model'
    rpn_config {{ rpn_use_sparse_pooling: {full} rpn_sparse_pooling_use_batch_norm: False
                 rpn_sparse_pooling_conv_after_fusion: True rpn_sparse_pooling_after_vgg: {vgg}
                 rpn_dual_sparse_pooling_after_vgg: {vgg} }} }}
dataset_config {{ output_indices: {indices} }}
"""


def _retina(on, level):
    return f"""
model_config {{ model_name: 'retinanet_model'
    retinanet_config {{ use_sparse_pooling: {on} use_pyramid_level_at_SHPL: 'P2' }} }}
dataset_config {{ output_indices: True use_pyramid_level_at_SHPL: '{level}' }}
"""


@pytest.mark.parametrize("text, want", [
    (_rpn(True, False), [((1, 1), (700, 800))]),                           # fpn_people_dual_NHSP_train.config
    (_rpn(True, True), [((1, 1), (700, 800)), ((8, 8), (704, 800))]),      # fpn_people_dual_2NHSP_train.config
    (_rpn(False, True), [((1, 1), (700, 800)), ((8, 8), (704, 800))]),     # fpn_people_dual_SHPL.config: entry [1]
    (_rpn(False, False), []),
    (_rpn(True, True, indices=False), []),                                 # no indices from the dataset: no SHPL
    (_retina(True, "P2"), [((4, 4), (700, 800))]),                         # retinanet_car_SHPL.config
    (_retina(True, "P5"), [((32, 32), (700, 800))]),
    (_retina(False, "P2"), []),                                            # r3det_car.config
])
def test_fusion_levels_of_the_reference_configs(text, want):
    from sparse_pooling_amd import config as C
    assert C.fusion_levels(C.load_shpl_config(text), (700, 800)) == want


def test_fusion_levels_feed_the_after_vgg_entry():
    """The list built over fusion_levels has the entry fill_sparse_pooling_feed reads as [1]."""
    import numpy as np
    from sparse_pooling_amd import config as C
    levels = C.fusion_levels(C.load_shpl_config(_rpn(True, True)), (700, 800))
    sps = [{"M_val": np.ones(1), "Mij_pool": np.zeros((1, 2), np.int64), "M_size": np.array([int(b[0] // s[1]) *
                                                                                            int(b[1] // s[1]), 1]),
            "img_index_flip_pool": np.zeros((1, 3), np.int64), "bev_index_flip_pool": np.zeros((0, 3))}
           for s, b in levels]
    feed = C.fill_sparse_pooling_feed({}, sps, True, after_vgg=True, use_after_vgg=True)
    assert feed[C.PL_M_SIZE][0] == 700 * 800 and feed[C.PL_M_SIZE_VGG][0] == 88 * 100
