"""The hand-made grouped map (tests/grouped_map.py) does separate TF's BEV->image pooling order from a plain
per-pixel sum, on the CPU oracle: the precondition that keeps the image-side conv's GPU tests
(tests/test_gpu_conv_img.py) from passing with either order."""
import numpy as np

import grouped_map as gm
from oracle import shpl_oracle as orc


def test_planted_pixels_separate_the_two_orders():
    m = gm.make()
    C = 8
    _, bev = gm.features(4, C)
    scale = gm.channel_scale(C)
    got = orc.sparse_pool_trans_op(m["mij"], m["mval"], m["m_size"], bev.reshape(-1, C), m["idx"], m["img_shape"])
    plain = gm.plain_sum(m, bev)
    assert len(m["planted"]) >= 3 and {x for _, x in m["planted"]} >= {0, 32, 39}
    for y, x in m["planted"]:
        np.testing.assert_array_equal(got[0, y, x], 2.0 * scale)  # 0 + 2^24 s + (s + s) - 2^24 s
        np.testing.assert_array_equal(plain[0, y, x], np.zeros(C, np.float32))  # ((2^24 s + s) + s) - 2^24 s
    # everywhere else the two orders agree to rounding: the plants alone carry the difference
    mask = np.ones(got.shape[1:3], bool)
    for y, x in m["planted"]:
        mask[y, x] = False
    np.testing.assert_allclose(got[0][mask], plain[0][mask], rtol=1e-5, atol=1e-5)


def test_map_has_the_shapes_the_gpu_tests_rely_on():
    m = gm.make()
    H, W = gm.IMG_HW
    mij, idx = m["mij"], m["idx"]
    per_col = np.bincount(mij[:, 1], minlength=gm.N_COLS)
    assert set(per_col) == {0, 1, 2, 3}
    assert 50 <= gm.N_COLS <= 70 and 120 <= len(mij) <= 180
    assert len({(r, k) for r, k in mij}) < len(mij)  # duplicate (row, column) pairs
    used = idx[per_col > 0]
    pix = used[:, 1] * W + used[:, 2]
    assert (np.bincount(pix) > 1).any()  # several columns on one pixel
    assert {0, 31, 32, 39} <= set(used[:, 2]) and {0, H - 1} <= set(used[:, 1])
    live = m["mval"][np.isin(mij[:, 1], [k for ks in gm.PLANT_COLS for k in ks], invert=True)]
    assert (live >= 0.25).all() and (live < 2.0).all()
    img, bev = gm.features(4, 8)
    for a in (img, bev):
        assert not (a.view(np.uint32) & 0xFFFF).any()  # bf16-representable
    # no other column lands on a planted pixel
    for (y, x), ks in zip(gm.PLANTED, gm.PLANT_COLS):
        on = np.nonzero((idx[:, 1] == y) & (idx[:, 2] == x))[0]
        assert set(on) == set(ks)
