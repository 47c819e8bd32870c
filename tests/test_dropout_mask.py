"""The dropout mask's definition (include/shpl.h), restated in numpy (dropout_mask_ref.py) and held to the
published known answers of Philox4x32-10; the kept fraction of the restatement is Bernoulli(T / 65536). CPU only:
the library's mask is compared with this restatement bit for bit in test_gpu_head_dropout.py."""
import math

import numpy as np
import pytest

import dropout_mask_ref as ref

# counter, key, output (Random123's known-answer tests of philox4x32_10)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]

ROWS, CHANNELS = 126, 192
SEEDS = {0.5: 20261, 0.8: 8087}  # chosen on the CPU: the restatement alone meets the bound below


def test_philox_known_answers():
    for counter, key, out in KAT:
        got = tuple(int(v) for v in ref.philox4x32_10(counter, key))
        assert got == out, [hex(v) for v in got]
    # over arrays, the same words
    cs = [np.array([k[0][i] for k in KAT[:1] * 3], dtype=np.uint32) for i in range(4)]
    got = ref.philox4x32_10(cs, KAT[0][1])
    assert all(tuple(int(w[i]) for w in got) == KAT[0][2] for i in range(3))


def test_threshold_and_scale():
    assert ref.threshold(0.5) == 32768 and ref.scale(0.5) == 2.0
    assert ref.threshold(1.0) == 65536 and ref.scale(1.0) == 1.0
    assert ref.threshold(0.8) == 52429 and ref.scale(0.8) == float(np.float32(65536.0 / 52429))
    assert ref.threshold(1e-9) == 1  # clamped: never a mask that keeps nothing by construction
    assert ref.mask(5, 11, 1.0, 3).all()


def test_mask_indexing_follows_the_definition():
    """Element (r, c) by the scalar definition: group c >> 3, 16-bit field c & 7 of the four words."""
    seed, kp = 0x1234567890ABCDEF, 0.5
    m = ref.mask(9, 21, kp, seed, row0=(1 << 32) - 4)  # rows on both sides of the 32-bit carry
    T = ref.threshold(kp)
    for r in range(9):
        R = (1 << 32) - 4 + r
        for c in range(21):
            w = ref.philox4x32_10((R & 0xffffffff, R >> 32, c >> 3, 0), (seed & 0xffffffff, seed >> 32))
            j = c & 7
            h = (int(w[j >> 1]) >> (16 * (j & 1))) & 0xffff
            assert m[r, c] == (1 if h < T else 0), (r, c)
    # the mask of a row does not depend on how many rows or channels the call has
    assert np.array_equal(ref.mask(9, 21, kp, seed)[:4, :13], ref.mask(4, 13, kp, seed))


@pytest.mark.parametrize("kp", [0.5, 0.8])
def test_kept_fraction(kp):
    p = ref.threshold(kp) / 65536.0
    n = ROWS * CHANNELS
    m = ref.mask(ROWS, CHANNELS, kp, SEEDS[kp])
    frac = float(m.mean())
    bound = 4.0 * math.sqrt(p * (1.0 - p) / n)
    print(f"keep_prob {kp}: kept {frac:.5f}, T/65536 {p:.5f}, bound {bound:.5f}")
    assert abs(frac - p) <= bound
    # no row and no channel is all kept or all dropped at this size
    assert 0 < m.sum(0).min() and m.sum(0).max() < ROWS and 0 < m.sum(1).min() and m.sum(1).max() < CHANNELS


def test_seeds_differ():
    a, b = ref.mask(ROWS, CHANNELS, 0.5, 1), ref.mask(ROWS, CHANNELS, 0.5, 2)
    assert 0.4 < float((a != b).mean()) < 0.6
    assert not np.array_equal(ref.mask(ROWS, CHANNELS, 0.5, 1), ref.mask(ROWS, CHANNELS, 0.5, 1 + (1 << 32)))
