"""The dropout mask of the heads (include/shpl.h), restated in numpy from its definition and independent of the
library: Philox4x32-10 and the (seed, row, channel, keep_prob) indexing. Shared by test_dropout_mask.py (CPU) and
test_gpu_head_dropout.py."""
import math

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Random123's Philox4x32-10 over arrays: counter = 4 uint32 arrays (or ints), key = 2; returns 4 uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(MASK32) for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]  # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(MASK32),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(MASK32)]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return [v.astype(np.uint32) for v in c]


def threshold(keep_prob):
    """T of the contract: clamp(floor(keep_prob * 65536 + 0.5), 1, 65536)."""
    return int(min(max(math.floor(float(keep_prob) * 65536.0 + 0.5), 1), 65536))


def scale(keep_prob):
    return float(np.float32(65536.0 / threshold(keep_prob)))


def mask(rows, channels, keep_prob, seed, row0=0):
    """uint8 [rows, channels]: 1 kept, 0 dropped, for the global rows row0 .. row0 + rows."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    r = (np.arange(rows, dtype=np.uint64) + np.uint64(row0)).reshape(-1, 1)
    groups = (channels + 7) // 8
    g = np.arange(groups, dtype=np.uint64).reshape(1, -1)
    w = philox4x32_10((r & np.uint64(MASK32), r >> np.uint64(32), g, 0), (seed & MASK32, seed >> 32))
    h = np.empty((rows, groups, 8), dtype=np.uint32)
    for j in range(8):
        h[:, :, j] = (w[j >> 1] >> np.uint32(16 * (j & 1))) & np.uint32(0xFFFF)
    return (h.reshape(rows, groups * 8)[:, :channels] < threshold(keep_prob)).astype(np.uint8)
