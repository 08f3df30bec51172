"""Philox4x32-10 in numpy, written from the published algorithm (Salmon, Moraes, Dror, Shaw: "Parallel random numbers:
as easy as 1, 2, 3", SC'11, section 3.3 and table 2), not from the library's sources: the tests pin the library's two
device copies (csrc/philox.h, csrc/train_kernels.hip) to it, and tests/test_philox_ref.py pins it to the Random123
known-answer vectors.

One round maps the counter (c0, c1, c2, c3) under the round key (k0, k1) to
    (hi(M1 * c2) ^ c1 ^ k0,  lo(M1 * c2),  hi(M0 * c0) ^ c3 ^ k1,  lo(M0 * c0))
with 32x32 -> 64 bit products; between rounds the key is bumped by the Weyl constants (W0, W1)."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter (N, 4), key (2,) or (N, 2): unsigned 32-bit words (any integer dtype).  Returns (N, 4) uint32."""
    c = np.asarray(counter, dtype=np.uint64).reshape(-1, 4) & MASK
    k = np.broadcast_to(np.asarray(key, dtype=np.uint64).reshape(-1, 2) & MASK, (c.shape[0], 2))
    c0, c1, c2, c3 = (c[:, j].copy() for j in range(4))
    k0, k1 = k[:, 0].copy(), k[:, 1].copy()
    for _ in range(10):
        p0 = np.uint64(M0) * c0  # < 2^64: no wrap
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK
        k0 = (k0 + np.uint64(W0)) & MASK
        k1 = (k1 + np.uint64(W1)) & MASK
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


def words(x):
    """(low, high) 32-bit words of an unsigned 64-bit value."""
    x = int(x) & 0xFFFFFFFFFFFFFFFF
    return x & 0xFFFFFFFF, x >> 32


def stream(seed, second, first_index, n4):
    """The 4 * n4 words of the library's streams: counter = (index lo, index hi, second lo, second hi) for index =
    first_index .. first_index + n4 - 1, key = (seed lo, seed hi).  `second` is the draw number of dm_randn, the
    (call << 16) | (block + 1) stream of the dropout masks."""
    idx = np.uint64(first_index) + np.arange(n4, dtype=np.uint64)
    ctr = np.empty((n4, 4), dtype=np.uint64)
    ctr[:, 0], ctr[:, 1] = idx & MASK, idx >> np.uint64(32)
    ctr[:, 2], ctr[:, 3] = words(second)
    return philox4x32_10(ctr, words(seed))
