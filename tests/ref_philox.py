"""Philox4x32-10 in numpy (Salmon et al., SC'11; Random123's constants and round function) and the map from its word 0 to the
Exp(1) variate of the seeded sampler (include/midihip.h, mh_sample_top_p_k_seeded):

    counter = (uint32 ctr, uint32 pos, uint32 lane, 0)     key = (seed & 0xffffffff, seed >> 32)
    x = word 0 of Philox4x32-10(counter, key);  n = x >> 9;  u = (2 n + 1) 2^-24;  q = -log(u)

Pinned to Random123's known answers in test_seeded_host.py.  Test infrastructure only."""
from __future__ import annotations

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter [..., 4], key [..., 2] (anything numpy casts to uint32, broadcast against each other) -> uint32 [..., 4]"""
    c = np.asarray(counter, dtype=np.uint64) & MASK
    k = np.asarray(key, dtype=np.uint64) & MASK
    c0, c1, c2, c3 = np.broadcast_arrays(c[..., 0], c[..., 1], c[..., 2], c[..., 3], k[..., 0])[:4]
    k0, k1 = k[..., 0], k[..., 1]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2        # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def u_of_bits(x) -> np.ndarray:
    """the uniform of a word, exact in float64 (and in float32): (2 (x >> 9) + 1) 2^-24, in [2^-24, 1 - 2^-24]"""
    n = np.asarray(x, dtype=np.uint32) >> np.uint32(9)
    return (2.0 * n.astype(np.float64) + 1.0) * 2.0 ** -24


def q_of_bits(x) -> np.ndarray:
    """float64 -log(u): what the device's accurate logf approximates"""
    return -np.log(u_of_bits(x))


def noise(seed, ctr, pos: int, lanes: int = 64):
    """seed: B ints in [0, 2^64) (or their int64 storage), ctr: B ints -> (bits uint32 [B, lanes], q float64 [B, lanes])"""
    seed = np.array([int(s) % (1 << 64) for s in np.asarray(seed, dtype=object).reshape(-1)], dtype=np.uint64)
    ctr = np.array([int(c) % (1 << 32) for c in np.asarray(ctr, dtype=object).reshape(-1)], dtype=np.uint64)
    B = seed.shape[0]
    assert ctr.shape == (B,)
    counter = np.zeros((B, lanes, 4), dtype=np.uint64)
    counter[..., 0] = ctr[:, None]
    counter[..., 1] = np.uint64(pos)
    counter[..., 2] = np.arange(lanes, dtype=np.uint64)[None, :]
    key = np.stack([seed & MASK, seed >> np.uint64(32)], axis=-1)[:, None, :]
    bits = philox4x32_10(counter, key)[..., 0]
    return bits, q_of_bits(bits)
