"""The fused sampler with a seed per row: the wrappers of mh_sample_top_p_k_seeded and mh_sample_noise_seeded (include/midihip.h).
Reached as ``ops.sample_top_p_k_seeded`` / ``ops.sample_noise_seeded`` (ops resolves the names on first use, as it does
ops_rows', and for the same reason; the stand-ins are in tests/emu_seeded.py)."""
from __future__ import annotations

import torch

from .ops import _p, _rowmajor, _stream, dt, lib
from .ops_rows import mask_stride

NOISE_LANES = 64  # ranks per row that mh_sample_noise_seeded writes (= SAMPLE_MAX_K)


def _check_seed_ctr(seed, ctr, B: int, what: str) -> None:
    assert isinstance(seed, torch.Tensor) and seed.dtype == torch.int64 and seed.shape == (B,) and seed.is_contiguous(), \
        f"{what}: seed must be a contiguous int64 tensor of shape ({B},) (the storage of the 64 seed bits)"
    assert isinstance(ctr, torch.Tensor) and ctr.dtype == torch.int32 and ctr.shape == (B,) and ctr.is_contiguous(), \
        f"{what}: ctr must be a contiguous int32 tensor of shape ({B},)"


def sample_top_p_k_seeded(logits, first_mask, lo_tab, hi_tab, ev, pos: int, seed, ctr, out, V: int, temp, top_p, top_k, ban_mask,
                          out_b=None, out_c=None, first_span=(0, 0), max_range: int = 0, fill_rest: int = 0, fill_id: int = 0):
    """ops.sample_top_p_k_rows with row b's Exp(1) variates computed in the kernel from (seed[b], ctr[b], pos, rank) instead of
    read from a ``q``: ``seed`` is int64 [B] holding the 64 bits of row b's seed (a Python int s in [0, 2^64) is stored as
    s - 2^64 when s >= 2^63), ``ctr`` int32 [B] the index of the event being sampled in row b's result.  Both are read on the
    device, so a captured launch follows what they hold at replay time."""
    B = logits.shape[0]
    assert out.dtype == torch.int64
    assert lo_tab.dtype == torch.int32 and lo_tab.is_contiguous() and hi_tab.is_contiguous() and ev.dtype == torch.int64
    for t in (out_b, out_c):
        assert t is None or (t.dtype == torch.int64 and t.is_contiguous() and t.numel() == B)
    for t, ty, name in ((temp, torch.float32, "temp"), (top_p, torch.float32, "top_p"), (top_k, torch.int32, "top_k")):
        assert isinstance(t, torch.Tensor) and t.dtype == ty and t.shape == (B,) and t.is_contiguous(), \
            f"sample_top_p_k_seeded: {name} must be a contiguous {ty} tensor of shape ({B},)"
    _check_seed_ctr(seed, ctr, B, "sample_top_p_k_seeded")
    fs = mask_stride(first_mask, B, V, "sample_top_p_k_seeded: first_mask")
    bs = mask_stride(ban_mask, B, V, "sample_top_p_k_seeded: ban_mask")
    lib().call("mh_sample_top_p_k_seeded", _p(logits), _rowmajor(logits), _p(first_mask), fs, _p(ban_mask), bs, int(first_span[0]),
               int(first_span[1]), _p(lo_tab), _p(hi_tab), lo_tab.shape[1], int(max_range), _p(ev), pos, _p(seed), _p(ctr), _p(out),
               out.stride(0), _p(out_b), _p(out_c), B, V, _p(temp), _p(top_p), _p(top_k), fill_rest, fill_id, dt(logits), _stream())
    return out


def sample_noise_seeded(seed, ctr, pos: int, bits=None, q=None):
    """-> (bits int32 [B, 64] holding the uint32 Philox words, q float32 [B, 64]): what the seeded sampler computes for the 64
    ranks of every row at token position ``pos`` -- the same device function"""
    B = seed.shape[0]
    _check_seed_ctr(seed, ctr, B, "sample_noise_seeded")
    if bits is None:
        bits = torch.empty((B, NOISE_LANES), dtype=torch.int32, device=seed.device)
    if q is None:
        q = torch.empty((B, NOISE_LANES), dtype=torch.float32, device=seed.device)
    assert bits.dtype == torch.int32 and bits.shape == (B, NOISE_LANES) and bits.is_contiguous()
    assert q.dtype == torch.float32 and q.shape == (B, NOISE_LANES) and q.is_contiguous()
    lib().call("mh_sample_noise_seeded", _p(seed), _p(ctr), int(pos), B, _p(bits), _p(q), _stream())
    return bits, q


def seed_storage(seeds) -> list:
    """Python ints in [0, 2^64) -> the int64 values with the same 64 bits"""
    return [s - (1 << 64) if s >= (1 << 63) else s for s in (int(x) for x in seeds)]
