"""CPU stand-ins for mh_kv_append_rows_via and mh_attn_decode_rows_via (ops.kv_append_rows_via / ops.attn_decode_rows_via), in the
style of emu_ragged.py: restatements from the definitions -- row b at position row_pos[b] of cache sequence row_cache[b], an inactive
row (row_cache outside [0, n)) writing nothing and getting zeros -- with the argument checks of the entry points and of the
wrappers.  ``install()`` is emu_fork.install() (and with it the seeded, pool and row-parameter stand-ins) with these two patched on
top; it yields the same CALL LOG, in which the stand-ins appear under their own names.  Test infrastructure only."""
from __future__ import annotations

import contextlib

import torch

import emu_fork
import emu_ragged
from emu_shared import rotated


def _check(name, qkv, kc, vc, B, H, hd, Lmax, row_pos, row_cache):
    if hd != 64:
        raise RuntimeError(f"{name}: head_dim {hd} unsupported (64)")
    if row_pos is None:
        raise RuntimeError(f"{name}: row_pos is NULL")
    if row_cache is None:
        raise RuntimeError(f"{name}: row_cache is NULL")
    assert row_pos.dtype == torch.int32 and row_pos.shape == (B,) and qkv.shape == (B, 3 * H * hd)
    assert row_cache.dtype == torch.int32 and row_cache.shape == (B,)
    assert kc.dim() == 4 and kc.shape[1:] == (H, Lmax, hd) and vc.shape == kc.shape and 0 < kc.shape[0] < 65536
    return [int(p) for p in row_pos.tolist()], [int(c) for c in row_cache.tolist()], kc.shape[0]


def kv_append_rows_via(qkv, cos_t, sin_t, kc, vc, B, H, hd, Lmax, row_pos, row_cache):
    D = H * hd
    pos, cache, n = _check("kv_append_rows_via", qkv, kc, vc, B, H, hd, Lmax, row_pos, row_cache)
    for b, (p, c) in enumerate(zip(pos, cache)):
        if not 0 <= c < n or not 0 <= p < Lmax:  # (the kernel writes nothing for such a row)
            continue
        q, k, v = rotated(qkv[b:b + 1], cos_t, sin_t, p, H, hd)
        qkv[b, :D] = q.reshape(D)
        qkv[b, D:2 * D] = k.reshape(D)
        kc[c, :, p] = k[0]
        vc[c, :, p] = v[0]


def attn_decode_rows_via(qkv, kc, vc, o, B, H, hd, Lmax, scale, row_pos, row_cache):
    pos, cache, n = _check("attn_decode_rows_via", qkv, kc, vc, B, H, hd, Lmax, row_pos, row_cache)
    for b, (p, c) in enumerate(zip(pos, cache)):
        if not 0 <= c < n:
            o[b] = 0
            continue
        rows = min(max(p + 1, 1), Lmax)
        o[b] = emu_ragged._attend(qkv[b, :H * hd].view(H, hd), kc[c], vc[c], rows, scale, o.dtype)
    return o


_NAMES = ("kv_append_rows_via", "attn_decode_rows_via")


@contextlib.contextmanager
def install():
    """emu_fork.install() + the stand-ins above (logged like every other op); yields the call log"""
    import midi_model_amd.ops as real
    with emu_fork.install() as log:
        try:
            for n in _NAMES:
                setattr(real, n, emu_ragged._logged(n, globals()[n], log))
            yield log
        finally:
            for n in _NAMES:
                delattr(real, n)
