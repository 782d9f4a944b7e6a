"""Lookahead decoding's two kernel wrappers: the per-row K/V append and decode attention THROUGH A ROW MAP (mh_kv_append_rows_via,
mh_attn_decode_rows_via in include/midihip.h).  Reached as ``ops.kv_append_rows_via`` / ``ops.attn_decode_rows_via`` (ops
resolves the names on first use, like the other side-cars and for the reason given there).  Raw device pointers on the current
stream, no torch math."""
from __future__ import annotations

import torch

from .ops import _p, _stream, dt, lib


def _via_check(qkv, kc, vc, B: int, H: int, hd: int, Lmax: int, row_pos, row_cache) -> int:
    """the shapes the entry points cannot see; -> the number of cache sequences"""
    for name, t in (("row_pos", row_pos), ("row_cache", row_cache)):
        if t is None or t.dtype != torch.int32 or t.shape != (B,) or not t.is_contiguous() or t.device != qkv.device:
            raise ValueError(f"{name}: one device int32 per row ([{B}], contiguous, on {qkv.device}): "
                             + ("None" if t is None else f"{t.dtype} {tuple(t.shape)} on {t.device}"))
    if kc.dim() != 4 or kc.shape[1:] != (H, Lmax, hd) or vc.shape != kc.shape or kc.dtype != qkv.dtype or vc.dtype != qkv.dtype \
            or not kc.is_contiguous() or not vc.is_contiguous():
        raise ValueError(f"a cache of whole sequences [n, {H}, {Lmax}, {hd}] of {qkv.dtype}, K and V alike: {tuple(kc.shape)} "
                         f"{kc.dtype}, {tuple(vc.shape)} {vc.dtype}")
    if qkv.shape != (B, 3 * H * hd) or not qkv.is_contiguous():
        raise ValueError(f"qkv [{B}, {3 * H * hd}], contiguous: {tuple(qkv.shape)}")
    return int(kc.shape[0])


def kv_append_rows_via(qkv, cos_t, sin_t, kc, vc, B: int, H: int, hd: int, Lmax: int, row_pos, row_cache):
    """kv_append_rows with row b stored into cache sequence row_cache[b] (int32 [B] on the device; outside [0, kc.shape[0]): the row
    is inactive and writes nothing); kc / vc [n, H, Lmax, hd]"""
    n = _via_check(qkv, kc, vc, B, H, hd, Lmax, row_pos, row_cache)
    lib().call("mh_kv_append_rows_via", _p(qkv), _p(cos_t), _p(sin_t), _p(kc), _p(vc), B, H, hd, Lmax, _p(row_pos), _p(row_cache), n,
               dt(qkv), _stream())


def attn_decode_rows_via(qkv, kc, vc, o, B: int, H: int, hd: int, Lmax: int, scale: float, row_pos, row_cache):
    """attn_decode_rows with row b attending to rows [0, row_pos[b]] of cache sequence row_cache[b]; an inactive row's o is zeros"""
    n = _via_check(qkv, kc, vc, B, H, hd, Lmax, row_pos, row_cache)
    if o.shape != (B, H * hd) or o.dtype != qkv.dtype or not o.is_contiguous():
        raise ValueError(f"o [{B}, {H * hd}] of {qkv.dtype}, contiguous: {tuple(o.shape)} {o.dtype}")
    lib().call("mh_attn_decode_rows_via", _p(qkv), _p(kc), _p(vc), _p(o), B, H, hd, Lmax, scale, _p(row_pos), _p(row_cache), n,
               dt(qkv), _stream())
    return o
