"""The prefix-slot wrappers: decode attention for a batch whose rows stand at positions of their own behind G prompts that rows may
SHARE (mh_attn_prefix_partial_slots, mh_attn_decode_append_rows_shared in include/midihip.h).  Reached as
``ops.attn_prefix_partial_slots`` / ``ops.attn_decode_append_rows_shared`` (ops resolves the names on first use, like the pool, seeded
and fork forms, and for the reason given there).  Raw device pointers on the current stream, one launch each, no torch math."""
from __future__ import annotations

from typing import NamedTuple

import torch

from .ops import _p, _stream, dt, lib

CHUNK = 256  # MH_ATTN_PREFIX_CHUNK


class SlotPrefix(NamedTuple):
    """the slots form of ``engine.stack_decode(shared=...)``, which goes with ``row_pos``: the slot caches (a KVState of G
    sequences of Pmax rows: ``kvs.k[layer]`` is [G, H, Pmax, hd]), ``slot_len`` (device int32 [G]; 0: an empty slot), ``row_slot``
    (device int32 [B]; -1: the row shares nothing) and the fp32 partials workspace, reused by every layer"""
    kvs: object
    slot_len: torch.Tensor
    row_slot: torch.Tensor
    workspace: torch.Tensor


def workspace_floats(B: int, H: int, Pmax: int) -> int:
    """acc [B, H, nch, 64] + (m, l) [B, H, nch, 2], nch = ceil(Pmax / CHUNK): the shape shared.py's workspace has"""
    return 66 * B * H * ((Pmax + CHUNK - 1) // CHUNK)


def _check(slot_len, row_slot, row_pos, B: int, G: int) -> None:
    for name, t, n in (("slot_len", slot_len, G), ("row_slot", row_slot, B), ("row_pos", row_pos, B)):
        assert t.dtype == torch.int32 and t.shape == (n,) and t.is_contiguous(), f"{name}: int32 [{n}] expected, {t.dtype} {tuple(t.shape)}"


def attn_prefix_partial_slots(qkv, cos_t, sin_t, kpre, vpre, slot_len, row_slot, row_pos, ws, B: int, H: int, hd: int, G: int,
                              Pmax: int, scale: float):
    """partials of the member rows of every slot against that slot's prefix rows [0, slot_len[g]) of kpre / vpre [G, H, Pmax, hd],
    row b rotated at row_pos[b] -> ws, at the index of (b, h, chunk)"""
    assert kpre.shape == (G, H, Pmax, hd) and vpre.shape == kpre.shape and kpre.is_contiguous() and vpre.is_contiguous()
    _check(slot_len, row_slot, row_pos, B, G)
    lib().call("mh_attn_prefix_partial_slots", _p(qkv), _p(cos_t), _p(sin_t), _p(kpre), _p(vpre), _p(slot_len), _p(row_slot),
               _p(row_pos), _p(ws), ws.numel(), B, H, hd, G, Pmax, scale, dt(qkv), _stream())
    return ws


def attn_decode_append_rows_shared(qkv, cos_t, sin_t, ksuf, vsuf, ws, o, B: int, H: int, hd: int, Lsuf: int, G: int, Pmax: int,
                                   scale: float, slot_len, row_slot, row_pos):
    """attn_decode_append_rows over the rows' own caches [B, H, Lsuf, hd], cache row j of row b being absolute position pre_b + j
    (pre_b = slot_len[row_slot[b]], 0 without a slot), + the merge of row b's ceil(pre_b / CHUNK) partials in ws"""
    assert ksuf.shape == (B, H, Lsuf, hd) and vsuf.shape == ksuf.shape and ksuf.is_contiguous() and vsuf.is_contiguous()
    _check(slot_len, row_slot, row_pos, B, G)
    lib().call("mh_attn_decode_append_rows_shared", _p(qkv), _p(cos_t), _p(sin_t), _p(ksuf), _p(vsuf), _p(ws), ws.numel(), _p(o), B,
               H, hd, Lsuf, G, Pmax, scale, _p(slot_len), _p(row_slot), _p(row_pos), dt(qkv), _stream())
    return o


def check_slots(slots, n: int, G: int) -> list:
    """the host copy of an admission's slots: n distinct ints inside [0, G); -> them as a list (ValueError otherwise)"""
    ids = [int(s) for s in slots]
    if len(ids) != n:
        raise ValueError(f"prefix slots: {len(ids)} slots for {n} sequences")
    if any(s < 0 or s >= G for s in ids):
        raise ValueError(f"prefix slots: a slot outside [0, {G}): {ids}")
    if len(set(ids)) != n:
        raise ValueError(f"prefix slots: a slot named twice: {ids}")
    return ids
