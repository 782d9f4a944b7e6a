"""The fork's one kernel wrapper: cache sequences duplicated inside a K/V cache that is in use (mh_kv_fork_rows in
include/midihip.h).  Reached as ``ops.kv_fork_rows`` (ops resolves the name on first use, like the pool and seeded forms, and for the
reason given there).  Raw device pointers on the current stream, ONE launch for every layer and for K and V, no torch math."""
from __future__ import annotations

import torch

from .ops import _p, _stream, dt, lib


def check_pairs(src, dst, lengths, B: int, Lmax: int) -> tuple:
    """the host copy of a fork's pairs: three sequences of one length n >= 1, ids inside [0, B), the dst ids distinct, no id on both
    sides (a chain 0 -> 1, 1 -> 2 has no defined order), 1 <= length <= Lmax; -> (src, dst, lengths) as lists of ints (ValueError
    otherwise)"""
    s, d, ln = [int(r) for r in src], [int(r) for r in dst], [int(n) for n in lengths]
    if not (len(s) == len(d) == len(ln)) or not s:
        raise ValueError(f"kv_fork_rows: {len(s)} sources, {len(d)} destinations and {len(ln)} lengths (one of each per pair, at "
                         f"least one pair)")
    if any(r < 0 or r >= B for r in s + d):
        raise ValueError(f"kv_fork_rows: a cache row outside [0, {B}): sources {s}, destinations {d}")
    if len(set(d)) != len(d):
        raise ValueError(f"kv_fork_rows: a destination row named twice: {d}")
    if set(s) & set(d):
        raise ValueError(f"kv_fork_rows: rows {sorted(set(s) & set(d))} are source and destination at once: sources {s}, "
                         f"destinations {d}")
    if any(n < 1 or n > Lmax for n in ln):
        raise ValueError(f"kv_fork_rows: a length outside [1, {Lmax}]: {ln}")
    return s, d, ln


def kv_fork_rows(kv_k, kv_v, src, dst, lengths, dev=None):
    """kv_k / kv_v: a whole cache [layers, B, H, Lmax, hd]; for pair p, positions [0, lengths[p]) of every (layer, head) of sequence
    src[p] go to the same place in sequence dst[p], and no other element is written.  ``src``, ``dst``, ``lengths``: the host copies,
    checked here (check_pairs) before the call; ``dev``: their device copy, int32 [3, n] (rows: src, dst, lengths), when the caller
    has uploaded one already, else it is made here."""
    assert kv_k.dim() == 5 and kv_v.shape == kv_k.shape and kv_k.is_contiguous() and kv_v.is_contiguous() and kv_k.dtype == kv_v.dtype
    layers, B, H, Lmax, hd = kv_k.shape
    s, d, ln = check_pairs(src, dst, lengths, B, Lmax)
    n = len(s)
    if dev is None:
        dev = torch.tensor([s, d, ln], dtype=torch.int32).to(kv_k.device)
    assert dev.dtype == torch.int32 and dev.shape == (3, n) and dev.is_contiguous() and dev.device == kv_k.device
    lib().call("mh_kv_fork_rows", _p(kv_k), _p(kv_v), _p(dev[0]), _p(dev[1]), _p(dev[2]), n, max(ln), layers, B, H, hd, Lmax,
               dt(kv_k), _stream())
