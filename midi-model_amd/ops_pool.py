"""The decode pool's one kernel wrapper: the packed K/V store into CHOSEN rows of a cache that is in use (mh_kv_store_seqs_rows in
include/midihip.h).  Reached as ``ops.kv_store_seqs_rows`` (ops resolves the name on first use, like the packed, wide and row
forms, and for the reason given there).  Raw device pointers on the current stream, one launch, no torch math."""
from __future__ import annotations

import torch

from .ops import _p, _stream, dt, lib


def check_rows(rows, n: int, B: int) -> list:
    """the host copy of an admission's cache rows: n distinct ints inside [0, B); -> them as a list (ValueError otherwise)"""
    ids = [int(r) for r in rows]
    if len(ids) != n:
        raise ValueError(f"kv_store_seqs_rows: {len(ids)} cache rows for {n} sequences")
    if any(r < 0 or r >= B for r in ids):
        raise ValueError(f"kv_store_seqs_rows: a cache row outside [0, {B}): {ids}")
    if len(set(ids)) != n:
        raise ValueError(f"kv_store_seqs_rows: a cache row named twice: {ids}")
    return ids


def kv_store_seqs_rows(qkv, plan, rows, kc, vc, H: int, hd: int, Lmax: int, rows_dev=None):
    """kv_store_seqs with sequence s of ``plan`` going to cache sequence rows[s]: kc / vc [B, H, Lmax, hd], B >= plan.n, and no
    other cache element is written.  ``rows``: the host copy (a sequence of ints), checked here -- distinct, inside [0, B) -- with
    the plan's lengths, before the call; ``rows_dev``: its device copy (int32 [n]) when the caller has one already (one upload for
    all layers), else it is made here."""
    assert plan.dev is not None, "SeqPlan.upload(device) first"
    assert qkv.shape == (plan.M, 3 * H * hd) and qkv.is_contiguous()
    B = kc.shape[0]
    assert kc.shape == (B, H, Lmax, hd) and vc.shape == kc.shape and kc.is_contiguous() and vc.is_contiguous()
    ids = check_rows(rows, plan.n, B)
    if plan.max_len > Lmax:
        raise ValueError(f"kv_store_seqs_rows: a sequence of {plan.max_len} rows in a cache of {Lmax}")
    if rows_dev is None:
        rows_dev = torch.tensor(ids, dtype=torch.int32).to(qkv.device)
    assert rows_dev.dtype == torch.int32 and rows_dev.shape == (plan.n,) and rows_dev.is_contiguous() and rows_dev.device == qkv.device
    lib().call("mh_kv_store_seqs_rows", _p(qkv), _p(plan.seq_start), _p(rows_dev), _p(kc), _p(vc), plan.n, B, plan.M, H, hd, Lmax,
               dt(qkv), _stream())
