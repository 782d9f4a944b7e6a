"""The three kernel wrappers of the 8-bit event-level K/V cache (attention_kvq.hip; mh_kv_store_seqs_rows_fp8,
mh_attn_decode_append_rows_fp8 and mh_kv_fork_rows_fp8 in include/midihip.h, which states the format).  Reached as
``ops.kv_store_seqs_rows_fp8``, ``ops.attn_decode_append_rows_fp8`` and ``ops.kv_fork_rows_fp8`` (ops resolves the names on first use,
like the pool and fork forms, and for the reason given there; stand-ins in tests/emu_kvq.py).  Raw device pointers on the current
stream, one launch each, no torch math.  A layer's cache is k8 / v8 uint8 [B, H, Lmax, 64] and sc float32 [B, H, Lmax, 2]."""
from __future__ import annotations

import torch

from .ops import _p, _stream, dt, lib
from .ops_fork import check_pairs
from .ops_pool import check_rows

HD = 64


def _check_cache(what: str, k8, v8, sc, lead: tuple):
    """k8 / v8 uint8 [*lead, H, Lmax, 64], sc float32 [*lead, H, Lmax, 2], contiguous, on one device; -> (H, Lmax)"""
    assert k8.dtype == torch.uint8 and v8.dtype == torch.uint8 and sc.dtype == torch.float32, f"{what}: uint8 codes and fp32 scales"
    assert k8.dim() == len(lead) + 3 and k8.shape[-1] == HD and tuple(k8.shape[:len(lead)]) == lead, f"{what}: k8 {tuple(k8.shape)}"
    assert v8.shape == k8.shape and tuple(sc.shape) == tuple(k8.shape[:-1]) + (2,), f"{what}: v8 {tuple(v8.shape)}, sc {tuple(sc.shape)}"
    assert k8.is_contiguous() and v8.is_contiguous() and sc.is_contiguous() and k8.device == v8.device == sc.device
    return k8.shape[-3], k8.shape[-2]


def kv_store_seqs_rows_fp8(qkv, plan, rows, k8, v8, sc, H: int, hd: int, Lmax: int, rows_dev=None):
    """ops.kv_store_seqs_rows into the fp8 cache of one layer: Q() of every K row (rotated, as ``qkv`` holds it) and V row of
    sequence s of ``plan`` goes to rows [0, L_s) of cache sequence rows[s], codes and scale pair; no other byte is written.  The
    host checks are that wrapper's (``ValueError`` before the call)."""
    assert plan.dev is not None, "SeqPlan.upload(device) first"
    assert hd == HD and qkv.dtype == torch.bfloat16, "kv_store_seqs_rows_fp8: bf16 activations, head_dim 64"
    assert qkv.shape == (plan.M, 3 * H * hd) and qkv.is_contiguous()
    B = k8.shape[0]
    assert _check_cache("kv_store_seqs_rows_fp8", k8, v8, sc, (B,)) == (H, Lmax)
    ids = check_rows(rows, plan.n, B)
    if plan.max_len > Lmax:
        raise ValueError(f"kv_store_seqs_rows_fp8: a sequence of {plan.max_len} rows in a cache of {Lmax}")
    if rows_dev is None:
        rows_dev = torch.tensor(ids, dtype=torch.int32).to(qkv.device)
    assert rows_dev.dtype == torch.int32 and rows_dev.shape == (plan.n,) and rows_dev.is_contiguous() and rows_dev.device == qkv.device
    lib().call("mh_kv_store_seqs_rows_fp8", _p(qkv), _p(plan.seq_start), _p(rows_dev), _p(k8), _p(v8), _p(sc), plan.n, B, plan.M, H,
               hd, Lmax, dt(qkv), _stream())


def attn_decode_append_rows_fp8(qkv, cos_t, sin_t, k8, v8, sc, o, B: int, H: int, hd: int, Lmax: int, scale: float, row_pos):
    """ops.attn_decode_append_rows over the fp8 cache of one layer (qkv is read unrotated and left untouched): the new row is
    quantized into cache row row_pos[b] and attended to as the cache holds it"""
    assert hd == HD and qkv.dtype == torch.bfloat16 and o.dtype == torch.bfloat16, "attn_decode_append_rows_fp8: bf16, head_dim 64"
    assert qkv.shape == (B, 3 * H * hd) and qkv.is_contiguous() and o.shape == (B, H * hd) and o.is_contiguous()
    assert row_pos is not None and row_pos.dtype == torch.int32 and row_pos.shape == (B,) and row_pos.is_contiguous()
    assert row_pos.device == qkv.device
    assert _check_cache("attn_decode_append_rows_fp8", k8, v8, sc, (B,)) == (H, Lmax)
    lib().call("mh_attn_decode_append_rows_fp8", _p(qkv), _p(cos_t), _p(sin_t), _p(k8), _p(v8), _p(sc), _p(o), B, H, hd, Lmax, scale,
               _p(row_pos), dt(qkv), _stream())
    return o


def kv_fork_rows_fp8(k8, v8, sc, src, dst, lengths, dev=None):
    """ops.kv_fork_rows over a whole fp8 cache (k8 / v8 [layers, B, H, Lmax, 64], sc [layers, B, H, Lmax, 2]): codes and scale pairs
    of positions [0, lengths[p]) of sequence src[p] into dst[p], bit for bit, ONE launch.  The host checks are that wrapper's."""
    assert k8.dim() == 5
    layers, B = k8.shape[:2]
    H, Lmax = _check_cache("kv_fork_rows_fp8", k8, v8, sc, (layers, B))
    s, d, ln = check_pairs(src, dst, lengths, B, Lmax)
    n = len(s)
    if dev is None:
        dev = torch.tensor([s, d, ln], dtype=torch.int32).to(k8.device)
    assert dev.dtype == torch.int32 and dev.shape == (3, n) and dev.is_contiguous() and dev.device == k8.device
    lib().call("mh_kv_fork_rows_fp8", _p(k8), _p(v8), _p(sc), _p(dev[0]), _p(dev[1]), _p(dev[2]), n, max(ln), layers, B, H, HD, Lmax,
               _stream())
