"""CPU stand-ins for the three entry points of the 8-bit K/V cache (ops.kv_store_seqs_rows_fp8, ops.attn_decode_append_rows_fp8,
ops.kv_fork_rows_fp8), in the style of emu_fork.py: restatements from the definition in ref_kvq.py -- Q() at the store and at the
append, attention in float64 over the exactly dequantized rows, rounded once -- with the checks of the wrappers.  ``install()`` is
emu_fork.install() with these patched on top; it yields the same CALL LOG, in which the stand-ins appear under their own names.  Test
infrastructure only."""
from __future__ import annotations

import contextlib

import torch

import emu_fork
import emu_pool
import emu_ragged
import ref_kvq
from emu_shared import rotated


def _cache(k8, v8, sc, lead):
    assert k8.dtype == torch.uint8 and v8.dtype == torch.uint8 and sc.dtype == torch.float32
    assert k8.shape[-1] == 64 and v8.shape == k8.shape and tuple(sc.shape) == tuple(k8.shape[:-1]) + (2,)
    assert tuple(k8.shape[:len(lead)]) == tuple(lead) and k8.is_contiguous() and v8.is_contiguous() and sc.is_contiguous()


def kv_store_seqs_rows_fp8(qkv, plan, rows, k8, v8, sc, H, hd, Lmax, rows_dev=None):
    assert hd == 64 and qkv.dtype == torch.bfloat16
    B = k8.shape[0]
    _cache(k8, v8, sc, (B, H, Lmax))
    kc = torch.zeros((B, H, Lmax, hd), dtype=qkv.dtype)
    vc = torch.zeros_like(kc)
    emu_pool.kv_store_seqs_rows(qkv, plan, rows, kc, vc, H, hd, Lmax, rows_dev=rows_dev)  # (its checks, its ValueErrors)
    start = plan.host_views()[0].tolist()
    for s, (a, b) in enumerate(zip(start[:-1], start[1:])):
        r, n = int(rows[s]), b - a
        k8[r, :, :n], sc[r, :, :n, 0] = ref_kvq.quantize(kc[r, :, :n])
        v8[r, :, :n], sc[r, :, :n, 1] = ref_kvq.quantize(vc[r, :, :n])


def attn_decode_append_rows_fp8(qkv, cos_t, sin_t, k8, v8, sc, o, B, H, hd, Lmax, scale, row_pos):
    assert qkv.dtype == torch.bfloat16 and o.dtype == torch.bfloat16
    _cache(k8, v8, sc, (B, H, Lmax))
    for b, pos in enumerate(emu_ragged._check("attn_decode_append_rows_fp8", qkv, B, H, hd, Lmax, row_pos)):
        pos = min(max(pos, 0), Lmax - 1)  # (the kernel clamps the row count to [1, Lmax])
        q, k, v = rotated(qkv[b:b + 1], cos_t, sin_t, pos, H, hd)
        k8[b, :, pos], sc[b, :, pos, 0] = ref_kvq.quantize(k[0])
        v8[b, :, pos], sc[b, :, pos, 1] = ref_kvq.quantize(v[0])
        for h in range(H):
            o[b, h * hd:(h + 1) * hd] = ref_kvq.attend64(q[0, h].double() * scale, k8[b, h], v8[b, h], sc[b, h], pos + 1).to(o.dtype)
    return o


def kv_fork_rows_fp8(k8, v8, sc, src, dst, lengths, dev=None):
    assert k8.dim() == 5
    _cache(k8, v8, sc, k8.shape[:4])
    emu_fork.kv_fork_rows(k8, v8, src, dst, lengths, dev=dev)  # (its checks, its ValueErrors; uint8 rows of 64)
    for a, b, n in zip(src, dst, lengths):
        sc[:, int(b), :, :int(n)] = sc[:, int(a), :, :int(n)]


_NAMES = ("kv_store_seqs_rows_fp8", "attn_decode_append_rows_fp8", "kv_fork_rows_fp8")


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
