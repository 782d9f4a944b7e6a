"""CPU stand-ins for the four entry points of generate_ragged (mh_kv_append_rows, mh_attn_decode_rows, mh_attn_decode_append_rows,
mh_kv_store_seqs), in the style of emu_shared.py: restatements from the definitions -- row b at position row_pos[b] of its own
cache, attention in float64 rounded once -- with the argument checks of the entry points.  ``install()`` is the packed fake backend
(emu_packed.install()) with these four patched on top, and it yields the CALL LOG: the name of every backend call made while it is
installed (every ops stand-in is wrapped), which is how a test shows that a refusal came before any launch.  Test infrastructure
only."""
from __future__ import annotations

import contextlib
import functools

import torch

import emu_ops
import emu_packed
from emu_shared import rotated


def _check(name, qkv, B, H, hd, Lmax, row_pos):
    if hd != 64:
        raise RuntimeError(f"{name}: head_dim {hd} unsupported (64)")
    if row_pos is None:
        raise RuntimeError(f"{name}: row_pos is NULL")
    assert row_pos.dtype == torch.int32 and row_pos.shape == (B,) and qkv.shape == (B, 3 * H * hd)
    return [int(p) for p in row_pos.tolist()]


def kv_append_rows(qkv, cos_t, sin_t, kc, vc, B, H, hd, Lmax, row_pos):
    D = H * hd
    for b, pos in enumerate(_check("kv_append_rows", qkv, B, H, hd, Lmax, row_pos)):
        if not 0 <= pos < Lmax:  # (the kernel writes nothing for such a row)
            continue
        q, k, v = rotated(qkv[b:b + 1], cos_t, sin_t, pos, H, hd)
        qkv[b, :D] = q.reshape(D)
        qkv[b, D:2 * D] = k.reshape(D)
        kc[b, :, pos] = k[0]
        vc[b, :, pos] = v[0]


def _attend(q, kc_b, vc_b, n, scale, dtype):
    """q [H, hd] (rotated) over the first n rows of one sequence's cache [H, Lmax, hd] -> [H * hd]"""
    s = torch.einsum("hd,hkd->hk", q.double() * scale, kc_b[:, :n].double())
    return torch.einsum("hk,hkd->hd", torch.softmax(s, -1), vc_b[:, :n].double()).reshape(-1).to(dtype)


def attn_decode_rows(qkv, kc, vc, o, B, H, hd, Lmax, scale, row_pos):
    for b, pos in enumerate(_check("attn_decode_rows", qkv, B, H, hd, Lmax, row_pos)):
        n = min(max(pos + 1, 1), Lmax)
        o[b] = _attend(qkv[b, :H * hd].view(H, hd), kc[b], vc[b], n, scale, o.dtype)
    return o


def attn_decode_append_rows(qkv, cos_t, sin_t, kc, vc, o, B, H, hd, Lmax, scale, row_pos):
    for b, pos in enumerate(_check("attn_decode_append_rows", qkv, B, H, hd, Lmax, row_pos)):
        pos = min(max(pos, 0), Lmax - 1)  # (the kernel clamps the row count to [1, Lmax])
        q, k, v = rotated(qkv[b:b + 1], cos_t, sin_t, pos, H, hd)
        kc[b, :, pos] = k[0]
        vc[b, :, pos] = v[0]
        o[b] = _attend(q[0], kc[b], vc[b], pos + 1, scale, o.dtype)
    return o


def kv_store_seqs(qkv, plan, kc, vc, H, hd, Lmax):
    if plan.max_len > Lmax:
        raise ValueError(f"kv_store_seqs: a sequence of {plan.max_len} rows in a cache of {Lmax}")
    D = H * hd
    assert qkv.shape == (plan.M, 3 * D) and kc.shape[0] == plan.n and hd % 8 == 0
    start = plan.host_views()[0].tolist()
    for s, (a, b) in enumerate(zip(start[:-1], start[1:])):
        kc[s, :, :b - a] = qkv[a:b, D:2 * D].view(b - a, H, hd).transpose(0, 1)
        vc[s, :, :b - a] = qkv[a:b, 2 * D:].view(b - a, H, hd).transpose(0, 1)


_NAMES = ("kv_append_rows", "attn_decode_rows", "attn_decode_append_rows", "kv_store_seqs")
_HOST_ONLY = ("skinny_ok", "rope_fused_ok", "norm_fold_ok", "swiglu_fused_ok", "dswiglu_ok", "attn_bwd_scaled_ok", "mask_spans",
              "get_option", "set_option", "token_segments", "scale_cols_jobs")  # answer from shapes alone: no launch behind them


def _logged(name, fn, log):
    @functools.wraps(fn)
    def f(*a, **k):
        log.append(name)
        return fn(*a, **k)
    return f


@contextlib.contextmanager
def install():
    """emu_packed.install() + the four stand-ins above; yields the call log (a list of op names, in call order)"""
    import midi_model_amd.ops as real
    log: list = []
    with emu_packed.install():
        wrapped = {}
        try:
            for n in _NAMES:
                setattr(real, n, globals()[n])
            for n in list(emu_ops._NAMES) + list(emu_packed._NAMES) + list(_NAMES):
                if n in _HOST_ONLY or not hasattr(real, n) or not callable(getattr(real, n)) or isinstance(getattr(real, n), type):
                    continue
                wrapped[n] = getattr(real, n)
                setattr(real, n, _logged(n, wrapped[n], log))
            yield log
        finally:
            for n, fn in wrapped.items():
                setattr(real, n, fn)
            for n in _NAMES:
                delattr(real, n)
