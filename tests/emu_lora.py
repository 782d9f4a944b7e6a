"""CPU stand-ins for the entry points behind a LoRA adapter per decode row (ops.lora_shrink_rows, ops.gemm_skinny_ext,
ops.skinny_ext_ok), in the style of emu_kvq.py: restatements from the definition in include/midihip.h with the checks of the wrappers.
``install()`` is emu_kvq.install() with these patched on top; it yields the same CALL LOG, in which the stand-ins appear under their
own names.  Test infrastructure only."""
from __future__ import annotations

import contextlib

import torch

import emu_kvq
import emu_ops
import emu_ragged


def skinny_ext_ok(x, K, rows=None):
    M = x.shape[0] if rows is None else rows
    return x.dtype == torch.bfloat16 and 1 <= M <= 256 and K % 256 == 0


def lora_shrink_rows(a, a_stack, t, row_adapter, slot_scale, G, R, parts, row_ids=None):
    M, N = t.shape
    if a.dtype != torch.bfloat16 or not (1 <= M <= 256) or a_stack.shape[1] % 256 or R % 8 or N != parts * G * R or a_stack.shape[0] != N:
        raise ValueError("lora_shrink_rows: operands")
    assert row_adapter.dtype == torch.int32 and row_adapter.numel() == M and slot_scale.dtype == torch.float32 and slot_scale.numel() == G
    x = (a[row_ids] if row_ids is not None else a).float()
    slot = (torch.arange(N) // R) % G
    acc = slot_scale[slot][None, :] * (x @ a_stack.float().T)
    t.copy_(torch.where(row_adapter.long()[:, None] == slot[None, :], acc, torch.zeros(())).to(t.dtype))
    return t


def gemm_skinny_ext(a, w, out, t, b_stack, parts, *, mode=0, res=None, norm_eps=0.0, row_ids=None, res_ids=None):
    from midi_model_amd.ops_lora import check_parts
    M, N = out.shape
    K2 = b_stack.shape[1]
    if out.dtype != torch.bfloat16 or not (1 <= M <= 256) or w.shape[1] % 256 or K2 % 256:
        raise ValueError("gemm_skinny_ext: operands")
    check_parts(mode, N, parts)
    assert t.shape == (M, parts * K2) and b_stack.shape[0] == w.shape[0]
    x = (a[row_ids] if row_ids is not None else a).float()
    r = x @ w.float().T
    rpp = w.shape[0] // parts
    for p in range(parts):
        r[:, p * rpp:(p + 1) * rpp] += t[:, p * K2:(p + 1) * K2].float() @ b_stack[p * rpp:(p + 1) * rpp].float().T
    if norm_eps > 0:
        r = r * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + norm_eps)
    if mode == emu_ops.SKINNY_GATEUP:
        emu_ops.swiglu_fwd(r.to(a.dtype), out)
        return out
    if res is not None:
        r = r + (res[res_ids] if res_ids is not None else res).float()
    out.copy_(r.to(out.dtype))
    return out


_NAMES = ("skinny_ext_ok", "lora_shrink_rows", "gemm_skinny_ext")


@contextlib.contextmanager
def install():
    """emu_kvq.install() + the stand-ins above (the two launches logged like every other op); yields the call log"""
    import midi_model_amd.ops as real
    with emu_kvq.install() as log:
        try:
            setattr(real, "skinny_ext_ok", skinny_ext_ok)
            for n in _NAMES[1:]:
                setattr(real, n, emu_ragged._logged(n, globals()[n], log))
            yield log
        finally:
            for n in _NAMES:
                delattr(real, n)
