"""The fused sampler with a parameter set per row: the wrapper of mh_sample_top_p_k_rows (include/midihip.h).  Reached as
``ops.sample_top_p_k_rows`` (ops resolves the name on first use, as it does the packed and the wide entry points, and for the same
reason: the CPU emulation of the test suite wants a stand-in of its own for every plain function of ops.py; the stand-in of this one
is in tests/emu_rowparams.py)."""
from __future__ import annotations

import torch

from .ops import _p, _rowmajor, _stream, dt, lib


def mask_stride(mask: torch.Tensor, B: int, V: int, what: str) -> int:
    """byte stride between the rows of a uint8 mask [V] (0: one mask for all rows) or [B, V]"""
    assert mask.dtype == torch.uint8 and mask.is_contiguous(), f"{what}: a contiguous uint8 mask is needed"
    assert mask.shape in ((V,), (B, V)), f"{what}: shape {tuple(mask.shape)}, ({V},) or ({B}, {V}) is needed"
    return 0 if mask.dim() == 1 else V


def sample_top_p_k_rows(logits, first_mask, lo_tab, hi_tab, ev, pos: int, q, out, V: int, temp, top_p, top_k, ban_mask,
                        out_b=None, out_c=None, first_span=(0, 0), max_range: int = 0, fill_rest: int = 0, fill_id: int = 0):
    """ops.sample_top_p_k with row b's own temp[b], top_p[b] (float32 [B]), top_k[b] (int32 [B]) and masks: first_mask / ban_mask
    are uint8 [V] (every row's) or [B, V] (row b's).  The three arrays are read on the device, so a captured launch follows what
    they hold at replay time.  first_span must cover every row's first mask.  The values are the caller's to validate (temp > 0,
    1 <= top_k <= min(SAMPLE_MAX_K, V)); the kernel clamps top_k into that range."""
    B = logits.shape[0]
    assert q.dtype == torch.float32 and q.is_contiguous() and q.shape == (B, V) and out.dtype == torch.int64
    assert lo_tab.dtype == torch.int32 and lo_tab.is_contiguous() and hi_tab.is_contiguous() and ev.dtype == torch.int64
    for t in (out_b, out_c):
        assert t is None or (t.dtype == torch.int64 and t.is_contiguous() and t.numel() == B)
    for t, ty, name in ((temp, torch.float32, "temp"), (top_p, torch.float32, "top_p"), (top_k, torch.int32, "top_k")):
        assert isinstance(t, torch.Tensor) and t.dtype == ty and t.shape == (B,) and t.is_contiguous(), \
            f"sample_top_p_k_rows: {name} must be a contiguous {ty} tensor of shape ({B},)"
    fs = mask_stride(first_mask, B, V, "sample_top_p_k_rows: first_mask")
    bs = mask_stride(ban_mask, B, V, "sample_top_p_k_rows: ban_mask")
    lib().call("mh_sample_top_p_k_rows", _p(logits), _rowmajor(logits), _p(first_mask), fs, _p(ban_mask), bs, int(first_span[0]),
               int(first_span[1]), _p(lo_tab), _p(hi_tab), lo_tab.shape[1], int(max_range), _p(ev), pos, _p(q), _p(out),
               out.stride(0), _p(out_b), _p(out_c), B, V, _p(temp), _p(top_p), _p(top_k), fill_rest, fill_id, dt(logits), _stream())
    return out
