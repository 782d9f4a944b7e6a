"""CPU stand-in for mh_sample_top_p_k_rows (ops.sample_top_p_k_rows), in the style of emu_ragged.py: row b is
emu_ops.sample_top_p_k's chain -- masked softmax of logits / temp in the activation dtype, ban, stable descending sort, top-p cut,
top-k, renormalise, argmax(p / q) -- restated with row b's temp[b], top_p[b], top_k[b] and row b's two masks, plus the argument
checks of the entry point and of the wrapper.  ``install()`` is emu_ragged.install() with this one patched on top; it yields the
same CALL LOG, in which the stand-in appears under its own name.  Test infrastructure only."""
from __future__ import annotations

import contextlib

import torch

import emu_ragged

SAMPLE_MAX_K, SAMPLE_MAX_RANGE = 64, 2048


def _row_mask(mask, b, B, V, name):
    if mask is None:
        raise RuntimeError(f"sample_top_p_k_rows: {name} is NULL")
    assert mask.dtype == torch.uint8 and mask.is_contiguous() and mask.shape in ((V,), (B, V)), (name, mask.shape)
    return mask if mask.dim() == 1 else mask[b]


def sample_top_p_k_rows(logits, first_mask, lo_tab, hi_tab, ev, pos, q, out, V, temp, top_p, top_k, ban_mask, out_b=None,
                        out_c=None, first_span=(0, 0), max_range=0, fill_rest=0, fill_id=0):
    B = logits.shape[0]
    for t, ty, name in ((temp, torch.float32, "temp"), (top_p, torch.float32, "top_p"), (top_k, torch.int32, "top_k")):
        if t is None:
            raise RuntimeError(f"sample_top_p_k_rows: {name} is NULL")
        assert t.dtype == ty and t.shape == (B,) and t.is_contiguous(), (name, t.dtype, t.shape)
    if q is None:
        raise RuntimeError("sample_top_p_k_rows: q is NULL")
    assert q.dtype == torch.float32 and q.shape == (B, V) and out.dtype == torch.int64
    if not (B > 0 and V > 0 and 0 <= pos < lo_tab.shape[1] and 0 <= fill_rest < max(out.stride(0), 1)):
        raise RuntimeError("sample_top_p_k_rows: bad args")
    if not (first_span[0] >= 0 and first_span[1] <= V and first_span[1] - first_span[0] <= SAMPLE_MAX_RANGE
            and max_range <= SAMPLE_MAX_RANGE):
        raise RuntimeError(f"sample_top_p_k_rows: a grammar mask spans more than {SAMPLE_MAX_RANGE} ids")
    ids = torch.empty((B,), dtype=torch.int64)
    cols = torch.arange(V)
    for b in range(B):
        fm, bm = _row_mask(first_mask, b, B, V, "first_mask"), _row_mask(ban_mask, b, B, V, "ban_mask")
        k = min(max(int(top_k[b]), 1), SAMPLE_MAX_K, V)  # (the kernel's clamp)
        p = torch.softmax((logits[b, :V].float() / float(temp[b])).to(logits.dtype).float(), -1)
        if pos == 0:
            assert bool((fm[:first_span[0]] == 0).all()) and bool((fm[first_span[1]:] == 0).all()), "first_span does not cover the mask"
            ok = fm.bool()
        else:
            e = int(ev[b])
            ok = (cols >= lo_tab[e, pos]) & (cols < hi_tab[e, pos])
        p = p * ok * (bm == 0)
        ps, pi = torch.sort(p, dim=-1, descending=True, stable=True)
        cum = torch.cumsum(ps, -1)
        ps[cum - ps > float(top_p[b])] = 0.0
        ps[k:] = 0.0
        ps = ps / ps.sum(-1, keepdim=True)
        ids[b] = pi[torch.argmax(ps / q[b], -1)]
    out.copy_(ids)
    if fill_rest:  # `out` is column `pos` of a [B, T] buffer: the following columns get the pad id
        flat = out.as_strided((out.shape[0], fill_rest + 1), (out.stride(0), 1), out.storage_offset())
        flat[:, 1:] = fill_id
    for t in (out_b, out_c):
        if t is not None:
            t.copy_(ids)
    return out


_NAMES = ("sample_top_p_k_rows",)


@contextlib.contextmanager
def install():
    """emu_ragged.install() + the stand-in above (logged like every other op); yields the call log"""
    import midi_model_amd.ops as real
    with emu_ragged.install() as log:
        try:
            for n in _NAMES:
                setattr(real, n, emu_ragged._logged(n, globals()[n], log))
            yield log
        finally:
            for n in _NAMES:
                delattr(real, n)
