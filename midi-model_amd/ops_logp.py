"""The fused sampler with the drawn id's log-probability as one more output: the wrappers of mh_sample_top_p_k_rows_logp and
mh_sample_top_p_k_seeded_logp (include/midihip.h).  Reached as ``ops.sample_top_p_k_rows_logp`` / ``ops.sample_top_p_k_seeded_logp``
(ops resolves the names on first use, as it does ops_rows' and ops_seeded's, and for the same reason; the stand-ins are in
tests/emu_logp.py)."""
from __future__ import annotations

import torch

from .ops import _p, _rowmajor, _stream, dt, lib
from .ops_rows import mask_stride
from .ops_seeded import _check_seed_ctr


def _check_common(what, logits, lo_tab, hi_tab, ev, out, out_b, out_c, temp, top_p, top_k, logp):
    B = logits.shape[0]
    assert out.dtype == torch.int64
    assert lo_tab.dtype == torch.int32 and lo_tab.is_contiguous() and hi_tab.is_contiguous() and ev.dtype == torch.int64
    for t in (out_b, out_c):
        assert t is None or (t.dtype == torch.int64 and t.is_contiguous() and t.numel() == B)
    for t, ty, name in ((temp, torch.float32, "temp"), (top_p, torch.float32, "top_p"), (top_k, torch.int32, "top_k")):
        assert isinstance(t, torch.Tensor) and t.dtype == ty and t.shape == (B,) and t.is_contiguous(), \
            f"{what}: {name} must be a contiguous {ty} tensor of shape ({B},)"
    # row b writes logp[b]: a float32 vector of B entries at any positive stride (a column of a [B, T] buffer)
    assert isinstance(logp, torch.Tensor) and logp.dtype == torch.float32 and logp.shape == (B,) and logp.device == logits.device \
        and (B == 1 or logp.stride(0) >= 1), f"{what}: logp must be a float32 tensor of shape ({B},) at a positive stride"
    return B, (logp.stride(0) if B > 1 else 1)


def sample_top_p_k_rows_logp(logits, first_mask, lo_tab, hi_tab, ev, pos: int, q, out, V: int, temp, top_p, top_k, ban_mask, logp,
                             out_b=None, out_c=None, first_span=(0, 0), max_range: int = 0, fill_rest: int = 0, fill_id: int = 0):
    """ops.sample_top_p_k_rows -- the same ids, bit for bit -- that also writes logp[b] = z_c - log sum_{v < V} exp(z_v) (fp32) over
    row b's logits as stored, for the id c the row drew: the model's own log-probability, whatever the row's temperature, top-p,
    top-k and masks are.  ``logp``: float32 [B], any positive stride (``logp_rows[:, i]``); nothing else of its storage is written."""
    B, ls = _check_common("sample_top_p_k_rows_logp", logits, lo_tab, hi_tab, ev, out, out_b, out_c, temp, top_p, top_k, logp)
    assert q.dtype == torch.float32 and q.is_contiguous() and q.shape == (B, V)
    fs = mask_stride(first_mask, B, V, "sample_top_p_k_rows_logp: first_mask")
    bs = mask_stride(ban_mask, B, V, "sample_top_p_k_rows_logp: ban_mask")
    lib().call("mh_sample_top_p_k_rows_logp", _p(logits), _rowmajor(logits), _p(first_mask), fs, _p(ban_mask), bs, int(first_span[0]),
               int(first_span[1]), _p(lo_tab), _p(hi_tab), lo_tab.shape[1], int(max_range), _p(ev), pos, _p(q), _p(out),
               out.stride(0), _p(out_b), _p(out_c), B, V, _p(temp), _p(top_p), _p(top_k), fill_rest, fill_id, dt(logits), _stream(),
               _p(logp), ls)
    return out


def sample_top_p_k_seeded_logp(logits, first_mask, lo_tab, hi_tab, ev, pos: int, seed, ctr, out, V: int, temp, top_p, top_k, ban_mask,
                               logp, out_b=None, out_c=None, first_span=(0, 0), max_range: int = 0, fill_rest: int = 0,
                               fill_id: int = 0):
    """ops.sample_top_p_k_seeded -- the same ids, bit for bit -- with the ``logp`` output of sample_top_p_k_rows_logp"""
    B, ls = _check_common("sample_top_p_k_seeded_logp", logits, lo_tab, hi_tab, ev, out, out_b, out_c, temp, top_p, top_k, logp)
    _check_seed_ctr(seed, ctr, B, "sample_top_p_k_seeded_logp")
    fs = mask_stride(first_mask, B, V, "sample_top_p_k_seeded_logp: first_mask")
    bs = mask_stride(ban_mask, B, V, "sample_top_p_k_seeded_logp: ban_mask")
    lib().call("mh_sample_top_p_k_seeded_logp", _p(logits), _rowmajor(logits), _p(first_mask), fs, _p(ban_mask), bs,
               int(first_span[0]), int(first_span[1]), _p(lo_tab), _p(hi_tab), lo_tab.shape[1], int(max_range), _p(ev), pos, _p(seed),
               _p(ctr), _p(out), out.stride(0), _p(out_b), _p(out_c), B, V, _p(temp), _p(top_p), _p(top_k), fill_rest, fill_id,
               dt(logits), _stream(), _p(logp), ls)
    return out
