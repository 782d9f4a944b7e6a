"""CPU stand-ins for mh_sample_top_p_k_rows_logp and mh_sample_top_p_k_seeded_logp (ops.sample_top_p_k_rows_logp /
ops.sample_top_p_k_seeded_logp), in the style of emu_kvq.py: the ids are the existing sampler stand-ins' (emu_rowparams, emu_seeded),
the new output is ref_logp.logp64 of the row's logits as stored and the id drawn, rounded to fp32 -- plus the two argument checks of
the entry points.  ``install()`` is emu_kvq.install() (``base``: another install() to stack on, e.g. emu_poolshare's for a session
with prefix slots) with these patched on top; it yields the same CALL LOG, in which the stand-ins appear under their own names.  Test
infrastructure only."""
from __future__ import annotations

import contextlib

import torch

import emu_kvq
import emu_ragged
import emu_rowparams
import emu_seeded
import ref_logp


def _check_logp(logp, B, what):
    if logp is None:
        raise RuntimeError(f"{what}: logp is NULL")
    assert logp.dtype == torch.float32 and logp.shape == (B,), (what, "logp", logp.dtype, logp.shape)
    if B > 1 and logp.stride(0) < 1:
        raise RuntimeError(f"{what}: logp_stride={logp.stride(0)}, at least 1 is needed")


def _write(logits, out, V, logp):
    ids = out.reshape(-1).clone()
    ok = (ids >= 0) & (ids < V)
    val = ref_logp.logp64(logits, torch.where(ok, ids, torch.zeros_like(ids)), V).float()
    logp.copy_(torch.where(ok, val, torch.full_like(val, -float("inf"))))  # (only the B addressed floats: logp is a strided view)


def sample_top_p_k_rows_logp(logits, first_mask, lo_tab, hi_tab, ev, pos, q, out, V, temp, top_p, top_k, ban_mask, logp, out_b=None,
                             out_c=None, first_span=(0, 0), max_range=0, fill_rest=0, fill_id=0):
    _check_logp(logp, logits.shape[0], "sample_top_p_k_rows_logp")
    emu_rowparams.sample_top_p_k_rows(logits, first_mask, lo_tab, hi_tab, ev, pos, q, out, V, temp, top_p, top_k, ban_mask,
                                      out_b=out_b, out_c=out_c, first_span=first_span, max_range=max_range, fill_rest=fill_rest,
                                      fill_id=fill_id)
    _write(logits, out, V, logp)
    return out


def sample_top_p_k_seeded_logp(logits, first_mask, lo_tab, hi_tab, ev, pos, seed, ctr, out, V, temp, top_p, top_k, ban_mask, logp,
                               out_b=None, out_c=None, first_span=(0, 0), max_range=0, fill_rest=0, fill_id=0):
    _check_logp(logp, logits.shape[0], "sample_top_p_k_seeded_logp")
    emu_seeded.sample_top_p_k_seeded(logits, first_mask, lo_tab, hi_tab, ev, pos, seed, ctr, out, V, temp, top_p, top_k, ban_mask,
                                     out_b=out_b, out_c=out_c, first_span=first_span, max_range=max_range, fill_rest=fill_rest,
                                     fill_id=fill_id)
    _write(logits, out, V, logp)
    return out


_NAMES = ("sample_top_p_k_rows_logp", "sample_top_p_k_seeded_logp")


@contextlib.contextmanager
def install(base=None):
    """emu_kvq.install() (or ``base()``) + the stand-ins above (logged like every other op); yields the call log"""
    import midi_model_amd.ops as real
    with (base or emu_kvq.install)() as log:
        try:
            for n in _NAMES:
                setattr(real, n, emu_ragged._logged(n, globals()[n], log))
            yield log
        finally:
            for n in _NAMES:
                delattr(real, n)
