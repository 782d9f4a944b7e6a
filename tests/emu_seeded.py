"""CPU stand-ins for mh_sample_top_p_k_seeded and mh_sample_noise_seeded (ops.sample_top_p_k_seeded / ops.sample_noise_seeded), in
the style of emu_rowparams.py: the variates come from ref_philox (numpy Philox4x32-10, float64 -log(u) rounded to float32), the
rest is emu_rowparams' chain on a q whose first 64 columns are those variates -- plus the argument checks of the entry points and
of the wrappers.  ``install()`` is emu_pool.install() (and with it emu_rowparams') with these two patched on top; it yields the
same CALL LOG, in which the stand-ins appear under their own names.  Test infrastructure only."""
from __future__ import annotations

import contextlib

import numpy as np
import torch

import emu_pool
import emu_ragged
import emu_rowparams
import ref_philox

LANES = 64


def _check(seed, ctr, B, what):
    if seed is None:
        raise RuntimeError(f"{what}: seed is NULL")
    if ctr is None:
        raise RuntimeError(f"{what}: ctr is NULL")
    assert seed.dtype == torch.int64 and seed.shape == (B,) and seed.is_contiguous(), (what, "seed", seed.dtype, seed.shape)
    assert ctr.dtype == torch.int32 and ctr.shape == (B,) and ctr.is_contiguous(), (what, "ctr", ctr.dtype, ctr.shape)


def _noise(seed, ctr, pos):
    bits, q = ref_philox.noise(seed.numpy().view(np.uint64), ctr.numpy(), pos, LANES)
    return bits, q.astype(np.float32)


def sample_noise_seeded(seed, ctr, pos, bits=None, q=None):
    B = (seed if seed is not None else ctr).shape[0]
    _check(seed, ctr, B, "sample_noise_seeded")
    if not (B > 0 and pos >= 0):
        raise RuntimeError("sample_noise_seeded: bad args")
    x, v = _noise(seed, ctr, pos)
    x, v = torch.from_numpy(x.view(np.int32).copy()), torch.from_numpy(v)
    if bits is None:
        bits = torch.empty((B, LANES), dtype=torch.int32)
    if q is None:
        q = torch.empty((B, LANES), dtype=torch.float32)
    assert bits.dtype == torch.int32 and bits.shape == (B, LANES) and q.dtype == torch.float32 and q.shape == (B, LANES)
    bits.copy_(x)
    q.copy_(v)
    return bits, q


def sample_top_p_k_seeded(logits, first_mask, lo_tab, hi_tab, ev, pos, seed, ctr, out, V, temp, top_p, top_k, ban_mask, out_b=None,
                          out_c=None, first_span=(0, 0), max_range=0, fill_rest=0, fill_id=0):
    B = logits.shape[0]
    _check(seed, ctr, B, "sample_top_p_k_seeded")
    q = torch.ones((B, V), dtype=torch.float32)  # (ranks >= 64 have probability 0: top_k <= 64)
    n = min(LANES, V)
    q[:, :n] = torch.from_numpy(_noise(seed, ctr, pos)[1][:, :n])
    return emu_rowparams.sample_top_p_k_rows(logits, first_mask, lo_tab, hi_tab, ev, pos, q, out, V, temp, top_p, top_k, ban_mask,
                                             out_b=out_b, out_c=out_c, first_span=first_span, max_range=max_range,
                                             fill_rest=fill_rest, fill_id=fill_id)


_NAMES = ("sample_top_p_k_seeded", "sample_noise_seeded")


@contextlib.contextmanager
def install():
    """emu_pool.install() + the stand-ins above (logged like every other op); yields the call log"""
    import midi_model_amd.ops as real
    with emu_pool.install() as log:
        try:
            for n in _NAMES:
                setattr(real, n, emu_ragged._logged(n, globals()[n], log))
            yield log
        finally:
            for n in _NAMES:
                delattr(real, n)
