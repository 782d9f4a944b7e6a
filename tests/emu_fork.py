"""CPU stand-in for mh_kv_fork_rows (ops.kv_fork_rows), in the style of emu_pool.py: positions [0, len) of every (layer, head) of cache
sequence src[p] copied to sequence dst[p] of a whole cache [layers, B, H, Lmax, hd], plus the checks of the wrapper (three tables of
one length, ids in range, dst distinct, no id on both sides, 1 <= len <= Lmax).  ``install()`` is emu_seeded.install() (and with it
emu_pool's and emu_rowparams') with this one patched on top; it yields the same CALL LOG, in which the stand-in appears under its own
name.  Test infrastructure only."""
from __future__ import annotations

import contextlib

import torch

import emu_ragged
import emu_seeded


def kv_fork_rows(kv_k, kv_v, src, dst, lengths, dev=None):
    assert kv_k.dim() == 5 and kv_v.shape == kv_k.shape and kv_k.is_contiguous() and kv_v.is_contiguous() and kv_k.dtype == kv_v.dtype
    layers, B, H, Lmax, hd = kv_k.shape
    assert hd % 8 == 0
    s, d, ln = [int(r) for r in src], [int(r) for r in dst], [int(n) for n in lengths]
    if not (len(s) == len(d) == len(ln)) or not s:
        raise ValueError(f"kv_fork_rows: {len(s)} sources, {len(d)} destinations and {len(ln)} lengths")
    if any(r < 0 or r >= B for r in s + d):
        raise ValueError(f"kv_fork_rows: a cache row outside [0, {B}): sources {s}, destinations {d}")
    if len(set(d)) != len(d):
        raise ValueError(f"kv_fork_rows: a destination row named twice: {d}")
    if set(s) & set(d):
        raise ValueError(f"kv_fork_rows: rows {sorted(set(s) & set(d))} are source and destination at once")
    if any(n < 1 or n > Lmax for n in ln):
        raise ValueError(f"kv_fork_rows: a length outside [1, {Lmax}]: {ln}")
    if dev is not None:  # (the device copy the kernel reads must be the host copy that was checked)
        assert dev.dtype == torch.int32 and dev.shape == (3, len(s)) and dev.is_contiguous() and dev.tolist() == [s, d, ln]
    for a, b, n in zip(s, d, ln):
        kv_k[:, b, :, :n] = kv_k[:, a, :, :n]
        kv_v[:, b, :, :n] = kv_v[:, a, :, :n]


_NAMES = ("kv_fork_rows",)


@contextlib.contextmanager
def install():
    """emu_seeded.install() + the stand-in above (logged like every other op); yields the call log"""
    import midi_model_amd.ops as real
    with emu_seeded.install() as log:
        try:
            for n in _NAMES:
                setattr(real, n, emu_ragged._logged(n, globals()[n], log))
            yield log
        finally:
            for n in _NAMES:
                delattr(real, n)
