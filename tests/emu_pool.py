"""CPU stand-in for mh_kv_store_seqs_rows (ops.kv_store_seqs_rows), in the style of emu_rowparams.py: emu_ragged.kv_store_seqs
restated with sequence s going to cache sequence rows[s], plus the checks of the wrapper (row ids in range and distinct, lengths
within the cache).  ``install()`` is emu_rowparams.install() with this one patched on top; it yields the same CALL LOG, in which the
stand-in appears under its own name.  Test infrastructure only."""
from __future__ import annotations

import contextlib

import torch

import emu_ragged
import emu_rowparams


def kv_store_seqs_rows(qkv, plan, rows, kc, vc, H, hd, Lmax, rows_dev=None):
    B, D = kc.shape[0], H * hd
    ids = [int(r) for r in rows]
    if len(ids) != plan.n:
        raise ValueError(f"kv_store_seqs_rows: {len(ids)} cache rows for {plan.n} sequences")
    if any(r < 0 or r >= B for r in ids):
        raise ValueError(f"kv_store_seqs_rows: a cache row outside [0, {B}): {ids}")
    if len(set(ids)) != len(ids):
        raise ValueError(f"kv_store_seqs_rows: a cache row named twice: {ids}")
    if plan.max_len > Lmax:
        raise ValueError(f"kv_store_seqs_rows: a sequence of {plan.max_len} rows in a cache of {Lmax}")
    assert qkv.shape == (plan.M, 3 * D) and kc.shape == (B, H, Lmax, hd) and vc.shape == kc.shape and hd % 8 == 0
    if rows_dev is not None:  # (the device copy the kernel reads must be the host copy that was checked)
        assert rows_dev.dtype == torch.int32 and rows_dev.tolist() == ids
    start = plan.host_views()[0].tolist()
    for s, (a, b) in enumerate(zip(start[:-1], start[1:])):
        kc[ids[s], :, :b - a] = qkv[a:b, D:2 * D].view(b - a, H, hd).transpose(0, 1)
        vc[ids[s], :, :b - a] = qkv[a:b, 2 * D:].view(b - a, H, hd).transpose(0, 1)


_NAMES = ("kv_store_seqs_rows",)


@contextlib.contextmanager
def install():
    """emu_rowparams.install() + the stand-in above (logged like every other op); yields the call log"""
    import midi_model_amd.ops as real
    with emu_rowparams.install() as log:
        try:
            for n in _NAMES:
                setattr(real, n, emu_ragged._logged(n, globals()[n], log))
            yield log
        finally:
            for n in _NAMES:
                delattr(real, n)
