"""CPU stand-ins for the wrappers of decode batches of 65 to 256 rows (midi_model_amd/ops_wide.py): ``gemm_skinny_wide`` is
emu_ops.gemm_skinny's arithmetic behind the entry point's refusals (bf16, 64 < rows <= 256, K a multiple of 256), ``skinny_wide_ok``
and ``decode_wide_enabled`` answer as the real ones do.  ``install()`` is the ragged fake backend (emu_ragged.install(), which yields
the CALL LOG) with these patched on top, the projection logged under its own name.  Test infrastructure only."""
from __future__ import annotations

import contextlib
import os

import torch

import emu_ops
import emu_ragged


def skinny_wide_ok(x, K, rows=None):
    return x.dtype == torch.bfloat16 and 64 < (x.shape[0] if rows is None else rows) <= 256 and K % 256 == 0


def decode_wide_enabled():
    return os.environ.get("MH_DECODE_WIDE", "1") != "0"


def gemm_skinny_wide(a, w, out, *, mode=0, res=None, norm_eps=0.0, row_ids=None, res_ids=None):
    M, K = out.shape[0], w.shape[1]
    if out.dtype != torch.bfloat16:
        raise RuntimeError("mh_gemm_skinny_wide failed (1): gemm_skinny_wide: bf16 only")
    if not 64 < M <= 256:
        raise RuntimeError(f"mh_gemm_skinny_wide failed (1): gemm_skinny_wide: needs 65 <= M <= 256 rows (M={M})")
    if K % 256:
        raise RuntimeError(f"mh_gemm_skinny_wide failed (1): gemm_skinny_wide: K={K} must be a multiple of 256")
    return emu_ops.gemm_skinny(a, w, out, mode=mode, res=res, norm_eps=norm_eps, row_ids=row_ids, res_ids=res_ids)


_NAMES = ("gemm_skinny_wide", "skinny_wide_ok", "decode_wide_enabled")
_LOGGED = ("gemm_skinny_wide",)  # the other two answer from shapes / the environment: no launch behind them


@contextlib.contextmanager
def install():
    """emu_ragged.install() + the stand-ins above; yields the call log"""
    import midi_model_amd.ops as real
    with emu_ragged.install() as log:
        try:
            for n in _NAMES:
                fn = globals()[n]
                setattr(real, n, emu_ragged._logged(n, fn, log) if n in _LOGGED else fn)
            yield log
        finally:
            for n in _NAMES:
                delattr(real, n)
