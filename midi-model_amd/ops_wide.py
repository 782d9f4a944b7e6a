"""Decode batches of 65 to 256 rows: the wrappers of mh_gemm_skinny_wide (include/midihip.h).  Reached as ``ops.gemm_skinny_wide``,
``ops.skinny_wide_ok`` and ``ops.decode_wide_enabled`` (ops resolves these names on first use, as it does the packed entry points,
and for the same reason: the CPU emulation of the test suite wants a stand-in of its own for every plain function of ops.py; the
stand-ins of these are in tests/emu_wide.py)."""
from __future__ import annotations

import os
from typing import Optional

import torch

from .ops import SKINNY_GATEUP, SKINNY_PLAIN, _p, _rowmajor, _stream, dt, lib

WIDE_MAX_ROWS = 256  # the entry point's cap; rows 1..64 belong to mh_gemm_skinny


def gemm_skinny_wide(a: torch.Tensor, w: torch.Tensor, out: torch.Tensor, *, mode: int = SKINNY_PLAIN,
                     res: Optional[torch.Tensor] = None, norm_eps: float = 0.0, row_ids: Optional[torch.Tensor] = None,
                     res_ids: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ops.gemm_skinny for 64 < M <= 256 rows (mh_gemm_skinny_wide): same arguments, same arithmetic and roundings"""
    M, N = out.shape
    K = w.shape[1]
    assert a.shape[1] == K and (row_ids is not None or a.shape[0] == M), (a.shape, out.shape)
    assert w.shape[0] == (2 * N if mode == SKINNY_GATEUP else N), (a.shape, w.shape, out.shape, mode)
    for t in (row_ids, res_ids):
        assert t is None or (t.dtype == torch.int64 and t.is_contiguous() and t.numel() == M)
    # (the kernel addresses with 32-bit element offsets: the tables behind row_ids / res_ids must stay below 2^31 elements)
    assert a.shape[0] * _rowmajor(a) < 2 ** 31 and (res is None or res.shape[0] * _rowmajor(res) < 2 ** 31), \
        "gemm_skinny_wide: table too large"
    lib().call("mh_gemm_skinny_wide", _p(a), _rowmajor(a), _p(w), _rowmajor(w), _p(out), _rowmajor(out), _p(res),
               _rowmajor(res) if res is not None else 0, mode, norm_eps, _p(row_ids), _p(res_ids), M, N, K, dt(out),
               _stream())
    return out


def skinny_wide_ok(x: torch.Tensor, K: int, rows: Optional[int] = None) -> bool:
    """whether mh_gemm_skinny_wide serves this decode projection: bf16, 65 to 256 rows (ops.skinny_ok answers for 1 to 64).
    ``rows``: the row count when ``x`` is a table the rows are gathered from (row_ids) and not the activations themselves"""
    M = x.shape[0] if rows is None else rows
    return x.dtype == torch.bfloat16 and 64 < M <= WIDE_MAX_ROWS and K % 256 == 0


def decode_wide_enabled() -> bool:
    """MH_DECODE_WIDE=0: decode batches of more than 64 rows keep the general GEMM form (the A/B arm and the escape hatch).
    A decode session asks once, when it is created."""
    return os.environ.get("MH_DECODE_WIDE", "1") != "0"
