"""A LoRA adapter per row of a decode batch, unmerged: the wrappers of mh_lora_shrink_rows and mh_gemm_skinny_ext
(gemm_skinny.hip; include/midihip.h states the arithmetic).  Reached as ``ops.lora_shrink_rows``, ``ops.gemm_skinny_ext`` and
``ops.skinny_ext_ok`` (ops resolves the names on first use, like the fp8-cache forms, and for the reason given there).  Raw device
pointers on the current stream, one launch each, no torch math; what the entry points refuse is refused here first, as a
``ValueError`` before any call.

A row's projection is  x W^T + s (x A^T) B^T  with A, B, s of the row's adapter.  For G slots of rank R:
  shrink   T[m, (p G + g) R + j] = s_g (x_m . A_{p,g}[j])  where row m uses slot g, 0 elsewhere      (one launch per projection)
  expand   G R more columns of contraction of the projection itself, against Bst[w, g R + j] = B_g[w, j]: a row's T is non-zero
           only in the block of its slot, a row without adapter adds exact zeros."""
from __future__ import annotations

from typing import Optional

import torch

from .ops import SKINNY_GATEUP, SKINNY_PLAIN, _p, _rowmajor, _stream, dt, lib

EXT_MAX_ROWS = 256


def skinny_ext_ok(x: torch.Tensor, K: int, rows: Optional[int] = None) -> bool:
    """whether the two entry points serve this decode projection: bf16, 1 to 256 rows, K a multiple of 256"""
    M = x.shape[0] if rows is None else rows
    return x.dtype == torch.bfloat16 and 1 <= M <= EXT_MAX_ROWS and K % 256 == 0


def _block_cols(mode: int, N: int) -> int:
    """columns of one workgroup's block by the launcher's DEFAULT rule.  The entry point is the authority: under the test option
    "skinny_nbt" its tiling differs and it refuses by its own rule (a RuntimeError from the call, still before any launch)."""
    return 16 if (mode == SKINNY_GATEUP or N < 2048) else 32


def check_parts(mode: int, N: int, parts: int) -> None:
    """ValueError where a part boundary would fall inside a workgroup's column block (mh_gemm_skinny_ext refuses it too)"""
    rows = 2 * N if mode == SKINNY_GATEUP else N
    if parts < 1 or rows % parts:
        raise ValueError(f"gemm_skinny_ext: {parts} parts do not divide {rows} weight rows")
    rpp = rows // parts
    if mode == SKINNY_GATEUP:
        ok = parts in (1, 2) or (rpp % 16 == 0 and N % rpp == 0)
    else:
        ok = parts == 1 or rpp % _block_cols(mode, N) == 0
    if not ok:
        raise ValueError(f"gemm_skinny_ext: a part boundary (every {rpp} weight rows) falls inside a {_block_cols(mode, N)}-column block")


def lora_shrink_rows(a: torch.Tensor, a_stack: torch.Tensor, t: torch.Tensor, row_adapter: torch.Tensor, slot_scale: torch.Tensor,
                     G: int, R: int, parts: int, row_ids: Optional[torch.Tensor] = None) -> torch.Tensor:
    """t[M, parts G R] = the masked, scaled products of the rows of ``a`` (or of a[row_ids]) with the stacked LoRA-A matrices
    ``a_stack`` [parts G R, K] (rows laid out [part][slot][R]); every element of ``t`` is written"""
    M, N = t.shape
    K = a_stack.shape[1]
    if a.dtype != torch.bfloat16 or a_stack.dtype != torch.bfloat16 or t.dtype != torch.bfloat16:
        raise ValueError("lora_shrink_rows: bf16 only")
    if not (1 <= M <= EXT_MAX_ROWS) or K % 256 or R % 8 or G < 1 or N != parts * G * R or a_stack.shape[0] != N:
        raise ValueError(f"lora_shrink_rows: M={M} K={K} G={G} R={R} parts={parts} against t {tuple(t.shape)}, a_stack {tuple(a_stack.shape)}")
    assert a.shape[1] == K and (row_ids is not None or a.shape[0] == M), (a.shape, t.shape)
    assert row_adapter.dtype == torch.int32 and row_adapter.is_contiguous() and row_adapter.numel() == M
    assert slot_scale.dtype == torch.float32 and slot_scale.is_contiguous() and slot_scale.numel() == G
    assert row_ids is None or (row_ids.dtype == torch.int64 and row_ids.is_contiguous() and row_ids.numel() == M)
    if a.shape[0] * _rowmajor(a) >= 2 ** 31 or N * _rowmajor(a_stack) >= 2 ** 31 or EXT_MAX_ROWS * _rowmajor(t) >= 2 ** 31:
        raise ValueError("lora_shrink_rows: operands too large for 32-bit element offsets")
    lib().call("mh_lora_shrink_rows", _p(a), _rowmajor(a), _p(a_stack), _rowmajor(a_stack), _p(t), _rowmajor(t), _p(row_adapter),
               _p(slot_scale), _p(row_ids), M, K, G, R, parts, dt(t), _stream())
    return t


def gemm_skinny_ext(a: torch.Tensor, w: torch.Tensor, out: torch.Tensor, t: torch.Tensor, b_stack: torch.Tensor, parts: int, *,
                    mode: int = SKINNY_PLAIN, res: Optional[torch.Tensor] = None, norm_eps: float = 0.0,
                    row_ids: Optional[torch.Tensor] = None, res_ids: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ops.gemm_skinny / gemm_skinny_wide (same arguments, 1 to 256 rows) with a second operand pair: weight row n also
    contracts t[m, part(n) K2 : part(n) K2 + K2] with b_stack[n, :K2], K2 = b_stack.shape[1], part(n) = n // (rows(w) // parts);
    row scale, residual, gathers and SwiGLU apply to the sum, the sum of squares comes from ``a`` alone"""
    M, N = out.shape
    K, K2 = w.shape[1], b_stack.shape[1]
    if out.dtype != torch.bfloat16 or any(x.dtype != torch.bfloat16 for x in (a, w, t, b_stack)):
        raise ValueError("gemm_skinny_ext: bf16 only")
    if not (1 <= M <= EXT_MAX_ROWS) or K % 256 or K2 % 256 or K2 == 0:
        raise ValueError(f"gemm_skinny_ext: needs 1..256 rows and K, K2 multiples of 256 (M={M} K={K} K2={K2})")
    check_parts(mode, N, parts)
    assert a.shape[1] == K and (row_ids is not None or a.shape[0] == M), (a.shape, out.shape)
    assert w.shape[0] == (2 * N if mode == SKINNY_GATEUP else N) and b_stack.shape[0] == w.shape[0], (w.shape, b_stack.shape, out.shape, mode)
    assert t.shape == (M, parts * K2), (t.shape, M, parts, K2)
    for ids in (row_ids, res_ids):
        assert ids is None or (ids.dtype == torch.int64 and ids.is_contiguous() and ids.numel() == M)
    if (a.shape[0] * _rowmajor(a) >= 2 ** 31 or (res is not None and res.shape[0] * _rowmajor(res) >= 2 ** 31)
            or w.shape[0] * max(_rowmajor(w), _rowmajor(b_stack)) >= 2 ** 31 or EXT_MAX_ROWS * max(_rowmajor(t), _rowmajor(out)) >= 2 ** 31):
        raise ValueError("gemm_skinny_ext: operands too large for 32-bit element offsets")
    lib().call("mh_gemm_skinny_ext", _p(a), _rowmajor(a), _p(w), _rowmajor(w), _p(out), _rowmajor(out), _p(res),
               _rowmajor(res) if res is not None else 0, _p(t), _rowmajor(t), _p(b_stack), _rowmajor(b_stack), mode, norm_eps,
               _p(row_ids), _p(res_ids), M, N, K, K2, parts, dt(out), _stream())
    return out
