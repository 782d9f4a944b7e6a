"""The grouped weight-gradient launch (mh_gemm_wgrad_grouped, csrc/gemm_pp256.hip): several weight gradients over the same
contraction rows in ONE launch, every 256 x 256 tile contracting the whole row range -- no split-K, no fp32 partials, no reduction
launch -- with the plain epilogue or the folded RMSNorm's chain rule as epilogue.  Reached as ops.wgrad_grouped / ops.wgrad_grouped_ok /
ops.wgrad_grouped_enabled / ops.wgrad_grouped_launches (resolved on first use, as ops_packed.py's entry points are, and for the
same reason).
"""
from __future__ import annotations

import ctypes
import os

import torch

from . import ops
from .lib import MH_BF16, lib
from .ops import _p, _rowmajor, _stream, dt


class _WgradProblem(ctypes.Structure):
    """mh_wgrad_problem of include/midihip.h"""
    _fields_ = [("dz", ctypes.c_void_p), ("lddz", ctypes.c_int64), ("x", ctypes.c_void_p), ("ldx", ctypes.c_int64),
                ("dw", ctypes.c_void_p), ("lddw", ctypes.c_int64), ("R", ctypes.c_void_p), ("ldr", ctypes.c_int64),
                ("N", ctypes.c_int64), ("K_out", ctypes.c_int64), ("alpha", ctypes.c_float), ("beta", ctypes.c_float),
                ("wnorm", ctypes.c_void_p), ("W", ctypes.c_void_p), ("ldw", ctypes.c_int64), ("colpart", ctypes.c_void_p)]


WGRAD_GROUP_MAX = 8          # problems per grouped launch (GRP_MAX of gemm_pp256.hip)
wgrad_grouped_launches = 0   # grouped launches issued by this process (tests assert the path through it)


def wgrad_grouped_enabled() -> bool:
    """MH_WGRAD_GROUPED=0 restores one split-K launch (+ reduction) per weight gradient"""
    return os.environ.get("MH_WGRAD_GROUPED", "1") != "0"


def wgrad_grouped_operands_ok(problems) -> bool:
    """whether mh_gemm_wgrad_grouped takes these (dz, x, dw, fold) problems: bf16 device tensors on the production GEMM, one
    contraction length, 16-byte lines where the kernel moves whole lines"""
    if not (1 <= len(problems) <= WGRAD_GROUP_MAX) or ops.get_option("gemm") == 0 or not wgrad_grouped_enabled():
        return False
    Kc = problems[0][0].shape[0]
    for dz, x, dw, fold in problems:
        if not (dz.is_cuda and dz.dtype == x.dtype == dw.dtype == torch.bfloat16 and dz.shape[0] == x.shape[0] == Kc):
            return False
        if _rowmajor(dz) % 8 or _rowmajor(x) % 8 or (dz.data_ptr() | x.data_ptr()) % 16:
            return False
        if fold is not None:
            wnorm, W, _ = fold
            if dw.shape[1] % 8 or _rowmajor(dw) % 8 or _rowmajor(W) % 8 or (dw.data_ptr() | W.data_ptr() | wnorm.data_ptr()) % 16:
                return False
    return True


def wgrad_grouped_ok(shapes, Kc: int, like: torch.Tensor) -> bool:
    """Whether the weight gradients of ``shapes`` = [(N, K_out), ...] over a common contraction of Kc rows go out as ONE grouped
    launch (wgrad_grouped): bf16 on the production GEMM, and 256 x 256 tiles that fill the 256 CUs in whole rounds -- a whole
    multiple of 256, or at most 10 % of the last round left empty.  Otherwise every gradient keeps its own split-K launch."""
    if not like.is_cuda or like.dtype != torch.bfloat16 or ops.get_option("gemm") == 0 or not wgrad_grouped_enabled():
        return False
    if not (1 <= len(shapes) <= WGRAD_GROUP_MAX) or Kc < 1:
        return False
    tiles = sum(((n + 255) // 256) * ((k + 255) // 256) for n, k in shapes)
    empty = -tiles % 256
    return empty * 10 <= 256


def wgrad_grouped(problems, accumulate: bool) -> None:
    """All weight gradients of ``problems`` in ONE launch, every tile contracting the whole row range (no split-K, no fp32
    partials, no reduction): problem = (dz [M, N], x [M, K], dw [N, K], fold) with dw (+)= dz^T @ x, or, behind a folded RMSNorm
    (fold = (wnorm [K], W [N, K], dnorm [K])), dw (+)= G' * wnorm[None, :] and dnorm (+)= colsum(G' * W) as ops.wgrad_folded -- the
    fold runs in the GEMM epilogue, mh_colsum folds its per-tile-row column sums.  One fp32 chain per element, fixed order."""
    global wgrad_grouped_launches
    assert wgrad_grouped_operands_ok(problems), "wgrad_grouped: bf16 problems over one contraction length on the production GEMM"
    M = problems[0][0].shape[0]
    arr = (_WgradProblem * len(problems))()
    folds, flops, rows = [], 0.0, 0
    for q, (dz, x, dw, fold) in zip(arr, problems):
        N, K = dw.shape
        assert dz.shape == (M, N) and x.shape == (M, K), (dz.shape, x.shape, dw.shape)
        q.dz, q.lddz, q.x, q.ldx, q.dw, q.lddw = _p(dz), _rowmajor(dz), _p(x), _rowmajor(x), _p(dw), _rowmajor(dw)
        q.R, q.ldr = (_p(dw), _rowmajor(dw)) if accumulate else (None, 0)
        q.N, q.K_out, q.alpha, q.beta = N, K, 1.0, 1.0 if accumulate else 0.0
        if fold is not None:
            wnorm, W, dnorm = fold
            assert W.shape == (N, K) and wnorm.shape == (K,) and dnorm.shape == (K,)
            nblk = lib().cdll.mh_wgrad_grouped_fold_blocks(N)
            colpart = torch.empty((nblk, K), dtype=torch.float32, device=dw.device)
            q.wnorm, q.W, q.ldw, q.colpart = _p(wnorm), _p(W), _rowmajor(W), _p(colpart)
            folds.append((colpart, nblk, dnorm, K))
        flops += 2.0 * M * N * K
        rows += N
    prof = ops.gemm_profile
    if prof is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    lib().call("mh_gemm_wgrad_grouped", arr, len(problems), M, MH_BF16, _stream())
    for colpart, nblk, dnorm, K in folds:
        lib().call("mh_colsum", _p(colpart), nblk, _p(dnorm), K, int(accumulate), dt(dnorm), _stream())
    wgrad_grouped_launches += 1
    if prof is not None:  # (the window includes the column-sum folds, as wgrad_folded's)
        e1.record()
        prof.append((e0, e1, flops, (rows, max(p[2].shape[1] for p in problems), M, 1, 1, 1, "+grouped")))
