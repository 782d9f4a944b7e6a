"""Mixed-precision training state: fp32 master weights, fp32 AdamW moments and an fp32 gradient accumulator behind the bf16
parameter buffer the forward / backward kernels run on (``TrainMIDIModel(precision="bf16-mixed")``).

The compute path is the bf16-true one, untouched.  What changes is the optimiser side:

  * every micro-batch's bf16 gradient is folded into ``g32`` (``mh_grad_fold_f32``: the first of a window overwrites, the
    later ones add -- one exact conversion and one fp32 add per element),
  * the clip norm is taken from ``g32`` (``mh_sumsq`` with the fp32 dtype),
  * ``mh_adamw_master`` updates ``master`` / ``m`` / ``v`` in fp32 and writes the bf16 working copy in the same pass, so after
    every update the model's flat buffer is exactly ``master`` rounded to bf16 (nearest, ties to even).

+16 bytes per parameter (3.7 GB for tv2o-medium).  The two wrappers live here, not in ``ops.py``.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops
from .lib import lib
from .ops import _p, _stream, dt

PRECISIONS_NATIVE = ("bf16-true", "bf16", "32-true", "32")   # names for "the dtype of the model decides" (also: None)
PRECISION_MIXED = "bf16-mixed"


def check_precision(precision: Optional[str]) -> Optional[str]:
    """the reference's ``--precision`` choices (train.py:365-371) this build runs; -> "bf16-mixed" or None (native)"""
    if precision is None or precision in PRECISIONS_NATIVE:
        return None
    if precision == PRECISION_MIXED:
        return PRECISION_MIXED
    raise ValueError(f"precision={precision!r} is not supported: this build trains in {', '.join(PRECISIONS_NATIVE)} (the model's own "
                     f"dtype, the default) or {PRECISION_MIXED} (fp32 master weights behind bf16 compute); the fp16 and fp64 "
                     "modes of the reference (16-mixed, 16-true, 64-true) are out of scope")


def grad_fold(src: torch.Tensor, dst: torch.Tensor, accumulate: bool) -> None:
    """dst = float(src), or dst += float(src): one micro-batch's gradient range into the fp32 accumulator"""
    assert dst.dtype == torch.float32 and src.numel() == dst.numel() and src.is_contiguous() and dst.is_contiguous()
    lib().call("mh_grad_fold_f32", _p(src), _p(dst), src.numel(), int(accumulate), dt(src), _stream())


def adamw_master(p32, p_lo, g32, m, v, lr, b1, b2, eps, wd, bc1, bc2, coef_dev) -> None:
    """torch.optim.AdamW's single-tensor update in fp32 on (p32, m, v) from g32 * coef; p_lo = the new p32 rounded to p_lo's dtype"""
    assert p32.dtype == g32.dtype == m.dtype == v.dtype == torch.float32
    assert p32.numel() == p_lo.numel() == g32.numel() == m.numel() == v.numel()
    lib().call("mh_adamw_master", _p(p32), _p(p_lo), _p(g32), _p(m), _p(v), p32.numel(), lr, b1, b2, eps, wd, bc1, bc2,
               _p(coef_dev), dt(p_lo), _stream())


class MixedState:
    """The optimiser's four flat fp32 buffers in the parameter layout (+ the clip scalars ``TrainMIDIModel._opt`` also holds)."""

    def __init__(self, flat_lo: torch.Tensor):
        if flat_lo.dtype != torch.bfloat16:
            raise TypeError(f"bf16-mixed keeps fp32 master weights behind a bfloat16 model; this model is {flat_lo.dtype} "
                            "(move it with .to(torch.bfloat16) first, or train it in its own dtype with precision=None)")
        dev = flat_lo.device
        self.flat_lo = flat_lo
        self.master = flat_lo.float()
        self.m = torch.zeros_like(self.master)
        self.v = torch.zeros_like(self.master)
        self.g32 = torch.zeros_like(self.master)
        self.sumsq = torch.zeros(1, dtype=torch.float32, device=dev)
        self.partial = torch.empty(1024, dtype=torch.float32, device=dev)
        self.coef = torch.ones(1, dtype=torch.float32, device=dev)
        self.norm = torch.zeros(1, dtype=torch.float32, device=dev)

    def fold(self, grad_lo: torch.Tensor, lo: int, hi: int, accumulate: bool) -> None:
        grad_fold(grad_lo[lo:hi], self.g32[lo:hi], accumulate)

    def derive_working_copy(self) -> None:
        """flat_lo <- master rounded to bf16 (after the master was written from outside: a checkpoint, a broadcast)"""
        ops.cast_from_f32(self.master, self.flat_lo, False)

    def step(self, n_mat: int, lr: float, betas, eps: float, weight_decay: float, bc1: float, bc2: float, coef) -> None:
        """the reference's two parameter groups: the matrix region with weight decay, the norm vectors without"""
        for a, b, wd in ((0, n_mat, weight_decay), (n_mat, self.master.numel(), 0.0)):
            if b > a:
                adamw_master(self.master[a:b], self.flat_lo[a:b], self.g32[a:b], self.m[a:b], self.v[a:b], lr, betas[0], betas[1],
                             eps, wd, bc1, bc2, coef)
