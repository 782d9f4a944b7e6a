"""Forward / backward / decode schedules of one LLaMA stack (event-level `net` or token-level `net_token`)
as explicit sequences of C-ABI kernel launches — no autograd graph, no tracing compiler.

Block wiring follows TF:models/llama/modeling_llama.py:295-324 (pre-norm residual layer) and :367-417
(model: layers + final norm); see SURVEY.md §8 a5-a9.  Weights of a layer are views into the model's flat
parameter buffer, with q|k|v and gate|up stored contiguously so each pair is ONE projection GEMM.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Callable, List, NamedTuple, Optional

import os

import torch

from . import ops, tokfirst


@dataclass
class StackSpec:
    name: str            # "net" | "net_token"
    D: int
    H: int
    I: int
    L: int
    eps: float
    theta: float
    kind: str            # "event" (causal flash attention, head_dim 64) | "token" (<=8-token sequences, head_dim 256)

    @property
    def hd(self) -> int:
        return self.D // self.H

    @property
    def scale(self) -> float:
        return self.hd ** -0.5


@dataclass
class LayerTensors:
    wqkv: torch.Tensor = None   # [3D, D]
    wo: torch.Tensor = None     # [D, D]
    wgu: torch.Tensor = None    # [2I, D]
    wd: torch.Tensor = None     # [D, I]
    n1: torch.Tensor = None     # [D]
    n2: torch.Tensor = None     # [D]


@dataclass
class StackTensors:
    """One of: weights, transposed weights ([in,out] copies for dgrad), gradients."""
    embed: torch.Tensor = None  # [V, D]
    layers: List[LayerTensors] = field(default_factory=list)
    norm: torch.Tensor = None   # [D]


class RopeTable:
    """fp32 cos/sin of pos * theta^(-2i/hd), [npos, hd/2] (TF:models/llama/modeling_llama.py:113-127)."""

    def __init__(self, hd: int, theta: float, device, npos: int = 0):
        self.hd, self.theta, self.device = hd, theta, device
        self.cos = self.sin = None
        self._fused = None
        self.n = 0
        if npos:
            self.ensure(npos)

    def ensure(self, npos: int):
        if npos <= self.n:
            return
        npos = max(npos, 2 * self.n, 64)
        inv_freq = 1.0 / (self.theta ** (torch.arange(0, self.hd, 2, dtype=torch.int64).float() / self.hd))
        ang = torch.arange(npos).float()[:, None] * inv_freq[None, :]
        self.cos = ang.cos().contiguous().to(self.device)
        self.sin = ang.sin().contiguous().to(self.device)
        self.n = npos
        self._fused = None

    def fused(self) -> torch.Tensor:
        """bf16 [npos, 96] = cos | -sin | +sin (head_dim 64): the table of mh_gemm_rope's epilogue"""
        if self._fused is None or self._fused.shape[0] != self.n:
            c, s = self.cos.to(torch.bfloat16), self.sin.to(torch.bfloat16)
            self._fused = torch.cat([c, -s, s], dim=1).contiguous()
        return self._fused


def _empty(shape, like: torch.Tensor, dtype=None):
    return torch.empty(shape, dtype=dtype or like.dtype, device=like.device)


def _check_heads(spec: StackSpec):
    want = 64 if spec.kind == "event" else 256
    if spec.hd != want:
        raise NotImplementedError(
            f"{spec.name}: head_dim {spec.hd} is not implemented by the HIP attention kernels "
            f"(event-level net needs 64, token-level net needs 256)")


def linear_wgrad(dy: torch.Tensor, x: torch.Tensor, dw: torch.Tensor, accumulate: bool):
    """dw[N,K] (+)= dy[M,N]^T @ x[M,K]: the contraction runs over the M rows, i.e. both operands are
    contraction-major as they lie in HBM; the GEMM reads them in that form (split-K over M)."""
    ops.gemm_nt(dy, x, dw, K=dy.shape[0], ta=True, tb=True, beta=1.0 if accumulate else 0.0)


# --------------------------------------------------------------------------------------------------
# training / prefill forward
# --------------------------------------------------------------------------------------------------
class LayerSaved(NamedTuple):
    """what one block keeps for its backward"""
    x: torch.Tensor                 # block input (the residual stream)
    rstd1: torch.Tensor
    h1: Optional[torch.Tensor]      # norm1(x); None in the folded form
    qkv: torch.Tensor
    o: torch.Tensor
    lse: Optional[torch.Tensor]     # event-level stack only
    x2: torch.Tensor                # residual stream after the attention half
    rstd2: torch.Tensor
    h2: Optional[torch.Tensor]      # norm2(x2); None in the folded form
    gu: torch.Tensor
    a: Optional[torch.Tensor]       # SwiGLU activation; None when lean (the backward recomputes it from gu)


class StackSaved(NamedTuple):
    """what stack_forward(save=True) hands to stack_backward"""
    layers: List[Optional[LayerSaved]]   # (a list: stack_backward releases each entry once its layer is done)
    x_last: torch.Tensor                 # input of the final RMSNorm
    rstdf: torch.Tensor
    nseq: int
    slen: int
    folded: Optional[list]               # the folded weights the forward ran with; None: the plain blocks
    first: Optional[tokfirst.TokFirst] = None   # layers[0] is tok_first_forward's (x = [hidden ; E ; E], qkv = its projection)
    seqs: Optional[object] = None               # packed batch: the ops.SeqPlan the forward ran with (nseq / slen are then unused)


def _norm_qkv(spec: StackSpec, lw: LayerTensors, x: torch.Tensor, slen: int, rope: RopeTable, pos0: int, rope_in_attn: bool,
              stats: bool):
    """First half of the plain block up to the attention: RMSNorm -> q|k|v projection, rotated at positions [pos0, pos0 + slen)
    unless ``rope_in_attn``.  ``stats``: the norm also stores rstd.  Returns (h1, rstd1 | None, qkv)."""
    M, D = x.shape
    h1 = _empty((M, D), x)
    rstd1 = _empty((M,), x, torch.float32) if stats else None
    ops.rmsnorm_fwd(x, lw.n1, h1, rstd1, spec.eps)
    qkv = _empty((M, 3 * D), x)
    if not rope_in_attn and ops.rope_fused_ok(h1, spec.hd):
        ops.gemm_rope(h1, lw.wqkv, qkv, rope.fused(), slen, pos0, spec.hd)
    else:
        ops.gemm_nt(h1, lw.wqkv, qkv)
        if not rope_in_attn:
            ops.rope_(qkv, rope.cos, rope.sin, slen, pos0, spec.H, spec.hd, +1)
    return h1, rstd1, qkv


def _attn_fwd_seqs(spec: StackSpec, qkv: torch.Tensor, o: torch.Tensor, rope: RopeTable, seqs) -> torch.Tensor:
    """Packed batch (event-level stack): ``qkv`` comes UNROTATED out of the plain projection -- the tuned GEMM's RoPE epilogue
    takes positions pos0 + row % slen and is left alone -- so RoPE is a pass of its own at the rows' positions within their
    sequences, then ONE attention launch over the sequence table.  Returns lse [H, M]."""
    ops.rope_pos_(qkv, rope.cos, rope.sin, seqs.pos, spec.H, spec.hd, +1)
    lse = _empty((spec.H * qkv.shape[0],), qkv, torch.float32)
    ops.attn_fwd_seqs(qkv, o, lse, seqs, spec.H, spec.scale)
    return lse


def _o_mlp(spec: StackSpec, lw: LayerTensors, x: torch.Tensor, o: torch.Tensor, save: bool, stats: bool):
    """Second half of the plain block, behind the attention: o projection + residual -> RMSNorm -> gate|up projection with
    SwiGLU -> down projection + residual.  ``save``: gate|up is written as well as the activation.  ``stats`` as in _norm_qkv.
    Returns (x3, x2, rstd2 | None, h2, gu | None, a)."""
    M, D = x.shape
    I = spec.I
    x2 = _empty((M, D), x)
    ops.gemm_nt(o, lw.wo, x2, beta=1.0, res=x)
    h2 = _empty((M, D), x)
    rstd2 = _empty((M,), x, torch.float32) if stats else None
    ops.rmsnorm_fwd(x2, lw.n2, h2, rstd2, spec.eps)
    a = _empty((M, I), x)
    gu = None
    if ops.swiglu_fused_ok(h2, I):                  # gate|up projection with SwiGLU as its epilogue
        if save:
            gu = _empty((M, 2 * I), x)
        ops.gemm_swiglu(h2, lw.wgu, gu, a)
    else:
        gu = _empty((M, 2 * I), x)
        ops.gemm_nt(h2, lw.wgu, gu)
        ops.swiglu_fwd(gu, a)
    x3 = _empty((M, D), x)
    ops.gemm_nt(a, lw.wd, x3, beta=1.0, res=x2)
    return x3, x2, rstd2, h2, gu, a


def layer_forward(spec: StackSpec, lw: LayerTensors, x: torch.Tensor, nseq: int, slen: int, rope: RopeTable,
                  kv_out: Optional[list] = None, save: bool = True, lean: bool = False, seqs=None):
    """One pre-norm LLaMA block (LlamaDecoderLayer.forward, TF:models/llama/modeling_llama.py:295-324) on x [nseq*slen, D]:
    RMSNorm -> q|k|v projection -> RoPE -> causal attention -> o projection + residual -> RMSNorm -> gate|up projection with
    SwiGLU epilogue -> down projection + residual.  7 launches for the event-level stack in bf16, where RoPE rides on the q|k|v
    projection (8 where it is a launch of its own; bench.py --mode block times exactly this function).  ``save=False`` is the
    forward-only form (prompt prefill, validation): gate|up is never written, only the activation.  ``lean`` (with save): the
    SwiGLU activation ``a`` is not kept -- the backward recomputes it from the
    stored gate|up with mh_swiglu_fwd, bit for bit (the fused epilogue and that kernel share their roundings) -- which takes
    I of the 8 D + 3 I saved elements per row off the activation memory (the 2x-hidden large shape at 16 x 4096 per GPU: 39 GB).
    ``seqs`` (event-level stack): the rows are a packed batch -- see _attn_fwd_seqs.
    Returns (block output, LayerSaved | None)."""
    M, D = x.shape
    H = spec.H
    # token-level stack: RoPE is applied inside the attention kernels (q,k of a (sequence, head) are in registers
    # there anyway), so qkv stays unrotated -- except for a prefill, whose K rows go to the cache rotated.
    # event-level stack (heads of 64): RoPE rides on the q|k|v projection's epilogue.
    rope_in_attn = spec.kind != "event" and kv_out is None
    h1, rstd1, qkv = _norm_qkv(spec, lw, x, slen, rope, 0, rope_in_attn or seqs is not None, stats=True)
    o = _empty((M, D), x)
    lse = None
    if seqs is not None:
        lse = _attn_fwd_seqs(spec, qkv, o, rope, seqs)
    elif spec.kind == "event":
        lse = _empty((nseq * H * ops.round_up(slen, 64),), x, torch.float32)
        ops.attn_fwd(qkv, o, lse, nseq, slen, H, spec.scale)
    elif rope_in_attn:
        ops.tokattn_fwd(qkv, o, nseq, slen, H, spec.scale, rope.cos, rope.sin)
    else:
        ops.tokattn_fwd(qkv, o, nseq, slen, H, spec.scale)
    if kv_out is not None:
        kv_out.append(qkv)
    x3, x2, rstd2, h2, gu, a = _o_mlp(spec, lw, x, o, save, stats=True)
    return x3, (LayerSaved(x, rstd1, h1, qkv, o, lse, x2, rstd2, h2, gu, None if lean else a) if save else None)


# The forward-only event-level block with both RMSNorms folded around its projections (r05): below these row counts the two
# extra ~3 us statistics launches (and, without pre-folded weights, the fold itself: ~20 us per layer of elementwise work) cost more
# than the two norm passes they replace (2 x 44 us at 65536 rows, proportional to the rows).
FOLD_MIN_ROWS_PREFOLDED = 8192
FOLD_MIN_ROWS_ON_THE_FLY = 131072   # (12 layers: the fold ~0.7 ms of elementwise launches against ~14 us saved per layer and 8192 rows)


def layer_forward_folded(spec: StackSpec, lw: LayerTensors, fold, x: torch.Tensor, nseq: int, slen: int, rope: RopeTable,
                         parts_in: Optional[torch.Tensor], kv_out: Optional[list] = None, saved_out: Optional[list] = None,
                         lean: bool = False, seqs=None):
    """layer_forward without its two RMSNorm passes (LlamaDecoderLayer.forward, TF:models/llama/modeling_llama.py:295-324;
    LlamaRMSNorm :62-67): ``fold`` = (wqkv * n1, wgu * n2) from fold_norm_weights, so norm(x) W^T = rstd (.) (x W'^T) and the
    normalised activations h1 / h2 are never written, read or kept (training: a fifth of the saved activations less per layer).
    The row statistics come out of the PRODUCING projections: the
    o and down projections (mh_gemm_rowss) leave per-64-column sums of squares of the rows they store (``parts`` [D/64, M]),
    mh_row_rstd turns them into rstd (one tiny launch), the q|k|v + RoPE and gate|up + SwiGLU projections apply it to their
    fp32 accumulators before their own epilogue arithmetic.  7 launches, none of them a pass over the residual stream.
    ``parts_in``: the statistics of ``x`` left by the previous block's down projection (None: computed from x itself).
    ``saved_out`` (training, r06; a list as ``kv_out`` is): receives the block's LayerSaved for layer_backward_folded, ``lean`` as in
    layer_forward; gate|up is written, and each half gets its own rstd.  The token-level stack takes this form in training only:
    RoPE stays inside its attention kernel, the q|k|v projection is the plain GEMM with a row scale.
    Returns (block output, its parts)."""
    M, D = x.shape
    H, I = spec.H, spec.I
    save = saved_out is not None
    wq_n, wgu_n = fold
    rstd1 = _empty((M,), x, torch.float32)
    if parts_in is not None:
        ops.row_rstd(rstd1, D, spec.eps, parts=parts_in)
    else:
        ops.row_rstd(rstd1, D, spec.eps, x=x)
    qkv = _empty((M, 3 * D), x)
    o = _empty((M, D), x)
    lse = None
    if seqs is not None:   # packed batch: the plain scaled projection, then _attn_fwd_seqs
        ops.gemm_nt_scaled(x, wq_n, qkv, rstd1)
        lse = _attn_fwd_seqs(spec, qkv, o, rope, seqs)
    elif spec.kind == "event":
        ops.gemm_rope(x, wq_n, qkv, rope.fused(), slen, 0, spec.hd, rowscale=rstd1)
        lse = _empty((nseq * H * ops.round_up(slen, 64),), x, torch.float32)
        ops.attn_fwd(qkv, o, lse, nseq, slen, H, spec.scale)
    else:
        ops.gemm_nt_scaled(x, wq_n, qkv, rstd1)
        ops.tokattn_fwd(qkv, o, nseq, slen, H, spec.scale, rope.cos, rope.sin)
    if kv_out is not None:
        kv_out.append(qkv)
    x3, parts3, x2, rstd2, gu, a = _folded_o_mlp(spec, lw, wgu_n, x, o, rstd1, save)
    if save:
        saved_out.append(LayerSaved(x, rstd1, None, qkv, o, lse, x2, rstd2, None, gu, None if lean else a))
    return x3, parts3


def _folded_o_mlp(spec: StackSpec, lw: LayerTensors, wgu_n: torch.Tensor, x: torch.Tensor, o: torch.Tensor, rstd1: torch.Tensor,
                  save: bool):
    """Second half of the folded block, behind the attention: o projection + residual ``x`` with the row statistics of what it
    stores -> rstd -> gate|up projection on the folded weights with the row scale and SwiGLU -> down projection + residual with
    statistics.  Returns (x3, its parts, x2, rstd2, gu | None, a)."""
    M, D = x.shape
    I = spec.I
    parts = _empty((D // 64, M), x, torch.float32)
    x2 = _empty((M, D), x)
    ops.gemm_rowss(o, lw.wo, x2, parts, res=x)
    # forward-only: one rstd and one parts buffer serve both halves
    rstd2 = _empty((M,), x, torch.float32) if save else rstd1
    ops.row_rstd(rstd2, D, spec.eps, parts=parts)
    gu = _empty((M, 2 * I), x) if save else None
    a = _empty((M, I), x)
    ops.gemm_swiglu(x2, wgu_n, gu, a, rowscale=rstd2)
    parts3 = _empty((D // 64, M), x, torch.float32) if save else parts
    x3 = _empty((M, D), x)
    ops.gemm_rowss(a, lw.wd, x3, parts3, res=x2)
    return x3, parts3, x2, rstd2, gu, a


def tok_first_forward(spec: StackSpec, lw: LayerTensors, fold, first: tokfirst.TokFirst, x: torch.Tensor, nseq: int,
                      rope: RopeTable, saved_out: list, lean: bool = False):
    """layer_forward_folded (training form) for the FIRST block of the token-level stack, whose input rows ``x`` [nseq * 8, D] are
    row 8n = first.hidden[n] and rows 8n + p = first.table[first.ids[n, p - 1]] (ops.concat_tok_fwd): the norm statistics and the
    q|k|v projection run once over x_cat = [hidden ; table] -- nseq + V rows instead of 8 nseq -- and the attention kernel takes
    its rows through the ids (tokfirst.tokattn_fwd_rows).  Same GEMM entry, same K loop, and a row's product does not depend on
    the tile it falls in: every q|k|v value, hence ``o`` and everything behind it, equals the dense schedule's bit for bit.
    The buffer is [hidden ; table ; table] (nseq + 2 V rows): the backward's weight gradient contracts [dz_h ; S_hi ; S_lo]
    against it, and the row-scaled projection, which takes its rows in groups of 4, runs over round_up(nseq + V, 4) of them.
    LayerSaved keeps x = that buffer and qkv = its projection in place of the [8 nseq, .] ones.  Returns (block output, its parts)."""
    N, D = first.hidden.shape
    V = first.table.shape[0]
    H = spec.H
    assert N == nseq and x.shape == (N * tokfirst.TN, D) and first.table.shape[1] == D
    wq_n, wgu_n = fold
    Mf = ops.round_up(N + V, 4)
    xc = _empty((N + 2 * V, D), x)
    xc[:N].copy_(first.hidden)
    xc[N:N + V].copy_(first.table)
    xc[N + V:].copy_(first.table)
    rstd_c = _empty((Mf,), x, torch.float32)
    ops.row_rstd(rstd_c, D, spec.eps, x=xc[:Mf])
    zc = _empty((Mf, 3 * D), x)
    ops.gemm_nt_scaled(xc[:Mf], wq_n, zc, rstd_c)
    o = _empty((N * tokfirst.TN, D), x)
    tokfirst.tokattn_fwd_rows(zc, first.ids, N, V, o, N, H, spec.scale, rope.cos, rope.sin)
    x3, parts3, x2, rstd2, gu, a = _folded_o_mlp(spec, lw, wgu_n, x, o, rstd_c, True)
    saved_out.append(LayerSaved(xc, rstd_c, None, zc, o, None, x2, rstd2, None, gu, None if lean else a))
    return x3, parts3


def train_fold_ok(spec: StackSpec, x: torch.Tensor) -> bool:
    """whether the TRAINING forward / backward of stack ``spec`` over the rows ``x`` can run with its RMSNorms folded around
    the projections (layer_forward_folded / layer_backward_folded): bf16 on the production GEMM with its K-step-64 loops,
    the fused SwiGLU epilogues in both directions, whole 64-column statistics chunks, 4-row groups, and -- event-level stack --
    the RoPE epilogue and the one-call attention backward"""
    ok = (x.dtype == torch.bfloat16 and ops.swiglu_fused_ok(x, spec.I) and ops.dswiglu_ok(x, spec.I) and spec.D % 64 == 0
          and x.shape[0] % 4 == 0 and ops.get_option("gemm_k64") == 1 and os.environ.get("MH_NORM_FOLD_TRAIN", "1") != "0")
    if ok and spec.kind == "event":
        ok = ops.rope_fused_ok(x, spec.hd) and ops.attn_bwd_scaled_ok(x)
    return ok


def runs_folded(spec: StackSpec, x: torch.Tensor, save: bool, kv_out: Optional[list], fold_kept: bool) -> bool:
    """Whether stack_forward over the rows ``x`` runs the folded blocks -- the one place that decides it; ``fold_kept``: the caller
    has (or would pass) folded weights it keeps current.  A training forward (``save``) folds only with kept weights -- the backward
    needs this step's -- and where train_fold_ok holds; a forward-only pass of the event-level stack folds from
    FOLD_MIN_ROWS_PREFOLDED rows up with kept weights, and from FOLD_MIN_ROWS_ON_THE_FLY up without, deriving them per call."""
    if save:
        return fold_kept and kv_out is None and train_fold_ok(spec, x)
    return (spec.kind == "event" and x.shape[0] >= (FOLD_MIN_ROWS_PREFOLDED if fold_kept else FOLD_MIN_ROWS_ON_THE_FLY)
            and ops.norm_fold_ok(x, spec.D, spec.hd, spec.I))


def layer_backward(spec: StackSpec, lw: LayerTensors, lg: LayerTensors, keep: LayerSaved, dx: torch.Tensor, nseq: int, slen: int,
                   rope: RopeTable, accumulate: bool, seqs=None) -> torch.Tensor:
    """The backward of layer_forward: dx = d loss / d block output -> d loss / d block input (written over ``dx``), the layer's
    parameter gradients to ``lg``."""
    M, D = dx.shape
    H, I = spec.H, spec.I
    # ---- MLP ----
    a = keep.a
    if a is None:                                   # lean forward: a = round(silu(gate)) * up again, from the stored gate|up
        a = _empty((M, I), dx)
        ops.swiglu_fwd(keep.gu, a)
    dgu = _empty((M, 2 * I), dx)
    if ops.dswiglu_ok(dx, I):                       # d a = dx @ wd with the SwiGLU backward as its epilogue
        ops.gemm_dswiglu(dx, lw.wd, keep.gu, dgu)
    else:
        da = _empty((M, I), dx)
        ops.gemm_nt(dx, lw.wd, da, tb=True)         # d a = dx @ wd      (wd [D, I] read contraction-major)
        ops.swiglu_bwd(keep.gu, da, dgu)
        del da
    linear_wgrad(dx, a, lg.wd, accumulate)
    del a
    dh2 = _empty((M, D), dx)
    ops.gemm_nt(dgu, lw.wgu, dh2, tb=True)          # d h2 = dgu @ wgu
    linear_wgrad(dgu, keep.h2, lg.wgu, accumulate)
    del dgu
    dx2 = _empty((M, D), dx)
    ops.rmsnorm_bwd(keep.x2, lw.n2, keep.rstd2, dh2, dx, dx2, lg.n2, accumulate)
    # ---- attention ----
    do = dh2                                        # reuse
    ops.gemm_nt(dx2, lw.wo, do, tb=True)            # d o = dx2 @ wo
    linear_wgrad(dx2, keep.o, lg.wo, accumulate)
    dqkv = _empty((M, 3 * D), dx)
    if seqs is not None:  # (packed batch: rotated back in the stores at row - start of its sequence)
        ops.attn_bwd_seqs(keep.qkv, keep.o, do, keep.lse, dqkv, seqs, H, spec.scale, rope.cos, rope.sin)
    elif spec.kind == "event":
        ops.attn_bwd(keep.qkv, keep.o, do, keep.lse, dqkv, nseq, slen, H, spec.scale, rope.cos, rope.sin)  # (rotated back in the stores)
    else:  # (saved qkv is unrotated: the forward ran with save=True, never as a prefill)
        ops.tokattn_bwd(keep.qkv, do, dqkv, nseq, slen, H, spec.scale, rope.cos, rope.sin)
    dh1 = do
    ops.gemm_nt(dqkv, lw.wqkv, dh1, tb=True)        # d h1 = dqkv @ wqkv
    linear_wgrad(dqkv, keep.h1, lg.wqkv, accumulate)
    del dqkv
    ops.rmsnorm_bwd(keep.x, lw.n1, keep.rstd1, dh1, dx2, dx, lg.n1, accumulate)
    return dx


def layer_backward_folded(spec: StackSpec, lw: LayerTensors, lg: LayerTensors, fold, keep: LayerSaved, dx: torch.Tensor, nseq: int,
                          slen: int, rope: RopeTable, accumulate: bool, seqs=None) -> torch.Tensor:
    """The backward of layer_forward_folded.  With z = x W'^T, y = rstd (.) z: the producers of d y store d z = rstd (.) d y
    (the SwiGLU-backward epilogue, the attention backward's stores), t = d z W' is the dgrad on the folded weights,
    dx = t - x (rstd^2 / D) rowdot(t, x) + dres the norm's backward without its weight, and the weight gradient G' = d z^T x
    turns into dW = G' (.) w and dw = colsum(G' (.) W) inside its split-K reduction (ops.wgrad_folded)."""
    M, D = dx.shape
    H = spec.H
    wq_n, wgu_n = fold
    # Event-level stack: the block's four weight gradients contract over the same M rows and their 256 x 256 tiles add up to the
    # CU count at the benchmarked shape, so they wait in ``pend`` (with the operands they keep alive: d z2, a, dx2, d z1) and go
    # out as ONE grouped launch without split-K (ops.wgrad_grouped).  The token-level stack (112 tiles per layer at a contraction
    # of 8 x the rows: split-K fills the chip, a group would not) and the packed-batch path keep one launch per gradient.
    I = spec.I
    pend = None
    if spec.kind == "event" and seqs is None and ops.wgrad_grouped_ok([(D, I), (2 * I, D), (D, D), (3 * D, D)], M, dx):
        pend = []
    dx2, do = _folded_mlp_o_backward(spec, lw, lg, wgu_n, keep, dx, accumulate, pend)
    dz1 = _empty((M, 3 * D), dx)
    if seqs is not None:
        ops.attn_bwd_seqs(keep.qkv, keep.o, do, keep.lse, dz1, seqs, H, spec.scale, rope.cos, rope.sin, rowscale=keep.rstd1)
    elif spec.kind == "event":
        ops.attn_bwd(keep.qkv, keep.o, do, keep.lse, dz1, nseq, slen, H, spec.scale, rope.cos, rope.sin, rowscale=keep.rstd1)
    else:
        ops.tokattn_bwd(keep.qkv, do, dz1, nseq, slen, H, spec.scale, rope.cos, rope.sin, rowscale=keep.rstd1)
    t1 = do
    ops.gemm_nt(dz1, wq_n, t1, tb=True)                      # t1 = d z1 @ W'qkv
    if pend is not None:
        pend.append((dz1, keep.x, lg.wqkv, (lw.n1, lw.wqkv, lg.n1)))
        ops.wgrad_grouped(pend, accumulate)                  # (before the norm backward below overwrites dx, the down projection's operand)
        pend.clear()
    else:
        ops.wgrad_folded(dz1, keep.x, lg.wqkv, lw.n1, lw.wqkv, lg.n1, accumulate)
    del dz1
    ops.rmsnorm_bwd_folded(keep.x, keep.rstd1, t1, dx2, dx)
    return dx


def _folded_mlp_o_backward(spec: StackSpec, lw: LayerTensors, lg: LayerTensors, wgu_n: torch.Tensor, keep: LayerSaved,
                           dx: torch.Tensor, accumulate: bool, pend: Optional[list] = None):
    """The folded block's backward from its output down to the attention: the MLP half, then the o projection.
    Returns (dx2 = the gradient of the residual stream between the halves, do = the gradient of the attention output).
    ``pend`` (a list): the three weight gradients are not launched but appended to it as ops.wgrad_grouped problems; the caller
    launches them before it overwrites ``dx``."""
    M, D = dx.shape
    I = spec.I
    # ---- MLP ----
    a = keep.a
    if a is None:
        a = _empty((M, I), dx)
        ops.swiglu_fwd(keep.gu, a)
    dz2 = _empty((M, 2 * I), dx)
    ops.gemm_dswiglu(dx, lw.wd, keep.gu, dz2, rowscale=keep.rstd2)     # rstd2 (.) SwiGLU'(gate|up) (dx @ wd)
    if pend is not None:
        pend.append((dx, a, lg.wd, None))
    else:
        linear_wgrad(dx, a, lg.wd, accumulate)
    del a
    t2 = _empty((M, D), dx)
    ops.gemm_nt(dz2, wgu_n, t2, tb=True)                     # t2 = d z2 @ W'gu
    if pend is not None:
        pend.append((dz2, keep.x2, lg.wgu, (lw.n2, lw.wgu, lg.n2)))
    else:
        ops.wgrad_folded(dz2, keep.x2, lg.wgu, lw.n2, lw.wgu, lg.n2, accumulate)
    del dz2
    dx2 = _empty((M, D), dx)
    ops.rmsnorm_bwd_folded(keep.x2, keep.rstd2, t2, dx, dx2)
    # ---- attention ----
    do = t2                                                  # reuse
    ops.gemm_nt(dx2, lw.wo, do, tb=True)
    if pend is not None:
        pend.append((dx2, keep.o, lg.wo, None))
    else:
        linear_wgrad(dx2, keep.o, lg.wo, accumulate)
    return dx2, do


class TokFirstGrads(NamedTuple):
    """what tok_first_backward hands back in place of the gradient of the [8 N, D] input rows"""
    dhidden: torch.Tensor   # [N, D] gradient of first.hidden
    dtable32: torch.Tensor  # [V, D] fp32 gradient of first.table (row pad_id zero)


def tok_first_backward(spec: StackSpec, lw: LayerTensors, lg: LayerTensors, fold, keep: LayerSaved, first: tokfirst.TokFirst,
                       dx: torch.Tensor, nseq: int, rope: RopeTable, accumulate: bool) -> TokFirstGrads:
    """The backward of tok_first_forward.  Down to d z1 (the attention backward's stores, rows through the ids) it is
    layer_backward_folded.  The rest is linear in d z1 for fixed inputs, and rows 8n + p (p >= 1) have one of V inputs, so with
    S_v = the sum of d z1 over the rows whose input is table row v (pad id included: a pad in mid-sequence carries gradient
    into W'), kept as two bf16 terms hi + lo (S to ~2^-17):
      t_cat = [dz_h ; S_hi ; S_lo] W'                                (one dgrad over N + 2 V rows)
      G'    = [dz_h ; S_hi ; S_lo]^T [hidden ; E ; E]                (one folded weight gradient, contraction N + 2 V)
      d hidden = rmsnorm_bwd_folded(hidden, rstd_h, t_h, dres rows 8n)
      d E_v = (T_hi + T_lo)_v - e_v (rstd_v^2 / D) rowdot(T_v, e_v) + the sum of dres over v's rows  (pad row: zero)
    where dres = the gradient of the residual stream between the halves.  The occurrence lists are made once and serve both
    segment sums; S is summed in a fixed order (tokfirst.occurrence_lists), without the atomics the embedding gradient allows
    itself, because it reaches the weight gradients."""
    M, D = dx.shape
    H, T = spec.H, tokfirst.TN
    N, V = first.hidden.shape[0], first.table.shape[0]
    assert N == nseq and M == N * T
    wq_n, wgu_n = fold
    xc, rstd_c, zc = keep.x, keep.rstd1, keep.qkv
    dres, do = _folded_mlp_o_backward(spec, lw, lg, wgu_n, keep, dx, accumulate)
    dz = _empty((M, 3 * D), dx)                              # (rows 8n stay unwritten: they go to dzc[:N])
    dzc = _empty((N + 2 * V, 3 * D), dx)                     # [dz_h ; S_hi ; S_lo]
    tokfirst.tokattn_bwd_rows(zc, first.ids, N, V, do, dz, dzc[:N], rstd_c, N, H, spec.scale, rope.cos, rope.sin)
    del do
    # row 8n + p per occurrence, in a fixed order: S feeds weight gradients and must not vary from run to run
    src, seg, vseg, vstart = tokfirst.occurrence_lists(first.ids[:, : T - 1], V, T, 1)
    S = _empty((V, 3 * D), dx, torch.float32)
    tokfirst.segment_sum_fixed_order(src, vseg, vstart, dz, S)
    del dz
    tokfirst.split_hi_lo(S, dzc[N:N + V], dzc[N + V:])
    del S
    tc = _empty((N + 2 * V, D), dx)
    ops.gemm_nt(dzc, wq_n, tc, tb=True)                      # t_cat = [dz_h ; S_hi ; S_lo] @ W'qkv
    ops.wgrad_folded(dzc, xc, lg.wqkv, lw.n1, lw.wqkv, lg.n1, accumulate)
    del dzc
    dres_h = _empty((N, D), dx)
    ops.copy_rows(dres, T * D, dres_h, D, N, D)
    dhid = _empty((N, D), dx)
    ops.rmsnorm_bwd_folded(xc[:N], rstd_c[:N], tc[:N], dres_h, dhid)
    acc32 = torch.zeros((V, D), dtype=torch.float32, device=dx.device)
    ops.embed_segment_bwd(src, seg, dres, D, acc32, first.pad_id)
    tokfirst.table_norm_bwd(tc[N:N + V], tc[N + V:], xc[N:N + V], rstd_c[N:N + V], acc32, first.pad_id)
    return TokFirstGrads(dhid, acc32)


def stack_forward(spec: StackSpec, W: StackTensors, x: torch.Tensor, nseq: int, slen: int, rope: RopeTable,
                  save: bool, kv_out: Optional[list] = None, lean: bool = False, folded=None,
                  first: Optional[tokfirst.TokFirst] = None, seqs=None):
    """x [nseq*slen, D] (inputs_embeds) -> (last_hidden_state [nseq*slen, D], StackSaved | None).
    save=True keeps what the backward needs (``lean``: minus the SwiGLU activations, recomputed in the backward);
    kv_out (prefill) receives each layer's post-RoPE qkv.  runs_folded picks the blocks: plain (layer_forward) or with the
    RMSNorms folded (layer_forward_folded).  ``folded`` = fold_norm_weights(W) kept current by the caller (a decode session's;
    MIDIModel.folded_weights, re-derived after every update -- the training forward takes no other, and the backward finds them
    in the context); a forward-only pass without one makes the fold here, from the live weights, per call.
    ``first`` (token-level stack, training): what the rows ``x`` were laid out from; where the folded training blocks run and
    tokfirst.table_first_ok holds, the first block takes tok_first_forward and stack_backward returns TokFirstGrads.
    ``seqs`` (event-level stack, training / validation): an uploaded ops.SeqPlan -- the rows are a PACKED batch, sequences of any
    lengths laid end to end (data.PackedBatch); ``nseq`` / ``slen`` are then 1 / M and only the attention and RoPE see the table.
    With ``kv_out`` it is a ragged prefill (stack_prefill_seqs): the qkv handed out are rotated at the rows' own positions."""
    _check_heads(spec)
    M, D = x.shape
    assert M == nseq * slen
    if seqs is not None:
        assert spec.kind == "event" and first is None and seqs.M == M and seqs.H == spec.H
        rope.ensure(seqs.max_len)
    else:
        rope.ensure(slen)
    if runs_folded(spec, x, save, kv_out, folded is not None):
        if folded is None:
            folded = fold_norm_weights(W)
    else:
        folded = None
    saved = [] if save else None
    parts = None
    if not (save and folded is not None and tokfirst.table_first_ok(spec, first, slen)):
        first = None
    for li, lw in enumerate(W.layers):
        if first is not None and li == 0:
            x, parts = tok_first_forward(spec, lw, folded[li], first, x, nseq, rope, saved, lean)
        elif folded is not None:
            x, parts = layer_forward_folded(spec, lw, folded[li], x, nseq, slen, rope, parts, kv_out, saved, lean, seqs)
        else:
            x, keep = layer_forward(spec, lw, x, nseq, slen, rope, kv_out, save, lean and save, seqs)
            if save:
                saved.append(keep)
    y = _empty((M, D), x)
    # (the forward-only folded pass is the one form that asks the final norm for no rstd)
    rstdf = _empty((M,), x, torch.float32) if save or folded is None else None
    ops.rmsnorm_fwd(x, W.norm, y, rstdf, spec.eps)
    return y, (StackSaved(saved, x, rstdf, nseq, slen, folded, first, seqs) if save else None)


def stack_backward(spec: StackSpec, W: StackTensors, G: StackTensors, ctx: StackSaved, dy: torch.Tensor,
                   rope: RopeTable, accumulate: bool, on_layer_done: Optional[Callable[[int], None]] = None):
    """dy = d loss / d last_hidden_state  ->  d loss / d inputs_embeds; parameter gradients go to G
    (overwritten, or added to when `accumulate`).  `on_layer_done(i)` fires when layer i's gradients are
    final (layers finish in reverse order) — the data-parallel reducer hangs its bucket launches on it.
    Where the forward ran tok_first_forward (ctx.first) the result is TokFirstGrads: the gradients of the hidden states and of
    the embedding table the input rows were laid out from."""
    M, D = dy.shape
    dx = _empty((M, D), dy)
    ops.rmsnorm_bwd(ctx.x_last, W.norm, ctx.rstdf, dy, None, dx, G.norm, accumulate)
    for li in range(len(W.layers) - 1, -1, -1):
        lw, lg = W.layers[li], G.layers[li]
        if ctx.first is not None and li == 0:
            dx = tok_first_backward(spec, lw, lg, ctx.folded[li], ctx.layers[li], ctx.first, dx, ctx.nseq, rope, accumulate)
        elif ctx.folded is not None:
            dx = layer_backward_folded(spec, lw, lg, ctx.folded[li], ctx.layers[li], dx, ctx.nseq, ctx.slen, rope, accumulate, ctx.seqs)
        else:
            dx = layer_backward(spec, lw, lg, ctx.layers[li], dx, ctx.nseq, ctx.slen, rope, accumulate, ctx.seqs)
        ctx.layers[li] = None                           # activations are released back to front
        if on_layer_done is not None:
            on_layer_done(li)
    return dx


# --------------------------------------------------------------------------------------------------
# KV-cached decode (one new position per sequence)
# --------------------------------------------------------------------------------------------------
class KVState:
    """Preallocated per-layer K/V buffers [B,H,Lmax,hd] replacing DynamicCache's torch.cat growth
    (TF:cache_utils.py:127-147).  Attached to whatever cache object the caller passes (app.py hands us
    HF DynamicCache instances it created itself, app.py:56,64)."""

    def __init__(self, spec: StackSpec, B: int, capacity: int, like: torch.Tensor):
        self.spec, self.B, self.cap, self.len = spec, B, capacity, 0
        shape = (spec.L, B, spec.H, capacity, spec.hd)
        self.k = torch.empty(shape, dtype=like.dtype, device=like.device)
        self.v = torch.empty(shape, dtype=like.dtype, device=like.device)

    def reserve(self, need: int):
        if need <= self.cap:
            return
        cap = max(need, 2 * self.cap)
        for nm in ("k", "v"):
            old = getattr(self, nm)
            new = torch.empty((self.spec.L, self.B, self.spec.H, cap, self.spec.hd), dtype=old.dtype, device=old.device)
            new[:, :, :, : self.len].copy_(old[:, :, :, : self.len])
            setattr(self, nm, new)
        self.cap = cap


class KVStateQ:
    """The event-level cache in 8 bits (DecodeSession(kv_dtype="fp8"); attention_kvq.hip): per layer ``k8`` / ``v8``
    uint8 [B, H, cap, 64] hold e4m3fn codes and ``sc`` float32 [B, H, cap, 2] the (K scale, V scale) of every (row, head, event) --
    136 bytes per head and event where KVState holds 256.  Never grown: a captured graph holds its addresses.  Served by
    stack_prefill_seqs(rows=...) and by the fused per-row attention of stack_decode(row_pos=...) alone; every other form refuses it."""

    def __init__(self, spec: StackSpec, B: int, capacity: int, like: torch.Tensor):
        if spec.kind != "event" or spec.hd != 64 or like.dtype != torch.bfloat16:
            raise ValueError(f"KVStateQ: the fp8 cache serves the event-level stack (head_dim 64) of a bf16 model: {spec.kind}, "
                             f"head_dim {spec.hd}, {like.dtype}")
        self.spec, self.B, self.cap, self.len = spec, B, capacity, 0
        shape = (spec.L, B, spec.H, capacity)
        self.k8 = torch.empty(shape + (spec.hd,), dtype=torch.uint8, device=like.device)
        self.v8 = torch.empty(shape + (spec.hd,), dtype=torch.uint8, device=like.device)
        self.sc = torch.empty(shape + (2,), dtype=torch.float32, device=like.device)

    def nbytes(self) -> int:
        return self.k8.numel() + self.v8.numel() + 4 * self.sc.numel()


def _refuse_kvq(kv, what: str) -> None:
    if isinstance(kv, KVStateQ):
        raise ValueError(f"{what}: the fp8 K/V cache is served by stack_prefill_seqs(rows=...) and the fused per-row attention of "
                         "stack_decode(row_pos=...) only")


def stack_prefill(spec: StackSpec, W: StackTensors, x: torch.Tensor, nseq: int, slen: int, rope: RopeTable, kv: KVState,
                  folded=None):
    """Causal forward over a whole prompt from an EMPTY cache, storing K/V rows [0, slen)."""
    _refuse_kvq(kv, "stack_prefill")
    assert kv.len == 0
    kv.reserve(slen)
    qkvs: list = []
    y, _ = stack_forward(spec, W, x, nseq, slen, rope, save=False, kv_out=qkvs, folded=folded)
    for li, qkv in enumerate(qkvs):
        ops.kv_store_prefill(qkv, kv.k[li], kv.v[li], nseq, slen, spec.H, spec.hd, kv.cap)
    kv.len = slen
    return y


def stack_prefill_seqs(spec: StackSpec, W: StackTensors, x: torch.Tensor, plan, rope: RopeTable, kv: KVState, folded=None,
                       rows=None, rows_dev=None):
    """stack_prefill for prompts of DIFFERENT lengths (generate_ragged): ``x`` [M, D] holds plan.n sequences laid end to end
    (``plan`` = an uploaded ops.SeqPlan), sequence s fills rows [0, L_s) of its own cache -- one packed forward, then one
    kv_store_seqs launch per layer.  kv.len is left alone: the rows stand at different positions, which the caller keeps
    (a ragged decode session: ``pos`` on the device).
    ``rows`` (DecodeSession.admit; a sequence of plan.n distinct ints inside [0, kv.B), ``rows_dev`` its int32 device copy):
    sequence s fills rows [0, L_s) of cache sequence rows[s] of a cache that is IN USE -- kv.B may exceed plan.n, the cache is not
    grown (a captured graph holds its address), and the other sequences are not touched: one kv_store_seqs_rows launch per layer.
    ``kv`` a ``KVStateQ`` (``rows`` only, bf16): that launch is kv_store_seqs_rows_fp8, which quantizes what it stores."""
    assert plan.M == x.shape[0]
    quant = isinstance(kv, KVStateQ)  # the fp8 cache: the store quantizes (one mh_kv_store_seqs_rows_fp8 per layer)
    if quant and rows is None:
        _refuse_kvq(kv, "stack_prefill_seqs without rows")
    if quant and x.dtype != torch.bfloat16:
        raise ValueError(f"stack_prefill_seqs: the fp8 K/V cache takes bf16 activations, not {x.dtype}")
    if rows is None:
        assert kv.B == plan.n
        kv.reserve(plan.max_len)
    else:
        assert plan.n <= kv.B
        if plan.max_len > kv.cap:
            raise ValueError(f"stack_prefill_seqs: a sequence of {plan.max_len} rows into a live cache of {kv.cap}")
    qkvs: list = []
    y, _ = stack_forward(spec, W, x, 1, plan.M, rope, save=False, kv_out=qkvs, folded=folded, seqs=plan)
    for li, qkv in enumerate(qkvs):
        if quant:
            ops.kv_store_seqs_rows_fp8(qkv, plan, rows, kv.k8[li], kv.v8[li], kv.sc[li], spec.H, spec.hd, kv.cap, rows_dev=rows_dev)
        elif rows is None:
            ops.kv_store_seqs(qkv, plan, kv.k[li], kv.v[li], spec.H, spec.hd, kv.cap)
        else:
            ops.kv_store_seqs_rows(qkv, plan, rows, kv.k[li], kv.v[li], spec.H, spec.hd, kv.cap, rows_dev=rows_dev)
    return y


def stack_extend(spec: StackSpec, W: StackTensors, x: torch.Tensor, nseq: int, slen: int, rope: RopeTable, kv: KVState):
    """A chunk of ``slen`` > 1 new positions per sequence behind ``kv.len`` cached ones (a cache-carrying forward with q_len > 1:
    chunked prefill, TF:models/llama/modeling_llama.py:386-389 position offset + TF:integrations/sdpa_attention.py:79-166).
    Per layer the plain block's two halves (_norm_qkv, _o_mlp) around a different middle: the chunk's q|k|v projection rotated at
    positions [n, n + slen), K/V appended to the cache, the cached K/V rows gathered in front of the chunk's rows, and the flash
    forward over the n + slen rows computing the chunk's query tiles only -- the same 11 launches per layer in bf16 (7 of the
    block, K/V store and gather, two torch copies: the chunk's rows into the gathered buffer and its outputs out of the
    attention's) whatever ``slen`` is (the event-by-event form this replaces took 5 x slen).  Event-level stack (heads of 64)."""
    _check_heads(spec)
    _refuse_kvq(kv, "stack_extend")
    assert spec.kind == "event"
    M, D = x.shape
    assert M == nseq * slen
    n, H, hd = kv.len, spec.H, spec.hd
    stot = n + slen
    kv.reserve(stot)
    rope.ensure(stot)
    for li, lw in enumerate(W.layers):
        _, _, qkv = _norm_qkv(spec, lw, x, slen, rope, n, rope_in_attn=False, stats=False)
        ops.kv_store_rows(qkv, kv.k[li], kv.v[li], nseq, slen, H, hd, kv.cap, n)
        full = _empty((nseq * stot, 3 * D), x)
        ops.kv_gather_rows(kv.k[li], kv.v[li], full, nseq, n, stot, H, hd, kv.cap)
        full.view(nseq, stot, 3 * D)[:, n:].copy_(qkv.view(nseq, slen, 3 * D))
        o_full = _empty((nseq * stot, D), x)
        lse = _empty((nseq * H * ops.round_up(stot, 64),), x, torch.float32)
        ops.attn_fwd_tail(full, o_full, lse, nseq, stot, H, spec.scale, n)
        o = o_full.view(nseq, stot, D)[:, n:].reshape(M, D)
        x = _o_mlp(spec, lw, x, o, save=False, stats=False)[0]
    kv.len = stot
    y = _empty((M, D), x)
    ops.rmsnorm_fwd(x, W.norm, y, None, spec.eps)
    return y


def fold_norm_weights(W: StackTensors, out=None):
    """[(wqkv * n1, wgu * n2) per layer]: the RMSNorm weights folded into the projections that follow them, for the
    decode path's one-launch norm + projection (mh_gemm_skinny with norm_eps).  Derived data: with ``out`` (a list this
    function returned earlier) the copies are rewritten in place, which is how a decode session follows weight updates."""
    if out is None:
        out = _FoldList((torch.empty_like(lw.wqkv), torch.empty_like(lw.wgu)) for lw in W.layers)
    if W.layers and W.layers[0].wqkv.is_cuda and all(lw.wqkv.is_contiguous() and lw.wgu.is_contiguous() for lw in W.layers):
        # ONE launch for the whole stack (the training step re-derives the fold after every optimizer step): the job table is
        # built once per list -- the matrices are views of the flat parameter buffer and the copies are rewritten in place
        jobs = getattr(out, "jobs", None)
        key = (W.layers[0].wqkv.data_ptr(), out[0][0].data_ptr())
        if jobs is None or jobs[0] != key:
            trip = []
            for lw, (fq, fg) in zip(W.layers, out):
                trip += [(lw.wqkv, lw.n1, fq), (lw.wgu, lw.n2, fg)]
            jobs = (key, ops.scale_cols_jobs(trip))
            if isinstance(out, _FoldList):
                out.jobs = jobs
        ops.scale_cols_batched(jobs[1], W.layers[0].wqkv.shape[1], W.layers[0].wqkv)
        return out
    for lw, (fq, fg) in zip(W.layers, out):
        fq.copy_(lw.wqkv.float() * lw.n1.float()[None, :])
        fg.copy_(lw.wgu.float() * lw.n2.float()[None, :])
    return out


class _FoldList(list):
    """fold_norm_weights' result: a list of (wqkv * n1, wgu * n2) that can carry the job table of its one-launch refresh"""
    jobs = None


LORA_PROJ = {"q_proj": ("qkv", 0), "k_proj": ("qkv", 1), "v_proj": ("qkv", 2), "o_proj": ("o", 0), "gate_proj": ("gu", 0),
             "up_proj": ("gu", 1), "down_proj": ("d", 0)}   # target module -> (projection of the fused layer, its part)


class LoraStack:
    """G slots of rank-R LoRA adapters for the decode step of ONE decoder stack, unmerged (stack_decode(lora=...)): a row's
    projection is x W^T + s (x A^T) B^T with A, B, s of the slot row_adapter[b] names, -1 for none (peft's LoraLayer.forward
    without dropout).  Per layer and fused projection (q|k|v 3 parts, o 1, gate|up 2, down 1) the slots' A matrices are stacked
    [part][slot][R] along the rows and their B matrices [slot][R] along the columns, in fixed buffers a captured graph reads;
    a slot that holds no adapter, the rows of a rank below R and the targets an adapter lacks are zeros.  The A stacks in front
    of q|k|v and gate|up are kept twice: as loaded, and with the layer's RMSNorm weight folded in (``refresh``), as
    fold_norm_weights does for W -- the shrink then runs on the unnormalised rows and the consumer's row scale covers it."""

    def __init__(self, spec: StackSpec, n_layers: int, G: int, R: int, B: int, like: torch.Tensor):
        if G < 1 or R < 8 or R % 8 or (G * R) % 256:
            raise ValueError(f"LoraStack: {G} slots of rank {R}: the rank must be a multiple of 8 and slots x rank one of 256")
        if like.dtype != torch.bfloat16 or not (1 <= B <= 256):
            raise ValueError(f"LoraStack: the unmerged decode form is bf16 with at most 256 rows ({B} rows of {like.dtype})")
        self.G, self.R, self.B = G, R, B
        D, I, GR = spec.D, spec.I, G * R
        z = lambda *shape: torch.zeros(shape, dtype=like.dtype, device=like.device)  # noqa: E731
        self.a = [dict(qkv=z(3 * GR, D), o=z(GR, D), gu=z(2 * GR, D), d=z(GR, I)) for _ in range(n_layers)]
        self.b = [dict(qkv=z(3 * D, GR), o=z(D, GR), gu=z(2 * I, GR), d=z(D, GR)) for _ in range(n_layers)]
        self.a_n = [(z(3 * GR, D), z(2 * GR, D)) for _ in range(n_layers)]
        self.slot_scale = torch.zeros(G, dtype=torch.float32, device=like.device)
        self.row_adapter = torch.full((B,), -1, dtype=torch.int32, device=like.device)
        self.dirty = True   # the norm-folded A stacks do not follow the raw ones yet: stack_decode refuses until ``refresh``

    def check_slot(self, g: int, layers) -> None:
        """the ValueErrors of ``load_slot``, and nothing else"""
        G, R = self.G, self.R
        if not 0 <= g < G or len(layers) != len(self.a):
            raise ValueError(f"LoraStack.load_slot: slot {g} of {G}, {len(layers)} layers of {len(self.a)}")
        for mods in layers:
            for name, (A, Bm) in mods.items():
                if name not in LORA_PROJ:
                    raise ValueError(f"LoraStack.load_slot: unknown target module {name!r}")
                if A.shape[0] > R or Bm.shape[1] != A.shape[0]:
                    raise ValueError(f"LoraStack.load_slot: rank {A.shape[0]} in slots of rank {R}")

    def load_slot(self, g: int, layers, scale: float) -> None:
        """slot g <- one adapter: ``layers`` [n_layers] of {target module: (A [r, in], B [out, r])}, r <= R; stream-ordered
        copies into the fixed buffers.  The stack is ``dirty`` until ``refresh`` has re-derived the folded A stacks."""
        self.check_slot(g, layers)
        G, R = self.G, self.R
        self.dirty = True
        for la, lb, mods in zip(self.a, self.b, layers):
            for name, (proj, part) in LORA_PROJ.items():
                rows = la[proj][(part * G + g) * R:(part * G + g + 1) * R]
                out = lb[proj].shape[0] // (3 if proj == "qkv" else 2 if proj == "gu" else 1)
                cols = lb[proj][part * out:(part + 1) * out, g * R:(g + 1) * R]
                rows.zero_()
                cols.zero_()
                if name in mods:
                    A, Bm = mods[name]
                    rows[:A.shape[0]].copy_(A)
                    cols[:, :A.shape[0]].copy_(Bm)
        self.slot_scale[g:g + 1].fill_(float(scale))

    def refresh(self, W: StackTensors) -> None:
        """re-derive the norm-folded A stacks from the raw ones and the live RMSNorm weights"""
        fake = StackTensors(layers=[LayerTensors(wqkv=la["qkv"], wgu=la["gu"], n1=lw.n1, n2=lw.n2) for la, lw in zip(self.a, W.layers)])
        fold_norm_weights(fake, self.a_n)
        self.dirty = False


def stack_decode(spec: StackSpec, W: StackTensors, x: torch.Tensor, rope: RopeTable, kv: KVState, pos_dev=None,
                 folded=None, final_norm: bool = True, x_ids=None, out: Optional[torch.Tensor] = None, shared=None,
                 row_pos=None, wide: Optional[bool] = None, lora: Optional[LoraStack] = None, row_cache=None):
    """x [B, D]: one new position per sequence at index kv.len (q_len == 1 => no causal mask,
    TF:integrations/sdpa_attention.py:120).

    With ``pos_dev`` (device int32[1]) the kernels take the position from device memory instead -- the form a captured
    hipGraph replays (decode.py); capacity and rope table must already cover it and kv.len is left to the caller.
    bf16 with at most 256 sequences runs the projections on the skinny kernels -- mh_gemm_skinny up to 64 rows,
    mh_gemm_skinny_wide from 65 to 256 (the same arithmetic on more row groups): 7 launches per layer (K/V append fused
    into the attention, gate|up and SwiGLU fused), 5 with ``folded`` (fold_norm_weights: the two RMSNorms ride on the
    q|k|v and gate|up projections); otherwise (fp32, more than 256 rows) the general GEMM is used (9 launches + split-K
    reductions).  ``wide=False`` sends 65 to 256 rows to the general form as well (None: MH_DECODE_WIDE, read here; a decode
    session reads it once and passes what it read).
    ``final_norm=False`` returns the residual stream before the stack's last RMSNorm (decode.py folds it into lm_head).
    ``x_ids`` (folded form only): ``x`` is an embedding table and row b of the input is x[x_ids[b]] -- the lookup happens
    inside the first layer's projections.
    ``shared`` = (kvp, pre_len_dev, workspace) (shared.SharedPrefix; event level, head_dim 64): the B rows continue ONE prompt
    whose K/V sit once in ``kvp`` (a KVState of one sequence, kvp.len rows) and ``kv`` holds only each row's suffix.  The
    position is kvp.len + kv.len (RoPE runs there), the new K/V row goes to suffix row kv.len, and in every form of the layer the
    attention step is the two launches of shared.py (attn_prefix_partial, attn_decode_append_shared: +1 launch per layer against
    the fused forms).  pre_len_dev goes with pos_dev: device int32[1] values a captured graph reads.
    ``row_pos`` (device int32 [B]; event level, head_dim 64; generate_ragged): row b stands at position row_pos[b] of its own
    cache -- RoPE there, K/V stored at that row, attention over rows [0, row_pos[b]] -- and the attention step of every form of the
    layer is the per-row entry point (same launch count).  The positions are always read on the device, eagerly too, so capacity,
    rope table and kv.len are the caller's business, as with pos_dev.  Not together with ``pos_dev``, nor with the one-prompt form
    of ``shared``.
    ``row_pos`` with ``shared`` = (kvs, slot_len, row_slot, workspace) (ops_share.SlotPrefix; DecodeSession(prefix_slots=G)): row b
    continues the prompt in slot row_slot[b] of ``kvs`` (a KVState of G sequences; slot_len[g] rows of slot g are valid), or none
    (-1), and ``kv`` holds what lies behind it: cache row j of row b is absolute position pre_b + j.  RoPE at row_pos[b]; the
    attention step of every form of the layer is the two launches of ops_share.py (attn_prefix_partial_slots,
    attn_decode_append_rows_shared: +1 launch per layer against the fused per-row form, for every row, sharing or not).
    ``kv`` a ``KVStateQ`` (DecodeSession(kv_dtype="fp8")): ``row_pos`` without ``shared`` in the fused layer forms only (bf16, at most
    256 rows) -- the attention step is mh_attn_decode_append_rows_fp8, same launch count; ``ValueError`` before any launch otherwise.
    ``lora`` (a LoraStack whose ``refresh`` followed the last load): an adapter per row, unmerged -- the fused folded form only
    (bf16, at most 256 rows, ``folded`` given), ``ValueError`` before any launch otherwise.  Each of the layer's four projections is
    preceded by its shrink (mh_lora_shrink_rows) and takes the expand as a second operand pair (mh_gemm_skinny_ext): 9 launches per
    layer.  The attention step, whichever form it has, is untouched.
    ``row_cache`` (device int32 [B], with ``row_pos``; DecodeSession(lookahead=k)): row b belongs to cache sequence row_cache[b] of
    ``kv`` -- a cache of kv.B <= B sequences that the rows of a group share -- or to none (-1: the row is inactive, stores nothing and
    attends to nothing).  The attention step of every form of the layer is the pair mh_kv_append_rows_via +
    mh_attn_decode_rows_via (ops_lookahead.py): the append completes first, so a row sees the keys the rows of its group stored
    below its position in the same layer; 6 launches per folded layer instead of 5.  Without ``row_pos``, with ``shared``, ``lora``
    or a ``KVStateQ``: ``ValueError`` before any launch."""
    _check_heads(spec)
    B, D = (x_ids.shape[0], x.shape[1]) if x_ids is not None else x.shape
    assert x_ids is None or folded is not None
    H, I, hd = spec.H, spec.I, spec.hd
    quant = isinstance(kv, KVStateQ)
    if row_cache is not None and (row_pos is None or shared is not None or lora is not None or quant or pos_dev is not None):
        raise ValueError("stack_decode(row_cache=...): the row map goes with per-row positions (row_pos) on the plain cache alone -- "
                         "not with pos_dev, a shared prompt, prefix slots, LoRA adapters or the fp8 cache")
    if quant and (row_pos is None or shared is not None):
        _refuse_kvq(kv, "stack_decode without row_pos" if row_pos is None else "stack_decode(shared=...)")
    from .ops_share import SlotPrefix
    slots = isinstance(shared, SlotPrefix)
    assert row_pos is None or ((shared is None or slots) and pos_dev is None and spec.kind == "event")
    assert not slots or row_pos is not None, "stack_decode: prefix slots go with per-row positions"
    pos = kv.len if pos_dev is None else 0
    attend = None  # what takes the place of the attention step, in all three forms of the layer
    if quant:  # (checked below: only the fused layer forms get here)
        def attend(qkv, o, li):
            ops.attn_decode_append_rows_fp8(qkv, rope.cos, rope.sin, kv.k8[li], kv.v8[li], kv.sc[li], o, B, H, hd, kv.cap, spec.scale,
                                            row_pos)
    elif row_cache is not None:
        def attend(qkv, o, li):
            ops.kv_append_rows_via(qkv, rope.cos, rope.sin, kv.k[li], kv.v[li], B, H, hd, kv.cap, row_pos, row_cache)
            ops.attn_decode_rows_via(qkv, kv.k[li], kv.v[li], o, B, H, hd, kv.cap, spec.scale, row_pos, row_cache)
    elif row_pos is not None:
        def attend(qkv, o, li):
            if fused:
                ops.attn_decode_append_rows(qkv, rope.cos, rope.sin, kv.k[li], kv.v[li], o, B, H, hd, kv.cap, spec.scale, row_pos)
            else:
                ops.kv_append_rows(qkv, rope.cos, rope.sin, kv.k[li], kv.v[li], B, H, hd, kv.cap, row_pos)
                ops.attn_decode_rows(qkv, kv.k[li], kv.v[li], o, B, H, hd, kv.cap, spec.scale, row_pos)
    if slots:
        kvs, slot_len, row_slot, ws = shared

        def attend(qkv, o, li):
            ops.attn_prefix_partial_slots(qkv, rope.cos, rope.sin, kvs.k[li], kvs.v[li], slot_len, row_slot, row_pos, ws, B, H, hd,
                                          kvs.B, kvs.cap, spec.scale)
            ops.attn_decode_append_rows_shared(qkv, rope.cos, rope.sin, kv.k[li], kv.v[li], ws, o, B, H, hd, kv.cap, kvs.B, kvs.cap,
                                               spec.scale, slot_len, row_slot, row_pos)
    elif shared is not None:
        from . import shared as sp
        kvp, pre_len_dev, ws = shared
        assert spec.kind == "event" and kvp.B == 1 and (pre_len_dev is None) == (pos_dev is None)
        pre, row = (kvp.len, kv.len) if pos_dev is None else (0, 0)
        pos = pre + row

        def attend(qkv, o, li):
            sp.attn_prefix_partial(qkv, rope.cos, rope.sin, kvp.k[li], kvp.v[li], ws, B, H, hd, kvp.cap, pre, pos, spec.scale,
                                   pre_len_dev, pos_dev)
            sp.attn_decode_append_shared(qkv, rope.cos, rope.sin, kv.k[li], kv.v[li], ws, o, B, H, hd, kv.cap, kvp.cap, pre, pos,
                                         spec.scale, pre_len_dev, pos_dev)
    if wide is None:
        wide = ops.decode_wide_enabled()
    # (rows=B: with x_ids, x is the embedding table and the step has as many rows as there are ids)
    use_wide = wide and ops.skinny_wide_ok(x, D, rows=B) and ops.skinny_wide_ok(x, I, rows=B)
    # x_ids come from a session with folds, which exists only where one of the two skinny entry points serves B rows
    assert x_ids is None or use_wide or B <= 64, "stack_decode: x_ids with a row count no skinny entry point serves"
    fused = (x_ids is not None) or use_wide or (ops.skinny_ok(x, D) and ops.skinny_ok(x, I))
    skinny = ops.gemm_skinny_wide if use_wide else ops.gemm_skinny  # one entry point per row-count class, same arguments
    if quant and not (fused and x.dtype == torch.bfloat16):
        raise ValueError(f"stack_decode: the fp8 K/V cache is served by the fused per-row attention only (bf16, at most 256 rows), "
                         f"not by the unfused kv_append_rows + attn_decode_rows pair: {B} rows of {x.dtype}")
    if lora is not None:
        if not (fused and folded is not None and x.dtype == torch.bfloat16 and ops.skinny_ext_ok(x, D, rows=B)
                and ops.skinny_ext_ok(x, I, rows=B)):
            raise ValueError(f"stack_decode: per-row LoRA adapters are served by the fused folded decode form only (bf16, at most 256 "
                             f"rows, folded weights): {B} rows of {x.dtype}, folded {'given' if folded is not None else 'missing'}"
                             + (" -- MH_DECODE_WIDE=0 (or wide=False) keeps 65 to 256 rows off that form" if B > 64 and not wide else ""))
        if lora.B != B or len(lora.a) != len(W.layers):
            raise ValueError(f"stack_decode: a LoraStack of {lora.B} rows and {len(lora.a)} layers for {B} rows and {len(W.layers)} layers")
        if lora.dirty:
            raise ValueError("stack_decode: the LoraStack was loaded into and not refreshed: its norm-folded A stacks are stale")
    if pos_dev is None and row_pos is None:  # (behind every refusal: nothing is allocated for a call that is refused)
        kv.reserve((pos if shared is None else kv.len) + 1)
        rope.ensure(pos + 1)
    for li, lw in enumerate(W.layers):
        if lora is not None:
            wqkv_n, wgu_n = folded[li]
            la, lb, (aq_n, agu_n) = lora.a[li], lora.b[li], lora.a_n[li]
            G_, R_, ra, sc = lora.G, lora.R, lora.row_adapter, lora.slot_scale
            ids = x_ids if li == 0 else None
            t3 = _empty((B, 3 * G_ * R_), x)
            ops.lora_shrink_rows(x, aq_n, t3, ra, sc, G_, R_, 3, row_ids=ids)
            qkv = _empty((B, 3 * D), x)
            ops.gemm_skinny_ext(x, wqkv_n, qkv, t3, lb["qkv"], 3, norm_eps=spec.eps, row_ids=ids)
            o = _empty((B, D), x)
            if attend is not None:
                attend(qkv, o, li)
            else:
                ops.attn_decode_append(qkv, rope.cos, rope.sin, kv.k[li], kv.v[li], o, B, H, hd, kv.cap, pos, spec.scale, pos_dev)
            t1 = _empty((B, G_ * R_), x)
            ops.lora_shrink_rows(o, la["o"], t1, ra, sc, G_, R_, 1)
            x2 = _empty((B, D), x)
            ops.gemm_skinny_ext(o, lw.wo, x2, t1, lb["o"], 1, res=x, res_ids=ids)
            t2 = _empty((B, 2 * G_ * R_), x)
            ops.lora_shrink_rows(x2, agu_n, t2, ra, sc, G_, R_, 2)
            a = _empty((B, I), x)
            ops.gemm_skinny_ext(x2, wgu_n, a, t2, lb["gu"], 2, mode=ops.SKINNY_GATEUP, norm_eps=spec.eps)
            t1 = _empty((B, G_ * R_), x)
            ops.lora_shrink_rows(a, la["d"], t1, ra, sc, G_, R_, 1)
            x3 = _empty((B, D), x)
            ops.gemm_skinny_ext(a, lw.wd, x3, t1, lb["d"], 1, res=x2)
            x = x3
            continue
        if fused and folded is not None:
            wqkv_n, wgu_n = folded[li]
            ids = x_ids if li == 0 else None  # layer 0 may read its input rows straight from the embedding table
            qkv = _empty((B, 3 * D), x)
            skinny(x, wqkv_n, qkv, norm_eps=spec.eps, row_ids=ids)
            o = _empty((B, D), x)
            if attend is not None:
                attend(qkv, o, li)
            else:
                ops.attn_decode_append(qkv, rope.cos, rope.sin, kv.k[li], kv.v[li], o, B, H, hd, kv.cap, pos, spec.scale, pos_dev)
            x2 = _empty((B, D), x)
            skinny(o, lw.wo, x2, res=x, res_ids=ids)
            a = _empty((B, I), x)
            skinny(x2, wgu_n, a, mode=ops.SKINNY_GATEUP, norm_eps=spec.eps)
            x3 = _empty((B, D), x)
            skinny(a, lw.wd, x3, res=x2)
            x = x3
            continue
        if fused:
            h1 = _empty((B, D), x)
            ops.rmsnorm_fwd(x, lw.n1, h1, None, spec.eps)
            qkv = _empty((B, 3 * D), x)
            skinny(h1, lw.wqkv, qkv)
            o = h1
            if attend is not None:
                attend(qkv, o, li)
            else:
                ops.attn_decode_append(qkv, rope.cos, rope.sin, kv.k[li], kv.v[li], o, B, H, hd, kv.cap, pos, spec.scale, pos_dev)
            x2 = _empty((B, D), x)
            skinny(o, lw.wo, x2, res=x)
            h2 = o
            ops.rmsnorm_fwd(x2, lw.n2, h2, None, spec.eps)
            a = _empty((B, I), x)
            skinny(h2, lw.wgu, a, mode=ops.SKINNY_GATEUP)  # gate|up never materialised
            x3 = _empty((B, D), x)
            skinny(a, lw.wd, x3, res=x2)
            x = x3
            continue
        h1 = _empty((B, D), x)
        ops.rmsnorm_fwd(x, lw.n1, h1, None, spec.eps)
        qkv = _empty((B, 3 * D), x)
        ops.gemm_nt(h1, lw.wqkv, qkv)
        o = h1
        if attend is not None:
            attend(qkv, o, li)
        else:
            ops.kv_append(qkv, rope.cos, rope.sin, kv.k[li], kv.v[li], B, H, hd, kv.cap, pos, pos_dev)
            ops.attn_decode(qkv, kv.k[li], kv.v[li], o, B, H, hd, kv.cap, pos + 1, spec.scale, pos_dev)
        x2 = _empty((B, D), x)
        ops.gemm_nt(o, lw.wo, x2, beta=1.0, res=x)
        h2 = o
        ops.rmsnorm_fwd(x2, lw.n2, h2, None, spec.eps)
        gu = _empty((B, 2 * I), x)
        ops.gemm_nt(h2, lw.wgu, gu)
        a = _empty((B, I), x)
        ops.swiglu_fwd(gu, a)
        x3 = _empty((B, D), x)
        ops.gemm_nt(a, lw.wd, x3, beta=1.0, res=x2)
        x = x3
    if pos_dev is None and row_pos is None:
        kv.len = (pos if shared is None else kv.len) + 1
    if not final_norm:
        return x
    y = out if out is not None else _empty((B, D), x)  # (`out`: the caller's buffer -- a decode session's `hidden` -- no copy)
    ops.rmsnorm_fwd(x, W.norm, y, None, spec.eps)
    return y
