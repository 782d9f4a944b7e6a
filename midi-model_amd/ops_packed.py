"""Packed batches: wrappers over the table form of the event-level attention (mh_rope_pos, mh_attn_fwd_seqs, mh_attn_bwd_seqs in
include/midihip.h) and the host code that builds their launch tables.  Reached as ``ops.attn_seq_plan`` etc. (ops resolves these
names on first use).  bf16, the product's dtype: raw device pointers on the current stream, one launch per kernel, no torch math.
fp32 (verification only) has no table-form kernels: ``attn_fwd_seqs`` / ``attn_bwd_seqs`` then run the uniform fp32 kernels sequence
by sequence and copy each sequence's lse between the two layouts with torch -- HIP kernels still, never torch arithmetic."""
from __future__ import annotations

import numpy as np
import torch

from .ops import _p, _stream, dt, lib


class SeqPlan:
    """What the table form of the event-level attention needs for one packed batch (attn_seq_plan): ``host`` is ONE int32 tensor
    [seq_start (n + 1) | pos (M) | work (nwork x 4)], every section starting on a multiple of 4 elements; ``upload`` sends it to
    the device without blocking, after which ``seq_start`` / ``pos`` / ``work`` are views of the device copy."""

    def __init__(self, host: torch.Tensor, lengths, H: int, M: int, Mpad: int, nwork: int, off_pos: int, off_work: int):
        self.host, self.lengths, self.H, self.M, self.Mpad, self.nwork = host, tuple(lengths), H, M, Mpad, nwork
        self.n, self.max_len = len(self.lengths), max(self.lengths)
        self._off_pos, self._off_work = off_pos, off_work
        self.dev = None
        self._stage = None

    def _views(self, t: torch.Tensor):
        return (t[:self.n + 1], t[self._off_pos:self._off_pos + self.M],
                t[self._off_work:self._off_work + 4 * self.nwork].view(self.nwork, 4))

    def host_views(self):
        """(seq_start, pos, work) as views of the host tensor"""
        return self._views(self.host)

    def upload(self, device) -> "SeqPlan":
        device = torch.device(device)
        if device.type == "cuda":  # pinned staging, non-blocking (as WindowSampler._to_device): the step gains no sync
            self._stage = self.host.pin_memory()
            self.dev = self._stage.to(device, non_blocking=True)
        else:
            self.dev = self.host.to(device)
        self.seq_start, self.pos, self.work = self._views(self.dev)
        return self


def attn_seq_plan(lengths, H: int, passes: int = 5) -> SeqPlan:
    """The launch tables of mh_attn_fwd_seqs / mh_attn_bwd_seqs for sequences of ``lengths`` rows laid end to end.  Pure host code.

    work item = (sequence, head, tile rank, first row of the sequence in the 64-padded scratch); workgroup b of the launch takes
    item b, and the dispatcher places it on XCD b % 8.  What the uniform kernels' work order does (attn_mfma_common.h, r06) is kept:
      * all tiles of a (sequence, head) pair lie on ONE XCD, whose L2 then serves the pair's K/V (or Q/dO) panels; the pairs are
        dealt to the XCDs longest sequence first, round robin, so the XCDs' loads differ by at most one pair of each length;
      * on an XCD the heavy tiles come first, across all sequences: a tile's weight is the number of 128-row tiles it reaches
        back over (its sequence's tile count minus its rank), the weights 1 .. max are cut into ``passes`` contiguous classes
        (the uniform kernels' "attn_passes", default 5) and the classes run from heaviest to lightest; inside a class the tiles
        of one pair stay together, heaviest first.  ``passes`` >= the largest tile count orders strictly by weight.
    Lists of unequal length are padded with empty slots (sequence -1) to whole rounds of 8."""
    L = np.asarray(list(lengths), dtype=np.int64)
    if L.ndim != 1 or L.size == 0 or (L < 1).any():
        raise ValueError("attn_seq_plan: every sequence needs at least one row")
    if H < 1 or passes < 1:
        raise ValueError("attn_seq_plan: bad head or pass count")
    n = int(L.size)
    start = np.concatenate([[0], np.cumsum(L)])
    M = int(start[-1])
    pad64 = (L + 63) // 64 * 64
    soff = np.concatenate([[0], np.cumsum(pad64)])
    Mpad = int(soff[-1])
    # (a sequence is addressed with 32-bit offsets from its own first row: the bound is on the longest one, not on M)
    if int(L.max()) * 3 * H * 64 >= 2 ** 31 or Mpad >= 2 ** 31:
        raise ValueError("attn_seq_plan: a sequence too long for 32-bit panel offsets, or more than 2^31 rows")
    pos = np.arange(M, dtype=np.int64) - np.repeat(start[:-1], L)
    nt = (L + 127) // 128
    order = np.argsort(-L, kind="stable")              # longest sequence first
    rank_of_seq = np.empty(n, dtype=np.int64)
    rank_of_seq[order] = np.arange(n)
    # one row per (sequence, head, tile)
    seq = np.repeat(np.arange(n), nt * H)
    within = np.arange(seq.size) - np.repeat(np.concatenate([[0], np.cumsum(nt * H)])[:-1], nt * H)
    head = within // nt[seq]
    rank = within - head * nt[seq]
    pair = rank_of_seq[seq] * H + head                 # pairs in dealing order
    xcd = pair % 8
    maxnt = int(nt.max())
    P = min(int(passes), maxnt)
    lo = np.arange(P, dtype=np.int64) * maxnt // P     # first "rank from the heaviest weight" of every class
    cls = np.searchsorted(lo, maxnt - (nt[seq] - rank), side="right") - 1
    idx = np.lexsort((rank, pair, cls, xcd))           # by XCD, then class, pair, rank
    xs = xcd[idx]
    first = np.searchsorted(xs, np.arange(8), side="left")
    count = np.searchsorted(xs, np.arange(8), side="right") - first
    slots = int(count.max())
    work = np.full((slots * 8, 4), -1, dtype=np.int32)
    work[:, 1:] = 0
    dst = (np.arange(idx.size) - first[xs]) * 8 + xs
    work[dst, 0] = seq[idx]
    work[dst, 1] = head[idx]
    work[dst, 2] = rank[idx]
    work[dst, 3] = soff[seq[idx]]
    off_pos = (n + 1 + 3) // 4 * 4
    off_work = off_pos + (M + 3) // 4 * 4
    host = np.zeros(off_work + work.size, dtype=np.int32)
    host[:n + 1] = start
    host[off_pos:off_pos + M] = pos
    host[off_work:] = work.ravel()
    return SeqPlan(torch.from_numpy(host), [int(x) for x in L], H, M, Mpad, slots * 8, off_pos, off_work)


def rope_pos_(qkv: torch.Tensor, cos_t: torch.Tensor, sin_t: torch.Tensor, pos: torch.Tensor, H: int, hd: int, direction: int = 1):
    """rope_ with row m rotated at pos[m] (int32 [M] on the device)"""
    M = qkv.shape[0]
    assert qkv.is_contiguous() and qkv.shape[1] == 3 * H * hd
    assert pos.dtype == torch.int32 and pos.shape == (M,) and pos.is_contiguous()
    lib().call("mh_rope_pos", _p(qkv), _p(cos_t), _p(sin_t), _p(pos), M, H, hd, direction, dt(qkv), _stream())
    return qkv


def _seq_plan_check(plan: SeqPlan, qkv: torch.Tensor, H: int):
    assert plan.dev is not None, "SeqPlan.upload(device) first"
    assert plan.dev.device == qkv.device, f"the plan's tables are on {plan.dev.device}, the rows on {qkv.device}"
    assert plan.H == H and qkv.shape == (plan.M, 3 * H * 64) and qkv.is_contiguous()


def _uniform_lse(lse, plan: SeqPlan, H: int, a: int, b: int, fill: bool):
    """fp32 only: sequence [a, b)'s lse in the uniform entry points' layout [H, Sp] (a copy of its columns of [H, M] if ``fill``)"""
    S = b - a
    t = torch.zeros((H, (S + 63) // 64 * 64), dtype=torch.float32, device=lse.device)
    if fill:
        t[:, :S].copy_(lse.view(-1)[:H * plan.M].view(H, plan.M)[:, a:b])
    return t


def attn_fwd_seqs(qkv, o, lse, plan: SeqPlan, H: int, scale: float):
    """attn_fwd over the sequences of ``plan``: o [M, H*64], lse fp32 [H, M].  bf16 (the product): ONE launch.  fp32 (verification
    only): the table form has no fp32 kernels -- the uniform plain kernels run sequence by sequence, one launch each."""
    from . import ops
    _seq_plan_check(plan, qkv, H)
    assert lse.numel() >= H * plan.M and lse.dtype == torch.float32
    if qkv.dtype == torch.float32:
        a = 0
        for S in plan.lengths:
            t = _uniform_lse(lse, plan, H, a, a + S, False)
            ops.attn_fwd(qkv[a:a + S], o[a:a + S], t, 1, S, H, scale)
            lse.view(-1)[:H * plan.M].view(H, plan.M)[:, a:a + S].copy_(t[:, :S])
            a += S
        return o
    lib().call("mh_attn_fwd_seqs", _p(qkv), _p(plan.seq_start), _p(plan.work), plan.nwork, _p(o), _p(lse), plan.M, plan.max_len, H, scale,
               dt(qkv),
               _stream())
    return o


def attn_bwd_seqs(qkv, o, dout, lse, dqkv, plan: SeqPlan, H: int, scale: float, cos_t=None, sin_t=None, rowscale=None):
    """attn_bwd over the sequences of ``plan``: one launch per kernel (bf16); cos_t / sin_t rotate back at row - start of its
    sequence; ``rowscale`` fp32 [M] (bf16 only).  fp32: sequence by sequence, as attn_fwd_seqs."""
    from . import ops
    _seq_plan_check(plan, qkv, H)
    if qkv.dtype == torch.float32:
        assert rowscale is None, "rowscale: the bf16 kernels only"
        a = 0
        for S in plan.lengths:
            ops.attn_bwd(qkv[a:a + S], o[a:a + S], dout[a:a + S], _uniform_lse(lse, plan, H, a, a + S, True), dqkv[a:a + S], 1, S, H,
                         scale, cos_t, sin_t)
            a += S
        return dqkv
    if rowscale is not None:
        assert rowscale.shape == (plan.M,) and rowscale.dtype == torch.float32 and rowscale.is_contiguous()
    scratch = torch.empty((2 * H * plan.Mpad,), dtype=torch.float32, device=qkv.device)
    lib().call("mh_attn_bwd_seqs", _p(qkv), _p(o), _p(dout), _p(lse), _p(scratch), _p(dqkv), _p(rowscale), _p(plan.seq_start),
               _p(plan.work), plan.nwork, plan.M, plan.Mpad, plan.max_len, H, scale, _p(cos_t), _p(sin_t), dt(qkv), _stream())
    return dqkv


# -------------------------------------------------------------------------- ragged decode (MIDIModel.generate_ragged)
def _row_pos_check(row_pos, B: int, qkv: torch.Tensor):
    assert row_pos is not None and row_pos.dtype == torch.int32 and row_pos.shape == (B,) and row_pos.is_contiguous()
    assert row_pos.device == qkv.device


def kv_append_rows(qkv, cos_t, sin_t, kc, vc, B: int, H: int, hd: int, Lmax: int, row_pos):
    """kv_append with sequence b at position row_pos[b] (int32 [B] on the device)"""
    _row_pos_check(row_pos, B, qkv)
    lib().call("mh_kv_append_rows", _p(qkv), _p(cos_t), _p(sin_t), _p(kc), _p(vc), B, H, hd, Lmax, _p(row_pos), dt(qkv), _stream())


def attn_decode_rows(qkv, kc, vc, o, B: int, H: int, hd: int, Lmax: int, scale: float, row_pos):
    """attn_decode with sequence b attending to its cache rows [0, row_pos[b]]"""
    _row_pos_check(row_pos, B, qkv)
    lib().call("mh_attn_decode_rows", _p(qkv), _p(kc), _p(vc), _p(o), B, H, hd, Lmax, scale, _p(row_pos), dt(qkv), _stream())
    return o


def attn_decode_append_rows(qkv, cos_t, sin_t, kc, vc, o, B: int, H: int, hd: int, Lmax: int, scale: float, row_pos):
    """kv_append_rows + attn_decode_rows in one launch (qkv is read unrotated and left untouched)"""
    _row_pos_check(row_pos, B, qkv)
    lib().call("mh_attn_decode_append_rows", _p(qkv), _p(cos_t), _p(sin_t), _p(kc), _p(vc), _p(o), B, H, hd, Lmax, scale,
               _p(row_pos), dt(qkv), _stream())
    return o


def kv_store_seqs(qkv, plan: SeqPlan, kc, vc, H: int, hd: int, Lmax: int):
    """the rotated K, V of a packed prefill -> cache rows [0, L_s) of every sequence s of ``plan``; kc / vc [n, H, Lmax, hd]"""
    assert plan.dev is not None, "SeqPlan.upload(device) first"
    assert qkv.shape == (plan.M, 3 * H * hd) and qkv.is_contiguous() and kc.shape[0] == plan.n
    if plan.max_len > Lmax:
        raise ValueError(f"kv_store_seqs: a sequence of {plan.max_len} rows in a cache of {Lmax}")
    lib().call("mh_kv_store_seqs", _p(qkv), _p(plan.seq_start), _p(kc), _p(vc), plan.n, plan.M, H, hd, Lmax, dt(qkv), _stream())
