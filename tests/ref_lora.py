"""TEST-ONLY: references, checks and a torch restatement for the two kernels behind a LoRA adapter per decode row
(mh_gemm_skinny_ext, mh_lora_shrink_rows; gemm_skinny.hip).  tests/test_lora_kernels_gpu.py runs the checks against the HIP entry
points, tests/test_lora_bounds_host.py runs the same checks on the CPU against `Emu` below and against named wrong kernels.

THE EXACT FAMILY is that of ref_gemm.py with ONE cap for both operand pairs, cap_of(K + K2): the accumulator of an output element
holds sum_k a_k w_k + sum_j t_j b_j, at most (K + K2) cap^2 <= 2^23 in units of the common q^2 -- both pairs share the unit
(qt qb = qa qw), so every partial sum in any order is an fp32 value and every correct kernel returns the same bits.  A case may
make T 64 times larger than A (qt = 64 qa, qb = qw / 64): the products keep their unit, and a row scale whose sum of squares
took T in is wrong by a factor no rounding hides.

The shrink's slot scales are powers of two, so scale x exact product is an fp32 value and its bf16 rounding the only one."""
from __future__ import annotations

import torch

import ref_gemm as G
import test_gemm_gpu as T
from ref_gemm import BF16, F32, F64
from ref_streamers import RMS_EPS  # noqa: F401

# (M, N, K, K2, parts, mode): the issue's list -- narrow tilings, then the wide ones
EXT_SHAPES = [
    (1, 16, 256, 256, 1, 0), (17, 48, 512, 256, 3, 0), (64, 2112, 256, 512, 3, 0), (33, 4128, 256, 256, 1, 0),
    (64, 40, 256, 256, 2, 1), (16, 16, 1024, 512, 2, 1),
    (65, 48, 256, 256, 3, 0), (129, 2112, 512, 256, 3, 0), (200, 40, 256, 512, 2, 1),
]
SHRINK_M = [1, 17, 64, 65, 129]
SHRINK_GR = [(4, 64), (8, 32)]
SHRINK_PARTS = [1, 2, 3]
SHRINK_K = [256, 1024]


def part_products(Tm, Bs, parts, K2):
    """Tm [M, parts K2], Bs [rows, K2] float64 -> [M, rows]: weight row w against the slice of its part"""
    rows = Bs.shape[0]
    rpp = rows // parts
    out = torch.empty((Tm.shape[0], rows), dtype=F64)
    for p in range(parts):
        out[:, p * rpp:(p + 1) * rpp] = Tm[:, p * K2:(p + 1) * K2] @ Bs[p * rpp:(p + 1) * rpp].T
    return out


def ext_operands(Trows, M, rows, K, K2, parts, seed):
    cap = G.cap_of(K + K2)
    A, W = G.exact_operands(Trows, rows, K, seed, cap=cap)
    Tm, Bs = G.ints((M, parts * K2), cap, seed + 7), G.ints((rows, K2), cap, seed + 8)
    return A, W, Tm, Bs


def check_ext(be, M, N, K, K2, parts, mode, eps=0.0, gather=False, res=False, odd_ldc=False, t_big=False, seed=171):
    """check_skinny of test_gemm_gpu.py with the second operand pair: bit-exact against the per-part integer sums, with `eps` the
    rounded-interval check (rstd from A alone)"""
    rows = 2 * N if mode == 1 else N
    Tn = M + 3 if gather else M
    A, W, Tm, Bs = ext_operands(Tn, M, rows, K, K2, parts, seed)
    ids = rids = None
    if gather:
        ids = (torch.arange(M) * 7 + 1) % Tn
        ids[0] = Tn - 1
        ids[M // 2] = ids[0]
        rids = (torch.arange(M) * 5 + 2) % Tn
        rids[M - 1] = Tn - 1
    A_rows = A[ids] if gather else A
    P1, P2 = A_rows @ W.T, part_products(Tm, Bs, parts, K2)
    P = P1 + P2
    assert float((A_rows.abs() @ W.abs().T + part_products(Tm.abs(), Bs.abs(), parts, K2)).max()) < 2 ** 24, "exactness margin"
    assert G.wide_share(P) >= 0.5 and float((P2 != 0).double().mean()) > 0.9
    qa = G.scale_to(A, 2.0)
    xa = qa * A_rows
    rstd = torch.rsqrt((xa * xa).sum(-1) / K + eps) if eps > 0.0 else torch.ones(M, dtype=F64)
    limit = 8.0 if mode == 1 else 4.0
    qw = G.scale_to(rstd[:, None] * qa * P[:, :N], limit)
    q2 = qa * qw
    qt, qb = (64 * qa, qw / 64) if t_big else (qa, qw)
    x = q2 * P
    R = G.residual(Tn, N, seed + 2, 2.0 ** -5) if res else None
    Rm = None if R is None else (R[rids] if gather else R)
    dev = be.dev
    a, w = T.to_dev(G.operand(A, qa, BF16, False), dev), T.to_dev(G.operand(W, qw, BF16, False, pad=16), dev)
    t, bst = T.to_dev(G.operand(Tm, qt, BF16, False, pad=24), dev), T.to_dev(G.operand(Bs, qb, BF16, False), dev)
    r = T.to_dev(T.nan_input(R.to(BF16), pad=24), dev) if res else None
    cbuf, c = T.new_out(M, N, BF16, dev, ldc=(N + 5) | 1 if odd_ldc else None)
    what = f"gemm_skinny_ext {M}x{N}x{K}+{K2} parts={parts} mode={mode} eps={eps} gather={gather} res={res} odd_ldc={odd_ldc} t_big={t_big}"
    be.gemm_skinny_ext(a, w, c, r, t, bst, mode, eps, None if ids is None else ids.to(dev),
                       None if rids is None or not res else rids.to(dev), M, N, K, K2, parts)
    assert G.fence_ok(cbuf, M, N), f"{what}: written outside the view"
    assert limit / 2 < float((rstd[:, None] * x[:, :N]).abs().max()) <= limit
    if eps > 0.0:
        d = (G.rstd_bound(rstd, K, BF16) / rstd)[:, None]
        e1, e2 = (x * rstd[:, None] * (1 - d)).to(F32).to(F64), (x * rstd[:, None] * (1 + d)).to(F32).to(F64)
        lo, hi = torch.minimum(e1, e2), torch.maximum(e1, e2)
    if mode == 0:
        if eps > 0.0:
            add = 0.0 if Rm is None else Rm
            msg = G.within_rounded_interval(c, lo + add, hi + add, BF16)
            assert float((G.rd(lo + add, BF16) == G.rd(hi + add, BF16)).double().mean()) > 0.9
        else:
            msg = G.mismatch(c, G.exact_out(P, q2, BF16, 1.0, 1.0 if res else 0.0, Rm), tile=(16, 32))
        assert msg is None, f"{what}: {msg}"
        return
    if eps == 0.0:
        gus = [G.exact_out(P, q2, BF16).to(BF16)]
    else:
        g_lo, g_hi = G.rd(lo, BF16).to(BF16), G.rd(hi, BF16).to(BF16)
        assert float((g_lo == g_hi).double().mean()) > 0.9
        gus = [torch.cat([g[:, :N], u[:, N:]], 1) for g in (g_lo, g_hi) for u in (g_lo, g_hi)]
    got = c.detach().cpu().to(F64)
    low = high = None
    for gu_t in gus:
        ref, terms = G.swiglu_fwd_ref(gu_t, BF16)
        bnd = G.swiglu_fwd_bound(terms, gu_t, BF16)
        low = ref - bnd if low is None else torch.minimum(low, ref - bnd)
        high = ref + bnd if high is None else torch.maximum(high, ref + bnd)
    wrong = ~((got >= low) & (got <= high))
    assert not wrong.any(), f"{what}: activation: {int(wrong.sum())}/{wrong.numel()} outside the bound, first {wrong.nonzero()[0].tolist()}"


def check_ext_variants(be, M, N, K, K2, parts, mode):
    """the issue's variants for one shape"""
    check_ext(be, M, N, K, K2, parts, mode, res=(mode == 0 and (M + N) % 2 == 0))
    check_ext(be, M, N, K, K2, parts, mode, eps=RMS_EPS, res=(mode == 0))
    check_ext(be, M, N, K, K2, parts, mode, gather=True, res=(mode == 0))
    check_ext(be, M, N, K, K2, parts, mode, gather=(mode == 1), odd_ldc=True)
    check_ext(be, M, N, K, K2, parts, mode, eps=RMS_EPS, t_big=True)


def adapter_maps(M, Gs):
    """all -1; all one slot; slot G-1; every row a different slot (as far as there are slots), unsorted, some rows none"""
    mixed = (torch.arange(M) * 5 + 3) % (Gs + 1) - 1        # -1 .. G-1 in an order that is not sorted
    return {"none": torch.full((M,), -1), "one": torch.full((M,), min(1, Gs - 1)), "last": torch.full((M,), Gs - 1), "mixed": mixed}


def slot_scales(Gs):
    return torch.tensor([2.0 ** ((g * 3) % 5 - 2) for g in range(Gs)], dtype=F64)     # 1/4 .. 4, neighbours differ


def check_shrink(be, M, Gs, R, parts, K, amap, gather=False, seed=271):
    N = parts * Gs * R
    Tn = M + 3 if gather else M
    A, W = G.exact_operands(Tn, N, K, seed)
    ids = None
    if gather:
        ids = (torch.arange(M) * 7 + 1) % Tn
        ids[0] = Tn - 1
    P = (A[ids] if gather else A) @ W.T
    assert G.wide_share(P) >= 0.5
    qa = G.scale_to(A, 2.0)
    qw = G.scale_to(qa * P, 4.0)
    sc = slot_scales(Gs)
    slot = (torch.arange(N) // R) % Gs
    x = sc[slot][None, :] * (qa * qw) * P
    assert G.is_f32(x)
    member = amap[:, None] == slot[None, :]
    ref = torch.where(member, G.rd(x, BF16), torch.zeros((), dtype=F64))
    dev = be.dev
    a, w = T.to_dev(G.operand(A, qa, BF16, False), dev), T.to_dev(G.operand(W, qw, BF16, False, pad=16), dev)
    tbuf, t = T.new_out(M, N, BF16, dev)
    be.lora_shrink(a, w, t, amap.to(torch.int32).to(dev), sc.to(F32).to(dev), None if ids is None else ids.to(dev), M, K, Gs, R, parts)
    what = f"lora_shrink_rows M={M} G={Gs} R={R} parts={parts} K={K} gather={gather}"
    assert G.fence_ok(tbuf, M, N), f"{what}: written outside the view"
    msg = G.mismatch(t, ref, tile=(16, 32))      # (NaN never equal: the poison must be gone everywhere, +0 where no member)
    assert msg is None, f"{what}: {msg}"


def check_shrink_all(be, M, Gs, R):
    for parts in SHRINK_PARTS:
        for K in SHRINK_K:
            for i, (name, amap) in enumerate(adapter_maps(M, Gs).items()):
                check_shrink(be, M, Gs, R, parts, K, amap, gather=(name == "mixed" and K == 256))


REFUSALS = [  # (what, kwargs of check_refusal, a word of the message)
    ("K2 = 128", dict(K2=128), "K2"),
    ("part boundary inside a column block", dict(N=48, parts=2), "part boundary"),
    ("fp32", dict(dtype=F32), "bf16"),
]


def check_refusal(be, N=48, K2=256, parts=3, dtype=BF16):
    """the call fails with a message, the output keeps its poison"""
    M, K = 17, 256
    A, W, Tm, Bs = ext_operands(M, M, N, K, K2, parts, 371)
    dev = be.dev
    a, w = T.to_dev(G.operand(A, 0.25, dtype, False), dev), T.to_dev(G.operand(W, 0.25, dtype, False, pad=16), dev)
    t, bst = T.to_dev(G.operand(Tm, 0.25, dtype, False, pad=24), dev), T.to_dev(G.operand(Bs, 0.25, dtype, False), dev)
    cbuf, c = T.new_out(M, N, dtype, dev)
    try:
        be.gemm_skinny_ext(a, w, c, None, t, bst, 0, 0.0, None, None, M, N, K, K2, parts, dtype=dtype)
    except RuntimeError as e:
        assert G.fence_ok(cbuf, M, N) and bool(torch.isnan(c).all()), "a refused call wrote to its output"
        return str(e)
    raise AssertionError("the call was not refused")


# ----------------------------------------------------------------------------------------------------------- torch restatement
class Emu:
    """the two entry points restated in torch on the same poisoned buffers (reads the views the header lets a kernel read, writes
    the output view); `flaw` names one wrong kernel"""
    dev = "cpu"
    FLAWS_EXT = ("rstd over [A | T]", "every part reads part 0", "the up half reads the gate's T")
    FLAWS_SHRINK = ("the slot mask left out", "the scale of the neighbouring slot", "zeros not written")

    def __init__(self, flaw=None):
        self.flaw = flaw

    def gemm_skinny_ext(self, a, w, c, r, t, bst, mode, eps, row_ids, res_ids, M, N, K, K2, parts, dtype=BF16):
        import emu_ops as emu
        rows = 2 * N if mode == 1 else N
        if dtype != BF16:
            raise RuntimeError("mh_gemm_skinny_ext failed (-1): gemm_skinny_ext: bf16 only")
        if K2 % 256:
            raise RuntimeError(f"mh_gemm_skinny_ext failed (-1): gemm_skinny_ext: K2={K2} must be a multiple of 256")
        rpp = rows // parts
        nb = 16 if (mode == 1 or N < 2048) else 32
        if not (parts == 1 or (mode == 1 and (parts == 2 or (rpp % 16 == 0 and N % rpp == 0))) or (mode == 0 and rpp % nb == 0)):
            raise RuntimeError(f"mh_gemm_skinny_ext failed (-1): gemm_skinny_ext: a part boundary (every {rpp} weight rows) falls inside")
        xr = (a[row_ids] if row_ids is not None else a[:M])[:, :K].float()
        acc = xr @ w[:rows, :K].float().T
        for wr in range(0, rows, rpp):
            p = wr // rpp
            if self.flaw == "every part reads part 0" or (self.flaw == "the up half reads the gate's T" and mode == 1 and wr >= N):
                p = 0
            acc[:, wr:wr + rpp] += t[:M, p * K2:(p + 1) * K2].float() @ bst[wr:wr + rpp, :K2].float().T
        if eps > 0.0:
            ss, n = xr.pow(2).sum(-1, keepdim=True), K
            if self.flaw == "rstd over [A | T]":
                ss, n = ss + t[:M, :K2].float().pow(2).sum(-1, keepdim=True), K + K2
            acc = acc * torch.rsqrt(ss / n + eps)
        if mode == 1:
            c.copy_(emu.swiglu_fwd(acc.to(BF16), torch.empty((M, N), dtype=BF16)))
            return
        if r is not None:
            acc = acc + (r[res_ids] if res_ids is not None else r[:M])[:, :N].float()
        c.copy_(acc.to(BF16))

    def lora_shrink(self, a, astack, t, row_adapter, slot_scale, row_ids, M, K, Gs, R, parts, dtype=BF16):
        N = parts * Gs * R
        xr = (a[row_ids] if row_ids is not None else a[:M])[:, :K].float()
        acc = xr @ astack[:N, :K].float().T
        slot = (torch.arange(N) // R) % Gs
        sc = slot_scale[(slot + 1) % Gs] if self.flaw == "the scale of the neighbouring slot" else slot_scale[slot]
        val = (sc[None, :] * acc).to(BF16)
        member = row_adapter.long()[:, None] == slot[None, :]
        if self.flaw == "the slot mask left out":
            member = torch.ones_like(member)
        if self.flaw == "zeros not written":
            t[member] = val[member]
            return
        t.copy_(torch.where(member, val, torch.zeros((), dtype=BF16)))
