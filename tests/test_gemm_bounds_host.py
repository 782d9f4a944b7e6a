"""CPU proof that the comparisons of tests/test_gemm_gpu.py bite: the GPU file's own checks, generators and case lists (its small
shapes), run against a backend that restates the entry points in torch.  The correct restatement (tests/emu_ops.py arithmetic,
with torch's fp32 product and with the 32-deep blocked fp32 order) is accepted bit for bit on the exact family and within the
bound on the Gaussian family; every named wrong kernel is rejected by at least one case of the GPU file's lists.  Also
re-measures the ratio that ref_gemm.py records for the Gaussian family's bound."""
import contextlib
import types

import pytest
import torch

import emu_ops as emu
import ref_gemm as G
import test_gemm_gpu as T
from ref_gemm import BF16, F32

SMALL = 3e7      # M N K of the cases the CPU runs


class Emu:
    """the C-ABI entry points test_gemm_gpu.Hip calls, restated in torch on the same poisoned buffers: reads what the header
    lets a kernel read and nothing else, writes the output view and nothing else.  `flaw` names one wrong kernel."""
    dev = "cpu"
    ops = types.SimpleNamespace(ab_library=contextlib.nullcontext)

    def __init__(self, flaw=None, blocked=False):
        self.flaw, self.blocked = flaw, blocked
        self.opt = dict(gemm=1, gemm_k64=1, gemm_lean_epi=1, skinny_mb=0, skinny_nbt=0)

    def set_option(self, name, value):
        self.opt[name] = value

    def get_option(self, name):
        return self.opt[name]

    # ---- reading operands: through the buffer behind the view, so that a flawed range reaches the poison
    @staticmethod
    def _base(v):
        return v._base if v._base is not None else v

    def _avail(self, v, trans):
        return self._base(v).shape[0 if trans else 1]

    def _cols(self, v, trans, rows, lo, hi):
        """logical [rows, hi - lo] in fp32"""
        b = self._base(v)
        return b[lo:hi, :rows].float().T if trans else b[:rows, lo:hi].float()

    def _product(self, a, ta, b, tb, M, N, lo, hi):
        hi = min(hi, self._avail(a, ta), self._avail(b, tb))
        if hi <= lo:
            return torch.zeros((M, N))
        x, y = self._cols(a, ta, M, lo, hi), self._cols(b, tb, N, lo, hi)
        if not self.blocked:
            return x @ y.T
        acc = torch.zeros((M, N))
        for k0 in range(0, hi - lo, 32):
            acc = acc + x[:, k0:k0 + 32] @ y[:, k0:k0 + 32].T
        return acc

    def _kstep(self, ta, tb, dtype):
        return T.kstep_of(ta, tb, self.opt["gemm_k64"], dtype, self.opt["gemm"])

    def _slices(self, K, splitk, step):
        sl = G.splitk_slices(K, splitk, step)
        f = self.flaw
        if f == "last 8-chunk of K dropped":
            sl = [(lo, min(hi, G.up(K, 8) - 8)) for lo, hi in sl]
        if f == "K read to the next multiple of the K-step":
            sl = [(lo, G.up(hi, step) if hi == K and hi > lo else hi) for lo, hi in sl]
        if f == "split-K slices overlap by one step":
            sl = [(lo - step if z and hi > lo else lo, hi) for z, (lo, hi) in enumerate(sl)]
        if f == "split-K slices leave a one-step gap":
            sl = [(min(lo + step, hi) if z else lo, hi) for z, (lo, hi) in enumerate(sl)]
        return sl

    # ---- epilogue and stores
    def _epi(self, acc, r, alpha, beta, dtype):
        x = alpha * acc
        if self.flaw == "product rounded to bf16 before the residual add" and dtype == BF16:
            x = x.to(BF16).float()
        if r is not None and beta != 0.0:
            x = alpha * (acc + beta * r.float()) if self.flaw == "alpha applied after the residual" else x + beta * r.float()
        return x

    def _store(self, c, x, tile=256):
        M, N = x.shape
        o, f = x.to(c.dtype), self.flaw
        keep = c.clone()
        c.copy_(o)
        if f == "last row of a ragged tile not stored" and M % tile:
            c[M - 1] = keep[M - 1]
        if f == "last column of a ragged tile not stored" and N % tile:
            c[:, N - 1] = keep[:, N - 1]
        if f == "store one 8-chunk past N" and self._base(c).shape[1] >= N + 8:
            self._base(c)[:M, N:N + 8] = 0
        if f == "one tile written twice, to its neighbour's place":
            if N > tile:
                w = min(tile, N - tile)
                c[:tile, tile:tile + w] = o[:tile, :w]
            elif M > tile:
                h = min(tile, M - tile)
                c[tile:tile + h, :tile] = o[:h, :tile]

    # ---- the entry points
    def gemm(self, a, ta, b, tb, c, r, M, N, K, alpha, beta, dtype, splitk, ws):
        sl = self._slices(K, splitk, self._kstep(ta, tb, dtype))
        parts = [self._product(a, ta, b, tb, M, N, lo, hi) for lo, hi in sl]
        if splitk == 1:
            return self._store(c, self._epi(parts[0], r, alpha, beta, dtype), 256 if self.opt["gemm"] and dtype == BF16 else 128)
        for z, p in enumerate(parts):
            ws[z] = p.to(BF16).float() if self.flaw == "split-K partials rounded to bf16" else p

    def splitk_reduce(self, ws, c, r, M, N, splitk, alpha, beta, dtype):
        s = ws[0].clone()
        for z in range(1, splitk):
            s = s + ws[z]
        self._store(c, self._epi(s, r, alpha, beta, dtype))

    def fold_blocks(self, M):
        return min(max(M, 1), 1024)

    def splitk_reduce_fold(self, ws, c, r, M, N, splitk, alpha, beta, wnorm, W, colpart):
        s = ws[0].clone()
        for z in range(1, splitk):
            s = s + ws[z]
        x = alpha * s
        nblk = self.fold_blocks(M)
        colpart[:nblk] = torch.zeros((nblk, N)).index_add_(0, torch.arange(M) % nblk, x * W.float())
        x = x * wnorm.float()[None, :]
        if r is not None and beta != 0.0:
            x = x + beta * r.float()
        self._store(c, x)

    def colsum(self, colpart, nblk, out, D, accumulate):
        s = colpart[:nblk].sum(0)
        out.copy_((s + out.float() if accumulate else s).to(out.dtype))

    def _scaled(self, acc, rowscale):
        return acc if rowscale is None else rowscale[:, None] * acc

    def gemm_swiglu(self, a, w, gu, act, M, I, K, rowscale=None):
        g = self._scaled(self._product(a, False, w, False, M, 2 * I, 0, K), rowscale).to(BF16)
        if gu is not None:
            self._store(gu, g.float())
        if self.flaw == "gate and up halves swapped":
            g = torch.cat([g[:, I:], g[:, :I]], 1)
        self._store(act, emu.swiglu_fwd(g, torch.empty((M, I), dtype=BF16)).float())

    def gemm_rope(self, a, w, c, table, npos, S, pos0, M, N, K, rowscale=None):
        x = self._scaled(self._product(a, False, w, False, M, N, 0, K), rowscale).to(BF16)
        pos = pos0 + torch.arange(M) % S
        if self.flaw == "RoPE position taken as m":
            pos = torch.arange(M).clamp_max(table.shape[0] - 1)
        emu.rope_(x, table[pos, :32].float(), table[pos, 64:96].float(), M, 0, N // 192, 64, +1)   # (row m of the gathered table)
        self._store(c, x.float())

    def gemm_dswiglu(self, a, b, gu, dgu, M, I, K, rowscale=None):
        da = self._scaled(self._product(a, False, b, True, M, I, 0, K), rowscale).to(BF16)
        self._store(dgu, emu.swiglu_bwd(gu, da, torch.empty((M, 2 * I), dtype=BF16)).float())

    def gemm_rowss(self, a, b, c, r, rowss, M, N, K):
        x = self._epi(self._product(a, False, b, False, M, N, 0, K), r, 1.0, 1.0, BF16)
        self._store(c, x)
        v = x if self.flaw == "rowss taken from the unrounded fp32 values" else x.to(BF16).float()
        rowss[: N // 64] = (v * v).view(M, N // 64, 64).sum(-1).T

    def row_rstd(self, x, parts, nparts, M, D, eps, rstd):
        emu.row_rstd(rstd, D, eps, x=x, parts=None if parts is None else parts[:nparts])

    def gemm_nt_scaled(self, a, b, c, rowscale, M, N, K):
        acc = self._product(a, False, b, False, M, N, 0, K)
        if self.flaw == "rowscale applied after the rounding":
            acc = acc.to(BF16).float()
        self._store(c, rowscale[:, None] * acc)

    def gemm_skinny(self, a, w, c, r, mode, eps, row_ids, res_ids, M, N, K):
        rows = (a[row_ids] if row_ids is not None else a[:M])[:, :K]
        x = rows.float() @ w[:, :K].float().T
        if eps > 0.0:
            x = x * torch.rsqrt(rows.float().pow(2).sum(-1, keepdim=True) / K + eps)
        if mode == 1:
            g = x.to(BF16)
            if self.flaw == "gate and up halves swapped":
                g = torch.cat([g[:, N:], g[:, :N]], 1)
            if self.flaw == "skinny SiLU replaced by max(g, 0)":
                return self._store(c, (g[:, :N].float().clamp_min(0).to(BF16).float() * g[:, N:].float()), 16)
            return self._store(c, emu.swiglu_fwd(g, torch.empty((M, N), dtype=BF16)).float(), 16)
        if r is not None and not (eps > 0.0 and self.flaw == "skinny residual dropped when norm_eps > 0"):
            x = x + (r[res_ids] if res_ids is not None and self.flaw != "skinny residual row taken from m" else r[:M]).float()
        self._store(c, x, 16)


def small(cases):
    return [c for c in cases if c[0] * c[1] * c[2] <= SMALL]


# --------------------------------------------------------------------------------------------------------- positive control
@pytest.mark.parametrize("blocked", [False, True], ids=["torch_fp32", "blocked_fp32"])
def test_the_correct_restatement_is_accepted(blocked):
    be = Emu(blocked=blocked)
    for M, N, K, layout in small(T.GEMM_EDGES):
        T.check_gemm(be, M, N, K, *layout, variants=T.ALL_VARIANTS[::2] if blocked else T.ALL_VARIANTS)
    for M, N, K, layout, splitk, alpha, beta, rmode in small(T.GEMM_SPLITK):
        T.check_gemm(be, M, N, K, *layout, splitk=splitk, alpha=alpha, beta=beta, rmode=rmode, variants=((0, 1), (1, 1)), seed=5)
    if blocked:
        return
    for case in list(gemm_cases(be)) + list(fused_cases(be)):    # (what the wrong kernels below are judged by)
        case()
    for M, N, K, splitk in small(T.GEMM128_F32):
        T.check_gemm(be, M, N, K, False, False, splitk=splitk, alpha=0.75, beta=0.5, rmode="inplace", dtype=F32, tile=(128, 128), seed=11)
    T.check_reduce(be, 33, 40, 4, 1.0, 1.0, "separate", ldc=42)
    T.check_reduce(be, 300, 12, 3, 0.75, 0.5, "inplace")
    T.check_reduce_fold(be, 1025, 40, 2, 0.5, 0.0, False)
    T.check_reduce_fold(be, 1023, 40, 3, 1.0, 1.0, True)
    for k64 in (0, 1):
        T.check_swiglu(be, 77, 128, 8, k64, True)
        T.check_rope(be, 257, 1, 64, 100, 5, k64)
        T.check_dswiglu(be, 77, 8, 8, k64)
    T.check_swiglu(be, 260, 128, 8, 1, False, scaled=True)
    T.check_rope(be, 260, 1, 8, 100, 5, 1, scaled=True)
    T.check_rope(be, 257, 2, 264, 1, 7)
    T.check_dswiglu(be, 257, 520, 72)
    T.check_dswiglu(be, 260, 64, 8, scaled=True)
    T.check_nt_scaled(be, 260, 250, 72)
    for exact_ss in (True, False):
        T.check_rowss(be, 257, 128, 64, True, exact_ss)
        T.check_rowss(be, 77, 64, 8, False, exact_ss)
    for mode in (0, 1):
        T.check_skinny(be, 15, 40, 512, mode, res=(mode == 0))
        T.check_skinny(be, 17, 40, 768, mode, eps=T.RMS_EPS, res=(mode == 0))
        T.check_skinny(be, 17, 40, 768, mode, gather=True, res=(mode == 0), odd_ldc=True)
        T.check_skinny(be, 17, 40, 768, mode, eps=T.RMS_EPS, gather=True)


def test_gaussian_family_accepts_both_fp32_orders():
    for blocked in (False, True):
        T.check_gauss(Emu(blocked=blocked))


def test_recorded_gemm_ratio_still_holds():
    ratio = G.measure_a_gemm()
    rec = G.A_TABLE["gemm"][0]
    assert ratio <= rec, f"the fp32 emulations are {ratio:.3e} sum|a b| from float64, recorded {rec:.1e}"
    assert ratio >= rec / 8, f"recorded ratio {rec:.1e} is far above the measured {ratio:.3e}"


# ------------------------------------------------------------------------------------------------------------ wrong kernels
def gemm_cases(be):
    """the GPU file's own lists, small shapes, as thunks"""
    for M, N, K, layout in small(T.GEMM_EDGES):
        yield lambda M=M, N=N, K=K, layout=layout: T.check_gemm(be, M, N, K, *layout, variants=((0, 1), (1, 1)))
    for M, N, K, layout, splitk, alpha, beta, rmode in small(T.GEMM_SPLITK):
        yield lambda M=M, N=N, K=K, layout=layout, s=splitk, al=alpha, b=beta, r=rmode: T.check_gemm(
            be, M, N, K, *layout, splitk=s, alpha=al, beta=b, rmode=r, variants=((0, 1), (1, 1)), seed=5)
    for alpha, beta, rmode in ((0.75, 0.0, None), (1.0, 1.0, "inplace"), (0.5, 0.5, "separate"), (2.0, 1.0, "separate")):
        yield lambda al=alpha, b=beta, r=rmode: T.check_gemm(be, 257, 250, 72, *T.NN, alpha=al, beta=b, rmode=r, seed=7)
    for M, N, K, splitk in small(T.TILE_ORDER):
        yield lambda M=M, N=N, K=K, s=splitk: T.check_gemm(be, M, N, K, *T.NN, splitk=s, seed=9)


def fused_cases(be):
    yield lambda: T.check_swiglu(be, 77, 128, 8)
    yield lambda: T.check_rope(be, 257, 1, 64, 100, 5)
    yield lambda: T.check_nt_scaled(be, 260, 250, 72)
    yield lambda: T.check_rowss(be, 257, 128, 64, True, True)
    yield lambda: T.check_rowss(be, 257, 128, 64, True, False)
    yield lambda: T.check_skinny(be, 15, 40, 512, 1)
    yield lambda: T.check_skinny(be, 17, 40, 768, 0, gather=True, res=True, odd_ldc=True)
    yield lambda: T.check_skinny(be, 17, 40, 768, 0, eps=T.RMS_EPS, res=True)
    yield lambda: T.check_skinny(be, 1, 16, 4096, 0, eps=T.RMS_EPS, res=True)
    yield lambda: T.check_skinny(be, 17, 40, 768, 1, eps=T.RMS_EPS)


WRONG = {
    "last 8-chunk of K dropped": gemm_cases,
    "K read to the next multiple of the K-step": gemm_cases,
    "split-K slices overlap by one step": gemm_cases,
    "split-K slices leave a one-step gap": gemm_cases,
    "split-K partials rounded to bf16": gemm_cases,
    "product rounded to bf16 before the residual add": gemm_cases,
    "alpha applied after the residual": gemm_cases,
    "last row of a ragged tile not stored": gemm_cases,
    "last column of a ragged tile not stored": gemm_cases,
    "store one 8-chunk past N": gemm_cases,
    "one tile written twice, to its neighbour's place": gemm_cases,
    "gate and up halves swapped": fused_cases,
    "RoPE position taken as m": fused_cases,
    "rowscale applied after the rounding": fused_cases,
    "rowss taken from the unrounded fp32 values": fused_cases,
    "skinny residual row taken from m": fused_cases,
    "skinny residual dropped when norm_eps > 0": fused_cases,
    "skinny SiLU replaced by max(g, 0)": fused_cases,
}


@pytest.mark.parametrize("flaw", list(WRONG))
def test_every_named_wrong_kernel_is_rejected(flaw):
    rejected = 0
    for case in WRONG[flaw](Emu(flaw)):
        try:
            case()
        except AssertionError:
            rejected += 1
            break
    assert rejected, f"no case of the GPU file's lists rejects: {flaw}"
