"""TEST-ONLY: references, operand generators and bounds of the GEMM-family tests (tests/test_gemm_gpu.py runs them against the
HIP kernels, tests/test_gemm_bounds_host.py proves on the CPU that the same comparisons reject named wrong kernels and accept a
correct restatement).  Everything works on CPU tensors; the callers move the buffers to the device.

THE EXACT FAMILY.  All operands are integers times one power of two q, dense in [-cap, cap] with cap = floor(sqrt(2^23 / K)), at
most 255 (eight significant bits: every value is a bf16).  Then for every output element sum_k |a_k| |b_k| <= K cap^2 <= 2^23:
every partial sum, in any order and any slicing, is an integer below 2^24 (in units of q^2) and so exactly representable in
fp32.  The fp32 accumulator of a correct kernel holds the exact product whatever its K loop, tile order or split-K slicing, and
the stored bf16 value is its round-to-nearest-even image: every correct kernel returns the SAME BITS.  `exact_operands` asserts
both conditions the argument needs: (1) |A| |B|^T < 2^24, and (2) at least half of the values that get rounded to bf16 -- the
outputs, and with split-K every slice's partials -- need more than 8 significant bits, so that an intermediate bf16 rounding
cannot hide.  alpha, beta and R are powers of two, 0.75 and small integers: `exact_out` asserts that alpha P, beta R and their sum
are fp32 values, so fused or unfused multiply-adds give the same bits.

POISON.  A row-major operand [rows, K] lives in a buffer with ld > K: zeros from K to the next multiple of 8 (the header's
contract; fp32: of 4), NaN from there to ld and in one more row behind the last.  A contraction-major operand [K, rows] has NaN in two more
rows behind K and in the columns from `rows` to ld.  An output view [M, N] is NaN inside and holds FENCE in its padding columns
and in one row behind the last: a value never written is NaN, a value written out of place breaks the fence.

THE FULL-MANTISSA FAMILY.  Integers below the cap use 6-8 operand bits; Gaussian bf16 operands use all of them.  Bound:

    |got - C64| <= E_T |C64| + a sum_k |a_k b_k| + TINY,      a = 4 x recorded ratio  (the A_TABLE convention of ref_streamers)

The ratio is the largest |emulation - C64| / sum_k |a_k b_k| over two fp32 emulations of the product on GAUSS_SHAPES: torch's
fp32 matmul and `blocked_fp32` (32-deep blocks added to an fp32 accumulator in K order, the kernels' order).  `measure_a_gemm`
measures it (the host test re-runs it: above the recorded value, or below 1/8 of it, fails); it is never taken from a kernel.

    op     measured ratio    A
    gemm   7.1e-08           3.0e-07   (recorded as 7.5e-08)
"""
from __future__ import annotations

import math

import numpy as np
import torch

from ref_streamers import (BF16, E, F32, F64, TINY, U24, bad, f64, rd, reduction_bound, rope_bound, rope_ref, rope_tables,  # noqa: F401
                           rstd_bound, swiglu_bwd_bound, swiglu_bwd_ref, swiglu_fwd_bound, swiglu_fwd_ref, worst)

A_TABLE = {"gemm": (7.5e-08, 0)}   # op -> (recorded largest ratio of the fp32 emulations, hardware approximations)
GAUSS_SHAPES = [(37, 24, 72), (20, 40, 264), (9, 16, 1096)]
FENCE = -19.5                      # a bf16 value no test produces in bulk
NAN = float("nan")


def a_gemm():
    ratio, hw = A_TABLE["gemm"]
    return 4 * ratio + hw * 2.0 ** -23


def up(x, m):
    return -(-x // m) * m


# ------------------------------------------------------------------------------------------------------------ exact family
def cap_of(K):
    return max(1, min(255, math.isqrt(2 ** 23 // K)))


def ints(shape, cap, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-cap, cap + 1, shape, generator=g).to(F64)


def is_f32(x64):
    return bool((x64.to(F32).to(F64) == x64).all())


def wide_share(x64):
    """share of the values that need more than 8 significant bits (a bf16 rounding changes them)"""
    return float((x64.to(F32).to(BF16).to(F64) != x64).double().mean())


def splitk_slices(K, splitk, kstep):
    """the launchers' slicing: whole K-steps per slice, the last one short, slices past K empty"""
    kps = up(-(-K // splitk), kstep)
    return [(min(z * kps, K), min((z + 1) * kps, K)) for z in range(splitk)]


def slice_products(A, B, slices):
    """A [M, K], B [N, K] float64 -> the exact partial product of every slice"""
    return [A[:, lo:hi] @ B[:, lo:hi].T if hi > lo else torch.zeros((A.shape[0], B.shape[0]), dtype=F64) for lo, hi in slices]


def exact_operands(M, N, K, seed, cap=None):
    """-> (A [M, K], B [N, K]): integer-valued float64 matrices of the exact family; asserts condition (1)"""
    cap = cap or cap_of(K)
    A, B = ints((M, K), cap, seed), ints((N, K), cap, seed + 1)
    assert float((A.abs() @ B.abs().T).max()) < 2 ** 24, "exactness margin"
    return A, B


def exact_partials(A, B, slices, wide=True):
    """the exact partial product of every slice (their sum is the product); asserts condition (2) on every non-empty slice and
    on the sum"""
    parts = slice_products(A, B, slices)
    if wide:
        for (lo, hi), p in zip(slices, parts):
            assert hi == lo or wide_share(p) >= 0.5, f"slice {lo}..{hi}: only {wide_share(p):.2f} of the partials need more than 8 bits"
        assert wide_share(sum(parts)) >= 0.5, f"only {wide_share(sum(parts)):.2f} of the outputs need more than 8 bits"
    return parts


def exact_out(P, q2, dtype, alpha=1.0, beta=0.0, R=None, wide=True):
    """rd(alpha q2 P + beta R): P the exact integer product, R float64 (already in real units).  Every step is an fp32 value."""
    x = alpha * q2 * P
    assert is_f32(x)
    if beta != 0.0:
        assert is_f32(beta * R) and is_f32(x + beta * R)
        x = x + beta * R
    assert not wide or dtype != BF16 or wide_share(x) >= 0.5
    return rd(x, dtype)


def residual(M, N, seed, unit, cap=127):
    """small integers times `unit` (a power of two not below the product's unit): alpha P + beta R stays an fp32 value"""
    return ints((M, N), cap, seed) * unit


def scale_to(P, limit):
    """the power of two q2 with max |q2 P| in (limit / 2, limit]"""
    return 2.0 ** math.floor(math.log2(limit / float(P.abs().max())))


# --------------------------------------------------------------------------------------------------------------- buffers
def operand(X, q, dtype, trans, pad=8):
    """X [rows, K] float64 (logical: rows x contraction) -> the poisoned buffer's view: [rows, K] row-major, or with `trans`
    [K, rows] contraction-major"""
    rows, K = X.shape
    gran = 8 if dtype == BF16 else 4     # elements of a 16-byte chunk
    if trans:
        buf = torch.full((K + 2, up(rows, 8) + pad), NAN, dtype=dtype)
        buf[:K, :rows] = (X.T * q).to(dtype)
        return buf[:K, :rows]
    K8 = up(K, gran)
    buf = torch.full((rows + 1, K8 + pad), NAN, dtype=dtype)
    buf[:rows, :K] = (X * q).to(dtype)
    buf[:rows, K:K8] = 0
    return buf[:rows, :K]


def out_view(M, N, dtype, ldc=None, init=None):
    """-> (buf [M + 1, ldc], view [M, N]): NaN (or `init`) inside, FENCE around"""
    buf = torch.full((M + 1, ldc or up(N, 8) + 8), FENCE, dtype=dtype)
    buf[:M, :N] = NAN if init is None else init.to(dtype)
    return buf, buf[:M, :N]


def fence_ok(buf, M, N):
    b = buf.cpu()
    return bool((b[:M, N:] == FENCE).all() and (b[M:] == FENCE).all())


# ----------------------------------------------------------------------------------------------------------- comparison
def explain(got, a_row, b_row, q2, add, dtype, step):
    """which K-step's contribution, dropped or doubled BEFORE the output rounding, gives `got`: rd(q2 (P -+ c) + add) == got"""
    K, P = a_row.numel(), float((a_row * b_row).sum())
    for width in (step, 8):      # a whole K-step, then a single 8-chunk
        for k0 in range(0, K, width):
            c = float((a_row[k0:k0 + width] * b_row[k0:k0 + width]).sum())
            for sign, word in ((-1.0, "dropped"), (1.0, "added twice")):
                if c != 0 and float(rd(torch.tensor(q2 * (P + sign * c) + add, dtype=F64), dtype)) == got:
                    return f"the value with the contribution of k {k0}..{min(k0 + width, K)} {word}"
    return "no single K-step or 8-chunk dropped or added twice gives it"


def mismatch(got, ref64, A=None, B=None, q2=1.0, tile=(256, 256), step=32, add=None):
    """None when `got` holds exactly ref64's values, the sign of a zero included (`torch.equal` on the stored bits, NaN never
    equal); else a message naming the first wrong index, its tile and, given the operands of ref = rd(q2 A B^T + add), the K
    range whose contribution explains the value"""
    g = got.detach().cpu().to(F64)
    wrong = ~(g == ref64) | (torch.signbit(g) != torch.signbit(ref64))      # (NaN compares unequal)
    if not wrong.any():
        return None
    m, n = (int(i) for i in wrong.nonzero()[0])
    msg = (f"{int(wrong.sum())}/{wrong.numel()} elements differ; first [{m}, {n}] (tile {m // tile[0]}, {n // tile[1]}; row {m % tile[0]}, "
           f"col {n % tile[1]} of it): got {float(g[m, n])!r}, want {float(ref64[m, n])!r}")
    if A is not None and math.isfinite(float(g[m, n])):
        msg += "; " + explain(float(g[m, n]), A[m], B[n], q2, 0.0 if add is None else float(add[m, n]), got.dtype, step)
    return msg


def out_of_bound(got, ref64, bnd):
    """None when every element is finite and inside the bound; else a message"""
    n = bad(got.detach().cpu(), ref64, bnd)
    if n == 0:
        return None
    g = got.detach().cpu().to(F64)
    w = (((g - ref64).abs() > bnd) | ~torch.isfinite(g)).nonzero()[0].tolist()
    return f"{n}/{g.numel()} elements outside the bound (worst {worst(got.detach().cpu(), ref64, bnd):.3g} x), first {w}"


# ---------------------------------------------------------------------------------------------------- full-mantissa family
def gauss_operands(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((M, K), generator=g).to(BF16).to(F64), torch.randn((N, K), generator=g).to(BF16).to(F64)


def gauss_ref(A, B):
    """-> (C64, sum_k |a_k b_k|)"""
    return A @ B.T, A.abs() @ B.abs().T


def gauss_bound(C64, terms, dtype):
    return E[dtype] * C64.abs() + a_gemm() * terms + TINY


def blocked_fp32(A, B, step=32):
    """numpy restatement of the kernels' accumulation: the 32-deep block products added to an fp32 accumulator in K order"""
    a, b = A.numpy().astype(np.float32), B.numpy().astype(np.float32)
    acc = np.zeros((a.shape[0], b.shape[0]), dtype=np.float32)
    for k0 in range(0, a.shape[1], step):
        acc = acc + (a[:, k0:k0 + step] @ b[:, k0:k0 + step].T).astype(np.float32)
    return torch.from_numpy(acc)


def measure_a_gemm():
    worst_ratio = 0.0
    for i, (M, N, K) in enumerate(GAUSS_SHAPES):
        A, B = gauss_operands(M, N, K, 50 + i)
        C64, terms = gauss_ref(A, B)
        for got in (A.to(F32) @ B.to(F32).T, blocked_fp32(A, B)):
            worst_ratio = max(worst_ratio, float(((got.to(F64) - C64).abs() / (terms + TINY)).max()))
    return worst_ratio


# ------------------------------------------------------------------------------------------------------- epilogue references
def within_rounded_interval(got, lo64, hi64, dtype):
    """None when rd(lo) <= got <= rd(hi) element-wise (lo <= hi: the interval an uncertain fp32 factor leaves the fp32 value in;
    where it holds no rounding boundary the two ends coincide and the comparison is bit-exact)"""
    g = got.detach().cpu().to(F64)
    a, b = rd(torch.minimum(lo64, hi64), dtype), rd(torch.maximum(lo64, hi64), dtype)
    wrong = ~((g >= a) & (g <= b))
    if not wrong.any():
        return None
    m, n = (int(i) for i in wrong.nonzero()[0])
    return f"{int(wrong.sum())}/{wrong.numel()} outside; first [{m}, {n}]: got {float(g[m, n])!r}, want {float(a[m, n])!r}..{float(b[m, n])!r}"


def rope_fused_table(cos_t, sin_t, npos, extra=3):
    """bf16 [npos + extra, 96] = cos | -sin | +sin, NaN rows behind the npos the kernel is told about"""
    c, s = cos_t[:npos].to(BF16), sin_t[:npos].to(BF16)
    return torch.cat([torch.cat([c, -s, s], 1), torch.full((extra, 96), NAN, dtype=BF16)], 0).contiguous()
