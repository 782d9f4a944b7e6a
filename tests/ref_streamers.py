"""TEST-ONLY: float64 references, error bounds and input generators of the streaming / reduction kernel tests
(tests/test_streamers_gpu.py runs them against the HIP kernels, tests/test_streamer_bounds_host.py proves on the CPU that
the same bounds reject named wrong kernels and accept the emulation).  Everything works on CPU and device tensors alike.

Bound of a result that is one rounded expression:

    |got - ref64| <= (n_round E_T + A_f32) sum|terms| + TINY

E_T = unit roundoff of the output dtype (2^-8 bf16: 8 significant bits; 2^-24 fp32); n_round = dtype roundings between the last rounding point
kernel and reference share exactly and the output (a shared INTERMEDIATE rounding whose argument carries fp32 error can land
on the neighbouring value: one ulp = 2 E_T, so such a point counts 2); sum|terms| = the absolute values of the added terms
(not |ref64|: the expressions cancel); A_f32 = allowance for the fp32 arithmetic in between, set by measurement:

    A_f32 = 4 x (largest |emu_ops on fp32 inputs - ref64| / sum|terms| on the tests' own inputs) + 2^-23 per hardware
            approximation in the kernel's chain (v_exp_f32, v_rcp_f32, v_rsq_f32, v_log_f32)

plus, where the expression consumes a reduced statistic (the row's sum of squares, the row dot), the reduction rule
(depth + 2) 2^-24 of that statistic.  The table (measured by `measure_a_f32()`, which the host test re-runs: a measured ratio
above the recorded one fails it):

    op            measured ratio   hw approximations        A_f32
    swiglu_fwd    1.5e-07          2 (exp, rcp)             8.38e-07
    swiglu_bwd    1.7e-07          2 (exp, rcp)             9.18e-07
    rmsnorm_fwd   1.7e-07          1 (rsq)                  7.99e-07
    rmsnorm_bwd   1.2e-07          0                        4.80e-07
    rope          1.1e-07          0                        4.40e-07
    softmax       6.8e-08          2 (exp, rcp)             5.10e-07   (per unit of 1 + |z - max|: see softmax_bound)
    adamw (fp32)  1.5e-07          0                        6.00e-07

bf16 AdamW rounds after every operation, and a rounding whose argument differs in the last fp32 bits between two correct
evaluations can land on either neighbour: the bound is ONE bf16 ulp of each output, and the share of elements that differ at
all from emu_ops.adamw stays under ADAMW_DIFF_CAP = max(2 x measured share of emu vs the float64-with-roundings reference,
1e-4).  Measured on the value test's inputs (2051 elements x 3 outputs): 0.0179 -> cap 0.036.  The share is this large
because bf16 operands put m + (1 - b1) (g - m) on exact ties for a few per cent of the elements, and the emulation forms
1 - b1 in double (0.1 rounded to fp32) where the kernel and the reference form 1.f - 0.9f = 0.100000024.
"""
from __future__ import annotations

import math

import torch

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
E = {BF16: 2.0 ** -8, F32: 2.0 ** -24}   # 8 / 24 significant bits: |x - rnd<T>(x)| <= E_T |x|
NVEC = {BF16: 8, F32: 4}          # elements of a 16-byte vector
U24, U23 = 2.0 ** -24, 2.0 ** -23
TINY = 2.0 ** -100                # fp32 flushes below 2^-126; operands of the tests stay below 2^26

# op -> (recorded largest ratio of the fp32 emulation, hardware approximations in the kernel's chain)
A_TABLE = {"swiglu_fwd": (1.5e-07, 2), "swiglu_bwd": (1.7e-07, 2), "rmsnorm_fwd": (1.7e-07, 1), "rmsnorm_bwd": (1.2e-07, 0), "rope": (1.1e-07, 0), "softmax": (6.8e-08, 2), "adamw": (1.5e-07, 0)}
ADAMW_DIFF_MEASURED = 0.018   # measure_adamw_diff(): 0.01788 (b1 = 0.9 puts m + 0.1 (g - m) of bf16 operands on exact ties often)
ADAMW_DIFF_CAP = max(2 * ADAMW_DIFF_MEASURED, 1e-4)
UNDECIDED_REL = 1e-5              # sampler: a top-p cut or a p/q lead closer than this is decided by fp32 summation order


def a_f32(op):
    ratio, hw = A_TABLE[op]
    return 4 * ratio + hw * U23


def f64(t):
    return t.to(F64)


def rd(t64, dtype):
    """a float64 value rounded through `dtype` (float64 -> fp32 -> bf16, the kernels' own route from their fp32 registers)"""
    return t64.to(F32).to(dtype).to(F64)


def ulp(x64, dtype):
    """the spacing of `dtype` at |x|"""
    p = 8 if dtype == BF16 else 24
    _, e = torch.frexp(x64.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(x64), e - p)


def bound(terms, dtype, n_round, a):
    return (n_round * E[dtype] + a) * terms + TINY


def bad(got, ref, bnd):
    """elements outside the bound (a NaN / inf output counts)"""
    g = got.to(F64)
    return int((((g - ref).abs() > bnd) | ~torch.isfinite(g)).sum())


def worst(got, ref, bnd):
    return float(((got.to(F64) - ref).abs() / bnd).max())


def randn(shape, dtype, seed, scale=1.0, device="cpu"):
    g = torch.Generator(device=device).manual_seed(seed)
    return (scale * torch.randn(shape, generator=g, device=device)).to(dtype)


def randu(shape, seed, lo, hi, device="cpu", signed=False):
    g = torch.Generator(device=device).manual_seed(seed)
    t = lo + (hi - lo) * torch.rand(shape, generator=g, device=device)
    if signed:
        t = t * (1.0 - 2.0 * torch.randint(0, 2, shape, generator=g, device=device))
    return t


# ----------------------------------------------------------------------------------------------------------------- AdamW
# The value test's inputs and hyper-parameters.  m has g's sign and p the opposite one, m ~ 0.2 g coef, v ~ 0.3 (g coef)^2: the
# update is 11-21 % of |p| and never cancels, so (a) every effect -- decay 0.95, clip coefficient 0.37, bc1 != bc2 -- moves its
# output by >= 8 ulps (the host test checks it on >= 99 % of elements) and (b) an intermediate rounding that lands on the
# neighbouring bf16 value (at most 2^-7 of the update, the new m or the new v term) moves the output by less than one ulp.
ADAMW_HYPER = (0.0056, 0.9, 0.95, 1e-8, 9.0, 1 - 0.9 ** 3, 1 - 0.95 ** 3)   # lr, b1, b2, eps, wd, bc1, bc2 (step 3)
ADAMW_STEP1 = (0.0056, 0.9, 0.99, 1e-8, 9.0, 0.1, 0.01)                     # the first step's bias corrections
ADAMW_COEF = 0.37
ADAMW_DEAD = 251    # every 251st element has g = m = v = 0: finite, only the decay applied


def adamw_inputs(n, dtype, seed, device="cpu"):
    g = randu((n,), seed + 1, 0.01, 0.03, device, signed=True)
    gr = g * ADAMW_COEF
    m = 0.2 * gr * randu((n,), seed + 2, 0.9, 1.1, device)
    v = 0.3 * gr * gr * randu((n,), seed + 3, 0.9, 1.1, device)
    p = -randu((n,), seed, 0.02, 0.03, device) * g.sign()
    dead = torch.arange(n, device=device) % ADAMW_DEAD == ADAMW_DEAD - 1
    for t in (g, m, v):
        t[dead] = 0.0
    return p.to(dtype), g.to(dtype), m.to(dtype), v.to(dtype)


def _f32(x):
    return torch.tensor(x, dtype=F32)


def adamw_ref(p, g, m, v, hyper, coef, dtype):
    """-> {name: (ref64, sum|terms|)}; bf16: rounded at every rnd<T> of adamw_kernel; fp32: unrounded float64.  The scalars
    are the fp32 values the kernel is handed and forms (1.f - b1, 1.f - b2, 1.f - lr wd, lr / bc1, sqrtf(bc2))"""
    lr, b1, b2, eps, wd, bc1, bc2 = (_f32(x) for x in hyper)
    omb1, omb2, b2, eps = float(_f32(1.0) - b1), float(_f32(1.0) - b2), float(b2), float(eps)
    decay = float((1.0 - lr.double() * wd.double()).float())
    step, sq2 = float(lr / bc1), float(bc2.sqrt())
    r = (lambda t: rd(t, dtype)) if dtype == BF16 else (lambda t: t)
    p, g, m, v = f64(p), f64(g), f64(m), f64(v)
    gr = r(g * (1.0 if coef is None else float(_f32(float(coef)))))
    pd = r(p * decay)
    dm = (gr - m) * omb1
    me = r(m + dm)
    vb = r(v * b2)
    ve = r(vb + omb2 * gr * gr)
    den = r(r(r(ve.sqrt()) / sq2) + eps)
    upd = step * (me / den)
    return {"p": (r(pd - upd), pd.abs() + upd.abs()), "m": (me, m.abs() + dm.abs()), "v": (ve, vb.abs() + omb2 * gr * gr)}


def adamw_bad(got, ref, dtype):
    """got = {name: tensor}, ref = adamw_ref(...) -> elements outside the bound, over the three outputs"""
    n = 0
    for k, (r64, terms) in ref.items():
        if dtype == BF16:
            bnd = ulp(torch.maximum(r64.abs(), got[k].to(F64).abs()), BF16)
            bnd = torch.where((r64 == 0) & (got[k].to(F64) == 0), torch.zeros_like(bnd), bnd)
        else:
            bnd = bound(terms, F32, 1, a_f32("adamw"))
        n += bad(got[k], r64, bnd)
    return n


def adamw_diff_share(got, emu_out):
    """share of elements (over p, m, v) whose bits differ from the emulation's"""
    d = sum(int((got[k] != emu_out[k]).sum()) for k in got)
    return d / sum(got[k].numel() for k in got)


# ------------------------------------------------------------------------------------------------------------ reductions
def sumsq_depth(n, dtype):
    """sumsq_partial_kernel: 1024 blocks x 256 lanes, a lane adds N squares per vector step, ceil(nvec / (1024 256)) steps,
    one tail step on block 0; then 6 (wave) + 2 (4 waves) levels, fold_partials_kernel 10 levels, the accumulate add"""
    N = NVEC[dtype]
    return -(-(n // N) // (1024 * 256)) * N + 1 + 6 + 2 + 10 + 1


def sum_depth(n):
    """sum_f32_kernel / count_valid_kernel: one block of 1024 lanes, ceil(n / 1024) serial adds, 6 + 4 tree levels"""
    return -(-n // 1024) + 6 + 4


def reduction_bound(abs_sum, depth):
    return (depth + 2) * U24 * abs_sum + TINY


def census_pattern(n, device="cpu"):
    """small non-zero integers in a fixed pattern (1, 2, 3, 1, ...) and the closed form of their sum and sum of squares: every
    partial sum is an integer below 2^24 for the tests' n, so the result is exact in fp32 whatever the order"""
    x = (1 + torch.arange(n, device=device) % 3).float()
    full, rest = divmod(n, 3)
    return x, 6 * full + (0, 1, 3)[rest], 14 * full + (0, 1, 5)[rest]


# --------------------------------------------------------------------------------------------------------------- SwiGLU
SWIGLU_GATES = [0.0, -0.0, 1e-30, -1e-30, 1e-3, -1e-3, 1.0, -1.0, -1.278, 8.0, -8.0, 20.0, -20.0, 87.0, -87.0, 88.5, -88.5,
                89.0, -89.0, 200.0, -200.0]


def swiglu_inputs(M, I, dtype, seed, device="cpu"):
    return randn((M, 2 * I), dtype, seed, 2.0, device), randn((M, I), dtype, seed + 1, 1.0, device)


def swiglu_fwd_ref(gu, dtype):
    I = gu.shape[1] // 2
    g, u = f64(gu[:, :I]), f64(gu[:, I:])
    a = rd(g * torch.sigmoid(g), dtype) * u
    return a, a.abs()


def _gate_allowance(gu):
    """mh_sigmoid rounds the product g * -log2 e to fp32 before v_exp_f32: 2^-24 |g| log2 e in the exponent, |g| 2^-24 relative
    in the exponential -- an error that grows with |g| and that the emulation (torch.sigmoid) does not have; 1 - sig and
    g (1 - sig) inherit it"""
    return f64(gu[:, : gu.shape[1] // 2]).abs() * U24


def swiglu_fwd_bound(terms, gu, dtype):
    # bf16: rnd<T>(silu) is an intermediate rounding of an fp32-approximate value (2) + the output's (1); fp32: rnd<float> is
    # the identity, one output rounding
    return bound(terms, dtype, 3 if dtype == BF16 else 1, a_f32("swiglu_fwd") + _gate_allowance(gu))


def swiglu_bwd_ref(gu, da):
    """-> (dgu64, terms): d gate = d u sig (1 + g (1 - sig)) cancels near g = -1.278; terms keeps both addends"""
    I = gu.shape[1] // 2
    g, u, d = f64(gu[:, :I]), f64(gu[:, I:]), f64(da)
    sig = torch.sigmoid(g)
    dg = d * u * (sig * (1 + g * (1 - sig)))
    tg = (d * u * sig).abs() * (1 + (g * (1 - sig)).abs())
    du = d * g * sig
    return torch.cat([dg, du], 1), torch.cat([tg, du.abs()], 1)


def swiglu_bwd_bound(terms, gu, dtype):
    ga = _gate_allowance(gu)
    return bound(terms, dtype, 1, a_f32("swiglu_bwd") + torch.cat([ga, ga], 1))


# -------------------------------------------------------------------------------------------------------------- RMSNorm
RMS_EPS = 1e-6


def rms_inputs(M, D, dtype, seed, device="cpu"):
    """x, w (spread 0.5 around 1, so that a forgotten weight shows), dy, dres"""
    return (randn((M, D), dtype, seed, 2.0, device), (1 + 0.5 * randn((D,), F32, seed + 1, 1.0, device)).to(dtype),
            randn((M, D), dtype, seed + 2, 1.0, device), randn((M, D), dtype, seed + 3, 1.0, device))


def rms_row_depth(D, dtype):
    """a lane adds ceil(D / 64) products serially (N per 16-byte chunk), then the 6-level wave tree; / D, + eps (or the dot's
    / D) on top"""
    return -(-D // 64) + 6 + 2


def rstd_ref(x, eps=RMS_EPS):
    x = f64(x)
    return torch.rsqrt((x * x).sum(-1) / x.shape[1] + eps)


def rstd_bound(rstd64, D, dtype):
    # the sum's relative error is halved by the rsqrt; v_rsq_f32 1 ulp; the stored value's rounding
    return ((rms_row_depth(D, dtype) + 2) * U24 / 2 + U23 + U24) * rstd64


def rmsnorm_fwd_ref(x, w, dtype, eps=RMS_EPS):
    r = rstd_ref(x, eps)
    y = f64(w) * rd(f64(x) * r[:, None], dtype)
    return r, y, y.abs()


def rmsnorm_fwd_bound(terms, D, dtype):
    # x * rstd is rounded to T (bf16: an intermediate rounding of an approximate value, 2; fp32: the product's own rounding, 1)
    # + the output's; rstd carries its own bound
    a = a_f32("rmsnorm_fwd") + (rms_row_depth(D, dtype) + 2) * U24 / 2
    return bound(terms, dtype, 3 if dtype == BF16 else 2, a)


def rmsnorm_bwd_ref(x, w, rstd, dy, dres, dtype):
    """rstd is the kernel's INPUT (fp32, shared exactly).  -> dx64, dx terms, dw64 [D] (this call's column sums), dw terms"""
    x, w, g, r = f64(x), f64(w), f64(dy), f64(rstd)[:, None]
    xh = x * r
    gw = g * w
    dot = (gw * xh).mean(-1, keepdim=True)
    absdot = (gw * xh).abs().mean(-1, keepdim=True)      # what the dot's own reduction error scales with
    dx = r * (gw - xh * dot)
    terms = (r * gw).abs() + (r * xh).abs() * absdot
    if dres is not None:
        dx = dx + f64(dres)
        terms = terms + f64(dres).abs()
    dwt = g * rd(xh, dtype)
    return dx, terms, dwt.sum(0), dwt.abs().sum(0)


def rmsnorm_bwd_bound(terms, D, dtype):
    return bound(terms, dtype, 1, a_f32("rmsnorm_bwd") + (rms_row_depth(D, dtype) + 2) * U24)


def rms_bwd_blocks(M):
    return min(max((M + 3) // 4, 1), 1024)


def colsum_depth(nblk):
    """mh_colsum: stage A (nblk > 32) folds ceil(nblk / 32) rows with 4 lanes per column (serial quarter + 3 adds), stage B
    adds the <= 32 surviving rows serially, + the accumulate add"""
    if nblk <= 32:
        return nblk + 1
    per = -(-nblk // 32)
    return -(-per // 4) + 3 + 32 + 1


def dw_depth(M):
    """rows a wave of mh_rmsnorm_bwd walks + the 4-wave fold + mh_colsum over the block partials"""
    nblk = rms_bwd_blocks(M)
    return -(-M // (4 * nblk)) + 3 + colsum_depth(nblk)


def dw_bound(dw64, terms, M, out_dtype):
    return reduction_bound(terms, dw_depth(M)) + E[out_dtype] * dw64.abs()


def folded_bwd_ref(x, rstd, t, dres):
    """mh_rmsnorm_bwd_folded: dx = t - x (rstd^2 / D) rowdot(t, x) + dres"""
    x, t, r = f64(x), f64(t), f64(rstd)[:, None]
    dot = (t * x).mean(-1, keepdim=True)
    absdot = (t * x).abs().mean(-1, keepdim=True)
    dx = t - x * (r * r * dot)
    terms = t.abs() + x.abs() * r * r * absdot
    if dres is not None:
        dx, terms = dx + f64(dres), terms + f64(dres).abs()
    return dx, terms


def census_rows(M, D, dtype, seed, device="cpu"):
    """the dw census of mh_rmsnorm_bwd: every row of x the same row, dy[m, c] = 1 where c == m mod D.  With an fp32 dw,
    dw[c] = (rows with m == c mod D) * rnd<T>(xhat[c]) exactly: the partial sums are small-integer multiples of one bf16
    (or, for fp32, 12-bit) value"""
    row = randn((D,), dtype, seed, 1.0, device)
    if dtype == F32:
        row = row.to(BF16).to(F32)     # 8 significant bits: count * value stays exact in fp32 whatever the order
    x = row[None, :].expand(M, D).contiguous()
    m = torch.arange(M, device=device)
    dy = torch.zeros((M, D), dtype=dtype, device=device)
    dy[m, m % D] = 1.0
    counts = torch.bincount(m % D, minlength=D).to(F64)
    return x, dy, counts


# ----------------------------------------------------------------------------------------------------------------- RoPE
def rope_ref(qkv, cos_t, sin_t, S, pos0, H, hd, direction, dtype, partner_shift=0, pos_shift=0):
    """-> (out64 [M, 3 H hd], terms).  cos / sin are rounded to T (shared exactly with the kernel); pair (i, i + hd / 2).
    partner_shift / pos_shift restate two wrong kernels for the host test."""
    M, D = qkv.shape[0], H * hd
    pos = pos0 + pos_shift + (torch.arange(M, device=qkv.device) % S)
    c = rd(f64(cos_t[pos]), dtype)[:, None, :]
    s = direction * rd(f64(sin_t[pos]), dtype)[:, None, :]
    out, terms = f64(qkv).clone(), torch.zeros(qkv.shape, dtype=F64, device=qkv.device)
    for part in range(2):
        v = f64(qkv[:, part * D:(part + 1) * D]).view(M, H, hd)
        x1, x2 = v[..., : hd // 2], v[..., hd // 2:]
        if partner_shift:
            x2 = torch.roll(x2, partner_shift, -1)
        out[:, part * D:(part + 1) * D] = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1).reshape(M, D)
        t = (x1 * c).abs() + (x2 * s).abs()
        terms[:, part * D:(part + 1) * D] = torch.cat([t, (x2 * c).abs() + (x1 * s).abs()], -1).reshape(M, D)
    return out, terms


def rope_bound(terms, dtype):
    return bound(terms, dtype, 1, a_f32("rope"))


def rope_tables(hd, npos, device="cpu"):
    """fp32 cos / sin [npos, hd / 2] of base 10000 (any table would do: the kernel reads what it is given)"""
    inv = 10000.0 ** (-torch.arange(0, hd, 2, dtype=F64, device=device) / hd)
    ang = torch.arange(npos, dtype=F64, device=device)[:, None] * inv[None, :]
    return ang.cos().to(F32), ang.sin().to(F32)


# -------------------------------------------------------------------------------------------------------- masked softmax
def softmax_ref(logits, lo, hi, first_mask, V, temp, dtype):
    """-> (probs64 [B, V], z - max [B, V]).  z = rnd<T>(logit / temp), temp the fp32 value the kernel is handed"""
    tf = float(torch.tensor(temp, dtype=F32))
    z = rd(f64(logits[:, :V]) / tf, dtype)
    zm = z - z.max(-1, keepdim=True).values
    e = zm.exp()
    p = e / e.sum(-1, keepdim=True)
    ids = torch.arange(V, device=logits.device)[None, :]
    rng = (ids >= lo[:, None]) & (ids < hi[:, None])
    mask = torch.where(lo[:, None] < 0, first_mask[None, :].bool().expand_as(rng), rng)
    return p * mask, zm


def softmax_bound(p64, zm, V):
    """exp(z - max): the fp32 subtraction and the multiply by log2 e each lose up to 2^-24 |z - max| in the exponent, so the
    allowance grows with 1 + |z - max|; the denominator is a sum of V positive terms (ceil(V / 64) serial + 6 levels); probs
    are fp32 whatever the logits' dtype"""
    return (U24 + a_f32("softmax") * (1 + zm.abs()) + (-(-V // 64) + 6 + 2) * U24) * p64 + TINY


def softmax_inputs(B, V, dtype, seed, device="cpu"):
    """row b of the B rows: kind b % 3 = first-mask row, range row, empty range; row 0's logits reach +-80"""
    logits = randn((B, V + (-V) % 8), dtype, seed, 2.0, device)
    logits[0, 1:V:5] = -80.0
    logits[0, :V:7] = 80.0
    logits[0, 3:V:7] = 79.0    # (one below the maximum: the row still depends on the temperature)
    lo = torch.tensor([(-1, V // 3, V // 2)[b % 3] for b in range(B)], dtype=torch.int32, device=device)
    hi = torch.tensor([(-1, V // 3 + V // 4 + 1, V // 2)[b % 3] for b in range(B)], dtype=torch.int32, device=device)
    fm = (torch.arange(V, device=device) % 3 != 1).to(torch.uint8)
    return logits, lo, hi, fm


# --------------------------------------------------------------------------------------------------------------- sampler
SAMPLER_LENGTHS = {2: [1, 2, 63, 64, 65, 127, 128], 8: [129, 191, 192, 193, 256, 257, 511, 512],
                   32: [513, 1023, 1024, 1025, 2047, 2048]}   # TMAX of the instantiation -> range length per row
SAMPLER_V = 3406


def sampler_case(tmax, dtype, seed, V=SAMPLER_V, top_k=20):
    """One launch of mh_sample_top_p_k at position 1 with synthetic range tables: row b draws from a range of
    SAMPLER_LENGTHS[tmax][b] ids at an odd `lo`; the last row's `hi` is past V (clipped); row 0 is peaked at the lowest id
    of its range and row 1 at the highest (one logit 60 above the rest at temp 0.5: every other probability is 0); row 2
    is left exactly one candidate by the ban mask."""
    lens = SAMPLER_LENGTHS[tmax]
    B = len(lens)
    g = torch.Generator().manual_seed(seed)
    logits = (3.0 * torch.randn((B, V + (-V) % 8), generator=g)).to(dtype)
    lo = torch.tensor([(37 + 101 * b) % 64 + 50 * b + 1 for b in range(B)], dtype=torch.int32)
    lo[2] = lo[1] + lens[1] + 3                              # behind row 1's peak: the ban mask's range holds no peak
    hi = lo + torch.tensor(lens, dtype=torch.int32)
    lo[B - 1] = V - lens[B - 1] + lens[B - 1] // 3          # the last range runs past V
    hi[B - 1] = lo[B - 1] + lens[B - 1]
    ban = torch.zeros(V, dtype=torch.uint8)
    ban[int(lo[2]):int(hi[2])] = 1
    ban[int(lo[2]) + lens[2] // 2] = 0                       # (other rows' ranges overlap the banned ids: fewer candidates)
    for b, c in ((0, int(lo[0])), (1, int(hi[1]) - 1)):
        logits[b, :V] = (logits[b, :V].float().clamp(-4, 4)).to(dtype)
        ban[c] = 0
        logits[b, c] = 64.0
    lo_tab = torch.stack([torch.zeros_like(lo), lo], 1).contiguous()
    hi_tab = torch.stack([torch.zeros_like(hi), hi], 1).contiguous()
    q = torch.empty((B, V)).exponential_(1.0, generator=g)
    return dict(logits=logits, lo_tab=lo_tab, hi_tab=hi_tab, ev=torch.arange(B), q=q, ban=ban, V=V, B=B,
                max_range=max(lens), fm=torch.zeros(V, dtype=torch.uint8), temp=0.5, top_p=0.9, top_k=top_k)


def sampler_emulate(case, emu):
    c = case
    out = torch.empty((c["B"],), dtype=torch.int64)
    emu.sample_top_p_k(c["logits"], c["fm"], c["lo_tab"], c["hi_tab"], c["ev"], 1, c["q"], out, c["V"], c["temp"], c["top_p"],
                       c["top_k"], ban_mask=c["ban"])
    return out


def sampler_undecided(case, emu):
    """rows whose draw fp32 summation order may decide: a top-p cut with |cum - p - top_p| below UNDECIDED_REL, or the two
    largest p / q closer than UNDECIDED_REL relative"""
    c = case
    B, V = c["B"], c["V"]
    lo, hi = c["lo_tab"][c["ev"], 1], c["hi_tab"][c["ev"], 1]
    probs = emu.masked_softmax(c["logits"], lo, hi, c["fm"], torch.empty((B, V)), V, c["temp"]) * (c["ban"] == 0)[None, :]
    ps, _ = torch.sort(probs.to(F64), dim=-1, descending=True, stable=True)
    k = c["top_k"]
    ps = ps[:, :k]
    cut = (torch.cumsum(ps, -1) - ps - c["top_p"]).abs()
    cut = torch.where(ps > 0, cut, torch.ones_like(cut)).min(-1).values
    kept = torch.where(torch.cumsum(ps, -1) - ps > c["top_p"], torch.zeros_like(ps), ps)
    r = kept / kept.sum(-1, keepdim=True) / c["q"][:, :k].to(F64)
    top2 = torch.topk(r, min(2, k), -1).values
    lead = (top2[:, 0] - top2[:, -1]) / top2[:, 0] if k > 1 else torch.ones(B, dtype=F64)
    lead = torch.where(top2[:, -1] > 0, lead, torch.ones_like(lead))     # a lone candidate leads by everything
    return (cut < UNDECIDED_REL * c["top_p"]) | (lead < UNDECIDED_REL)


# ------------------------------------------------------------------------------------------ A_f32: the measurement itself
def measure_a_f32(emu):
    """largest |emu_ops on fp32 inputs - ref64| / sum|terms| per op, on the value tests' small inputs"""
    out = {}

    def ratio(got, ref, terms):
        return float(((got.to(F64) - ref).abs() / (terms + TINY)).max())

    gu, da = swiglu_inputs(5, 24, F32, 24)
    a, d = torch.empty((5, 24)), torch.empty((5, 48))
    out["swiglu_fwd"] = ratio(emu.swiglu_fwd(gu, a), *swiglu_fwd_ref(gu, F32))
    out["swiglu_bwd"] = ratio(emu.swiglu_bwd(gu, da, d), *swiglu_bwd_ref(gu, da))
    rf = rb = 0.0
    for M, D in ((3, 8), (3, 504), (3, 520), (3, 1024)):
        x, w, dy, dres = rms_inputs(M, D, F32, 13)
        y, rstd, dx, dw = torch.empty((M, D)), torch.empty(M), torch.empty((M, D)), torch.zeros(D)
        emu.rmsnorm_fwd(x, w, y, rstd, RMS_EPS)
        _, y64, ty = rmsnorm_fwd_ref(x, w, F32)
        rf = max(rf, ratio(y, y64, ty))
        emu.rmsnorm_bwd(x, w, rstd, dy, dres, dx, dw, False)
        dx64, tx, _, _ = rmsnorm_bwd_ref(x, w, rstd, dy, dres, F32)
        rb = max(rb, ratio(dx, dx64, tx))
    out["rmsnorm_fwd"], out["rmsnorm_bwd"] = rf, rb
    cos_t, sin_t = rope_tables(64, 40)
    qkv = randn((7, 3 * 3 * 64), F32, 17)
    out["rope"] = ratio(emu.rope_(qkv.clone(), cos_t, sin_t, 5, 3, 3, 64, 1), *rope_ref(qkv, cos_t, sin_t, 5, 3, 3, 64, 1, F32))
    logits, lo, hi, fm = softmax_inputs(3, 65, F32, 36)
    p = emu.masked_softmax(logits, lo, hi, fm, torch.empty((3, 65)), 65, 1.3)
    p64, zm = softmax_ref(logits, lo, hi, fm, 65, 1.3, F32)
    out["softmax"] = float(((p.to(F64) - p64).abs() / ((1 + zm.abs()) * p64 + TINY)).max())
    out["adamw"] = 0.0
    for hyper in (ADAMW_HYPER, ADAMW_STEP1):
        p_, g_, m_, v_ = adamw_inputs(256 * 4 + 3, F32, 28)
        ref = adamw_ref(p_, g_, m_, v_, hyper, ADAMW_COEF, F32)
        emu.adamw(p_, g_, m_, v_, *hyper, torch.tensor([ADAMW_COEF]))
        out["adamw"] = max([out["adamw"]] + [ratio(t, *ref[k]) for k, t in (("p", p_), ("m", m_), ("v", v_))])
    return out


def measure_adamw_diff(emu):
    """share of elements on which emu_ops.adamw (bf16) differs from the float64-with-roundings reference"""
    p, g, m, v = adamw_inputs(256 * 8 + 3, BF16, 28)
    ref = adamw_ref(p, g, m, v, ADAMW_HYPER, ADAMW_COEF, BF16)
    emu.adamw(p, g, m, v, *ADAMW_HYPER, torch.tensor([ADAMW_COEF]))
    d = sum(int((f64(t) != ref[k][0]).sum()) for k, t in (("p", p), ("m", m), ("v", v)))
    return d / (3 * p.numel())
