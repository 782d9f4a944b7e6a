"""TEST-ONLY: float64 references, error bounds, input families and torch restatements of the training attention kernels
(attention_mfma3.hip / attention_mfma.hip: the bf16 MFMA forward, dQ and dK/dV; attention_small.hip: the plain thread-per-row
kernels and the token-level kernels).  tests/test_attention_train_gpu.py runs them against the HIP kernels;
tests/test_attention_bounds_host.py proves on the CPU that the same bounds accept the restatements and reject named wrong
variants of them.  Everything works on CPU and device tensors alike.

References are float64 torch on the exact values the kernels read.  The backward is the closed form with delta = rowsum(dO * O)
taken from the STORED O (the kernels read the rounded O, not the exact one):

    P = softmax(q k^T scale) (causal),  dS = P (dO V^T - delta) scale,  dQ = dS K,  dK = dS^T Q,  dV = P^T dO

Bound of the bf16 MFMA backward, per element of a gradient g with terms t_k (dS_k K_k, dS_k Q_k, P_k dO_k):

    |got - g| <= 1.25 2^-8 (|g| + R) + 1e-3 rms(g) + 64 2^-24 F,          R = sum_k |t_k|

The first two constants are the project's (test_attention_work_order_does_not_change_results, measured on an MI355X at S = 1100:
output rounding + dS / P rounded to bf16 for the MFMA).  The third term is the cancellation in dP - delta: both are 64-term fp32
dot products summed in different orders, each within gamma_64 <= 64 2^-24 of its abs-sum, and the difference is multiplied by
P scale and contracted like dS: F = the contraction with |dS| replaced by P (|dO| |V|^T + sum_c |dO_c| |O_c|) scale (F = 0 for
dV).  Without it the bound is 0 at S = 1 (dS = 0 exactly in the reference) where a correct kernel leaves ~1e-8.
dV is also held to 1.25 2^-8 (|g| + R) alone wherever R > 0: it has no cancellation.
rowscale: the kernels multiply before the output rounding, so the bound is |rowscale| x the unscaled one and a zero row is exactly 0.
Rotation back (store_grad_row): the ROUNDED pair (x1, x2) is rotated by the table ROUNDED to bf16 and rounded again, so with b
the unrotated bounds and c, s the fp32 table values:  pre = (1 + 2^-8) (|c| b1 + |s| b2) + 2^-8 (|c| |x1| + |s| |x2|)  (the second
term is the table's rounding, unit roundoff 2^-8) and the bound is (1 + 2^-8) pre + 2^-8 |y| (one output rounding).

Forward: FWD_BOUND restates tests/test_cache_attention_gpu.py (FWD_BOUND / check_fwd64): |o - o64| <= C_REL |o64| + C_RMS rms(V).
Its bf16 absolute term 3e-3 rms(V) stands for P rounded to bf16 for the PV product and was measured on gaussian rows, whose
softmax is spread out (2^-8 sum_j P_ij |V_j| = 3.1e-3 rms(V) there).  Each p_j is rounded to nearest (unit roundoff 2^-8), so the
rounding the kernel legitimately makes is bounded by 2^-8 sum_j P_ij |V_j|, which exceeds 3e-3 rms(V) where a few keys with large
|V| share a row's mass (the "super" family: the fp32 restatement with that one rounding reaches 1.16 of the old bound at S = 128).
The bf16 absolute term is therefore max(3e-3 rms(V), 2^-8 sum_j P_ij |V_j| + 5e-6 rms(V)) (the last: the fp32 bound's own absolute
term): the old bound wherever it was adequate, the derived rounding term elsewhere.
Its fp32 constants (5e-6) were measured on gaussian rows as well, whose scores are O(1).  A score held in fp32 carries 2^-24 |s| of its
own rounding whatever the order of the 64-term dot, and exp turns that absolute error into a relative one of p: at |s| ~ 16 (the
"super" family) the plain kernel, the fp32 restatement in the kernel's own order (restate_plain_fwd) and the vectorised one all reach
the same 1.066 of the old bound at S = 257, B = H = 3.  The fp32 absolute term therefore gains A_f32(plain_fwd) X(o) with
X(o) = (1 + 2 dmax_i) sum_j P_ij |V_j| (the token-level carrier below) and A_f32 = 4 x the restatement's measured ratio (no
hardware term: the old constants stand for those).

Kernels that compute in fp32 and round only what they store (the plain kernels, the token-level kernels), in the convention of
tests/ref_streamers.py:

    |got - g| <= n_round E_T R + (A_f32 + (depth + 2) 2^-24) X

E_T = 2^-8 (bf16) / 2^-24 (fp32), n_round = 1 (the store; the rounding of the rotated q, k in the bf16 token kernels is shared
exactly with the reference: products of two bf16 values are exact in fp32, so x1 c - x2 s is rounded once however it is
contracted).  X >= R carries every fp32 error of the chain, each relative to the abs-sum it acts on:
  plain backward   X = R + R_A + F.  R_A = the contraction of A_ik |t_k| with A_ik = scale sum_c |q_ic| |k_kc|: an error of the
                   64-term score dot moves exp(s - lse) by its absolute size; F as above (the cancellation term; its factor 64
                   is below depth + 2).  depth = 64 + S: thread per row, a 64-term dot then a sequential sum over <= S keys.
                   P comes from the lse the kernel is handed (it does not renormalise), so the reference uses that lse too.
  token level      the kernels renormalise: with dmax_i = max_j A_ij an error of the scores moves p_ij by <= 2 dmax_i p_ij, and
                   the row's sum of p dp with it.  X(o) = (1 + 2 dmax_i) sum_j p_ij |v_j|;  X(dq_i) = (1 + 2 dmax_i) sum_j G_ij |k_j|,
                   X(dk_j) = sum_i (1 + 2 dmax_i) G_ij |q_i|, G_ij = p_ij (|dO_i| |v_j| + sum_l p_il |dO_i| |v_l|) scale >= |dS_ij|;
                   X(dv_j) = sum_i (1 + 2 dmax_i) p_ij |dO_i|.  depth = 256 + 8 (a 256-term dot, then <= 8 keys).  With RoPE the
                   table is rounded to T once (rope_c / rope_s), |q|, |k| are |x1| |c| + |x2| |s| of the rotation, and the way back
                   combines R and X of the pair by |c|, |s| before the one output rounding.
A_f32 = 4 x the largest ratio |fp32 torch restatement - ref64| / X on this file's own inputs (measure_a_f32(), re-measured by
the host test: a ratio above the recorded one fails it) + 2^-23 per hardware approximation in the kernel's chain:

    op             measured ratio   hw approximations     A_f32
    plain_fwd      8.2e-08          (in FWD_BOUND)        3.28e-07   (restate_plain_fwd; added to FWD_BOUND's fp32 absolute term)
    plain_bwd      3.9e-07          1 (exp)               1.68e-06   (the largest at S = 1: the cancellation of dP - delta, relative to F)
    tok_fwd        6.0e-08          2 (exp, rcp)          4.78e-07
    tok_bwd        9.0e-08          2 (exp, rcp)          5.98e-07

Input families (seeded, pre-rounded to the dtype): "gauss" N(0, 1); "diag" q_i = k_i = 2 u_i; "super" q_i = 2 u_{i+1}, k_j = 2 u_j
(u ~ N(0, 1), 64 wide; token level: 1.5 u, 256 wide): the diagonal, or the masked neighbour i + 1, outweighs every other key of
the row by ~32 (36) in the exponent whatever i is, so a dropped diagonal or a leaked neighbour moves the row by O(1); the score
jumps ~46 binades at the diagonal, which also sends the forward's lazy reference maximum (threshold 2^40) through its slow path.

Accept / reject on the CPU (tests/test_attention_bounds_host.py -s; B * H = 1, every S of the GPU file's lists x the three families;
token level: every T in 1 .. 8, N = H = 3).  Worst accepted err/bound of the restatement, then per wrong variant the smallest, over the
S >= 33 where it changes the arithmetic, of its largest ratio over the families (it agrees bit for bit with the restatement at the
S listed as "no change"):

    restatement accepted     MFMA backward 0.652 (plain, row scale, rotated back, both), MFMA forward 0.723; plain fp32 backward 0.038,
                             forward 0.407; plain bf16 backward 0.929, forward 0.494; token bf16 0.910, token fp32 0.003
    variant                  MFMA (bf16)          plain fp32           plain bf16           no change at S =
    mask_off_by_one_wave     4.6e+16 (S = 63)     7.7e+18 (S = 129)    8.3e+17 (S = 129)    1, 2, 33 (plain: 1)
    drop_diag_wave           97.5 (S = 33)        2.2e+03 (S = 257)    230 (S = 257)        1, 2 (plain: 1)
    drop_half_masked_tile    99.9 (S = 65)        7.6e+03 (S = 257)    248 (S = 257)        -
    drop_last_q_tile         97.5 (S = 193)       7.6e+03 (S = 257)    248 (S = 257)        64, 128, 192, 256
    pad_rows_counted         98.1 (S = 127)       1.8e+04 (S = 63)     254 (S = 63)         64, 128, 192, 256
    delta_unrounded_o        5.32 (S = 33)        cannot show (fp32 O is not rounded)  8.97 (S = 257)   1
    ds_scaled_twice          87.4 (S = 33)        4.5e+03 (S = 257)    213 (S = 257)        -
    rot_wrong_sign           109 (S = 64)         (the plain kernels have no rotation and no row scale)   1
    rot_pos_off_by_one       140 (S = 65)                                                   -
    p_not_rounded            ACCEPTED, largest 0.549 (more precise than the kernel; the bound is one-sided)
    rowscale_after_rounding  largest 0.734: one more rounding of the stored value, at most one ulp, inside the bound everywhere --
                             the bound cannot tell it from the kernel and the host test only reports it
    token level              key_i_plus_1_visible 2.6e+07 (bf16) / 1.5e+08 (fp32) at T = 5, no change at T = 1;
                             t_treated_as_8 5.9e+05 / 5.8e+06 at T = 1, no change at T = 8
    gauss alone lets through 9 of 144 (variant, S) pairs, all of them delta_unrounded_o (0.50 .. 0.95 of the bound at S = 63, 64, 127,
    129, 192, 255, 256, 321, 449): the "diag" family rejects it at every S.

Measured on the MI355X (tests/test_attention_train_gpu.py -s, 2026-10-19; the whole file: 70 cases, 16.4 s of pytest wall time, the
slowest case 1.8 s).  Worst err/bound over all S, (B, H) and forms, per family (gauss / diag / super):

    MFMA backward            dq 0.641 / 0.496 / 0.681   dk 0.652 / 0.616 / 0.707   dv 0.579 / 0.509 / 0.658
      rotated back           dq 0.571 / 0.408 / 0.572   dk 0.605 / 0.350 / 0.642
      with the row scale     dq 0.650 / 0.452 / 0.683   dk 0.652 / 0.570 / 0.690   dv 0.623 / 0.424 / 0.657
    MFMA forward             o 0.756 / 0.859 / 0.927    lse 0.002 / 0.002 / 0.005
    plain fp32               o 0.164, lse 0.533 (all families; o reached 1.066 of FWD_BOUND's unamended fp32 term: see above);
                             backward dq 0.006 / 0.011 / 0.012   dk 0.008 / 0.011 / 0.012   dv 0.016 / 0.046 / 0.019
    plain bf16               o 0.491, lse 0.004; backward dq 0.924 / 0.310 / 0.907   dk 0.969 / 0.570 / 0.920   dv 0.969 / 0.807 / 0.945
                             (one store rounding against E_T R with |g| = R on single-term rows)
    token bf16               o 0.917 / 0.000 / 0.841   dq 0.553 / 0.000 / 0.431   dk 0.640 / 0.000 / 0.485   dv 0.919 / 0.810 / 0.842
    token fp32               all <= 0.002 (the depth rule is a worst case: 266 2^-24 (1 + 2 dmax) against random-walk errors)
    No kernel was outside a bound that its restatement is inside; every bit-equality (NaN pads, B = 1, attn_v3_wps, ops.attn_bwd) held.
"""
from __future__ import annotations

import torch

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
E = {BF16: 2.0 ** -8, F32: 2.0 ** -24}
U24, U23 = 2.0 ** -24, 2.0 ** -23
LOG2E = 1.4426950408889634
HD, SCALE = 64, 0.125
THD, TSCALE = 256, 256 ** -0.5

S_LIST = [1, 2, 33, 63, 64, 65, 97, 127, 128, 129, 191, 192, 193, 255, 256, 257, 321, 449, 515]
PLAIN_S = [1, 63, 64, 65, 129, 257]
FAMILIES = ("gauss", "diag", "super")
WAVE = 1           # the wave (32 rows of every 128-row tile) the one-wave wrong variants act on: rows 32..63, 160..191, ...

C_REL, C_RMS, GAMMA64 = 1.25 * 2.0 ** -8, 1e-3, 64 * U24
# |o - o64| <= C_REL |o64| + C_RMS rms(V); |lse - lse64| <= C_LSE max(1, |lse64|)   (tests/test_cache_attention_gpu.py: FWD_BOUND)
FWD_BOUND = {BF16: (2.0 ** -8, 3e-3, 1e-4), F32: (5e-6, 5e-6, 2e-6)}
# op -> (recorded largest ratio of the fp32 restatement, hardware approximations in the kernel's chain)
A_TABLE = {"plain_fwd": (8.2e-08, 0), "plain_bwd": (3.9e-07, 1), "tok_fwd": (6.0e-08, 2), "tok_bwd": (9.0e-08, 2)}   # measured 7.45e-08, 3.51e-07, 5.33e-08, 8.12e-08
TOK_DEPTH = THD + 8


def a_f32(op):
    ratio, hw = A_TABLE[op]
    return 4 * ratio + hw * U23


def rd(t64, dtype):
    """a float64 value rounded through `dtype` (float64 -> fp32 -> dtype, the kernels' own route from their fp32 registers)"""
    return t64.to(F32).to(dtype).to(F64)


def rms(x):
    return x.pow(2).mean().sqrt().item()


# ------------------------------------------------------------------------------------------------------- event level: layout
def heads(x, B, S, H, dt=F64):
    """[B * S, H * 64] -> [B, H, S, 64]"""
    return x.to(dt).view(B, S, H, HD).transpose(1, 2)


def rows(x):
    """[B, H, S, 64] -> [B * S, H * 64]"""
    B, H, S, _ = x.shape
    return x.transpose(1, 2).reshape(B * S, H * HD)


def split(qkv, B, S, H, dt=F64):
    D = H * HD
    return tuple(heads(qkv[:, i * D:(i + 1) * D], B, S, H, dt) for i in range(3))


def tril(S, device):
    return torch.ones(S, S, dtype=torch.bool, device=device).tril()


def event_inputs(family, B, S, H, dtype, seed, device="cpu"):
    """-> (qkv [B * S, 3 * H * 64], dO [B * S, H * 64]) of `dtype`, drawn on the CPU from `seed`"""
    g = torch.Generator().manual_seed(seed)
    D = H * HD
    qkv = torch.randn((B * S, 3 * D), generator=g)
    do = torch.randn((B * S, D), generator=g)
    if family != "gauss":
        u = torch.randn((B, H, S + 1, HD), generator=g)
        k = 2.0 * u[:, :, :S]
        q = k if family == "diag" else 2.0 * u[:, :, 1:]
        qkv[:, :D], qkv[:, D:2 * D] = rows(q), rows(k)
    return qkv.to(dtype).to(device), do.to(dtype).to(device)


def rowscale_input(M, seed, device="cpu"):
    """fp32 [M] in [0.5, 1.5], with exactly 0.0 and -1.0 on two rows (one row: 0.0)"""
    rs = 0.5 + torch.rand((M,), generator=torch.Generator().manual_seed(seed))
    rs[M // 2] = 0.0
    if M > 1:
        rs[M - 1] = -1.0
    return rs.to(device)


# ------------------------------------------------------------------------------------------------- event level: float64
def fwd64(qkv, B, S, H, scale=SCALE):
    """float64 causal softmax(q k^T scale) v and log-sum-exp over the exact inputs: (o [B * S, D], lse [B, H, S], rms(V),
    sum_j P_ij |V_j| [B * S, D], the same times 1 + 2 dmax_i)"""
    q, k, v = split(qkv, B, S, H)
    m = tril(S, qkv.device)
    s = torch.matmul(q, k.transpose(-1, -2)) * scale
    s = s.masked_fill(~m, float("-inf"))
    p = torch.softmax(s, -1)
    pav = torch.matmul(p, v.abs())
    w = 1.0 + 2.0 * (torch.matmul(q.abs(), k.abs().transpose(-1, -2)) * scale).masked_fill(~m, 0.0).amax(-1, keepdim=True)
    return rows(torch.matmul(p, v)), torch.logsumexp(s, -1), rms(v), rows(pav), rows(w * pav)


def fwd_ratios(o, lse, ref, dtype):
    """(worst err/bound of o, of lse) under FWD_BOUND; o [B * S, D], lse [B, H, S]"""
    o64, lse64, rms_v, pav, xo = ref
    c_rel, c_rms, c_lse = FWD_BOUND[dtype]
    absterm = torch.full_like(o64, c_rms * rms_v)
    if dtype == BF16:   # (the P rounding where the softmax is concentrated: module docstring)
        absterm = torch.maximum(absterm, E[BF16] * pav + 5e-6 * rms_v)
    else:               # (the sequential fp32 score dot, amplified by exp: module docstring)
        absterm = absterm + 4 * A_TABLE["plain_fwd"][0] * xo
    ro = ((o.to(F64) - o64).abs() / (c_rel * o64.abs() + absterm)).max().item()
    rl = ((lse.to(F64) - lse64).abs() / (c_lse * lse64.abs().clamp(min=1.0))).max().item()
    return ro, rl


class Bwd64:
    """float64 backward of one (qkv, dO): the parts that do not depend on the stored O are kept, grads(o) finishes them.
    lse given ([B, H, S]): P = exp(s - lse), what a kernel that is handed lse computes (the plain kernels)."""

    def __init__(self, qkv, do, B, S, H, scale=SCALE, lse=None):
        self.shape, self.scale = (B, S, H), scale
        self.q, self.k, self.v = split(qkv, B, S, H)
        self.do = heads(do, B, S, H)
        s = torch.matmul(self.q, self.k.transpose(-1, -2)) * scale
        m = tril(S, s.device)
        if lse is None:
            self.p = torch.softmax(s.masked_fill(~m, float("-inf")), -1)
        else:
            self.p = torch.exp(s - lse.to(F64)[..., None]) * m
        self.dp = torch.matmul(self.do, self.v.transpose(-1, -2))
        self.adp = torch.matmul(self.do.abs(), self.v.abs().transpose(-1, -2))
        self.a = torch.matmul(self.q.abs(), self.k.abs().transpose(-1, -2)) * scale

    def grads(self, o):
        """-> {name: (g, R, F, R_A)}, each [B * S, D], for delta from this stored o"""
        B, S, H = self.shape
        od = heads(o, B, S, H)
        delta = (self.do * od).sum(-1, keepdim=True)
        adelta = (self.do.abs() * od.abs()).sum(-1, keepdim=True)
        ds = self.p * (self.dp - delta) * self.scale
        fi = self.p * (self.adp + adelta) * self.scale
        q, k, do, p, a = self.q, self.k, self.do, self.p, self.a
        T = lambda x: x.transpose(-1, -2)
        mm = torch.matmul
        out = {"dq": (mm(ds, k), mm(ds.abs(), k.abs()), mm(fi, k.abs()), mm(a * ds.abs(), k.abs())),
               "dk": (mm(T(ds), q), mm(T(ds.abs()), q.abs()), mm(T(fi), q.abs()), mm(T(a * ds.abs()), q.abs())),
               "dv": (mm(T(p), do), mm(T(p), do.abs()), torch.zeros_like(do), mm(T(a * p), do.abs()))}
        return {nm: tuple(rows(x) for x in t) for nm, t in out.items()}


def mfma_bound(g, R, F):
    """the bf16 MFMA backward's bound (module docstring); rms over the whole gradient, as the work-order test takes it"""
    return C_REL * (g.abs() + R) + C_RMS * rms(g) + GAMMA64 * F


def f32_bound(R, X, dtype, op, depth):
    """kernels that compute in fp32 and round what they store (module docstring)"""
    return E[dtype] * R + (a_f32(op) + (depth + 2) * U24) * X


def plain_bound(g, R, F, RA, dtype, S):
    return f32_bound(R, R + RA + F, dtype, "plain_bwd", HD + S)


def _pair(x, B, S, H):
    v = x.view(B, S, H, HD)
    return v[..., :HD // 2], v[..., HD // 2:]


def _tab(t, S):
    return t[:S].to(F64)[None, :, None, :]


def rot_back64(x, cos, sin, B, S, H, sign=1.0, shift=0):
    """the way back of the rotation (by -theta of the row's position) with the table values as given: x [B * S, D] float64"""
    x1, x2 = _pair(x, B, S, H)
    c, s = _tab(cos[shift:], S), sign * _tab(sin[shift:], S)
    return torch.cat((x1 * c + x2 * s, x2 * c - x1 * s), -1).reshape(x.shape)


def rot_bound(b, x, y, cos, sin, B, S, H):
    """bound of the rotated-back gradient y from the bound b of the unrotated x (module docstring)"""
    b1, b2 = _pair(b, B, S, H)
    x1, x2 = _pair(x.abs(), B, S, H)
    c, s = _tab(cos, S).abs(), _tab(sin, S).abs()
    u = E[BF16]
    pre = torch.cat(((1 + u) * (c * b1 + s * b2) + u * (c * x1 + s * x2), (1 + u) * (c * b2 + s * b1) + u * (c * x2 + s * x1)), -1)
    return (1 + u) * pre.reshape(b.shape) + u * y.abs()


def scale_rows(x, rs):
    return x * rs.to(F64)[:, None]


# ----------------------------------------------------------------------------------------------- event level: restatement
WRONG_EVENT = ("mask_off_by_one_wave", "drop_diag_wave", "drop_half_masked_tile", "drop_last_q_tile", "pad_rows_counted",
               "delta_unrounded_o", "p_not_rounded", "ds_scaled_twice", "rowscale_after_rounding", "rot_wrong_sign",
               "rot_pos_off_by_one")
ACCEPTED_WRONG = ("p_not_rounded",)   # more precise than the kernel: the bound is one-sided


def restate_fwd(qkv, B, S, H, dtype, scale=SCALE):
    """fp32 softmax with the kernels' rounding points (bf16: P rounded for the PV product, O rounded): (o [B * S, D] of dtype,
    lse [B, H, S] fp32, the unrounded o)"""
    q, k, v = split(qkv, B, S, H, F32)
    s = torch.matmul(q, k.transpose(-1, -2)) * scale
    s = s.masked_fill(~tril(S, s.device), float("-inf"))
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - m)
    l = p.sum(-1, keepdim=True)
    pv = torch.matmul(p.to(dtype).to(F32), v) / l
    return rows(pv).to(dtype), (m + torch.log(l)).squeeze(-1), rows(pv)


def restate_plain_fwd(qkv, B, S, H, dtype, scale=SCALE):
    """attn_plain_fwd_kernel in its own order, fp32: q times scale first, the 64-term dot one product after the other, then key by
    key the online softmax (new maximum, both exponentials, l and the accumulator rescaled and added to).  -> (o of dtype, lse)"""
    q, k, v = split(qkv, B, S, H, F32)
    q = q * scale
    s = torch.zeros((B, H, S, S), dtype=F32, device=qkv.device)
    for d in range(HD):
        s = s + q[..., :, None, d] * k[..., None, :, d]
    m = torch.full((B, H, S), float("-inf"), dtype=F32, device=qkv.device)
    l, acc = torch.zeros_like(m), torch.zeros_like(q)
    i = torch.arange(S, device=qkv.device)
    for j in range(S):
        live = i >= j
        nm = torch.maximum(m, s[..., j])
        a, p = torch.exp(m - nm), torch.exp(s[..., j] - nm)
        l = torch.where(live, l * a + p, l)
        acc = torch.where(live[:, None], acc * a[..., None] + p[..., None] * v[..., j:j + 1, :], acc)
        m = torch.where(live, nm, m)
    return rows(acc * (1.0 / l)[..., None]).to(dtype), m + torch.log(l)


def restate_bwd(qkv, o, do, lse, B, S, H, dtype, mode, scale=SCALE, rowscale=None, cos=None, sin=None, wrong=None, o_unrounded=None):
    """The backward kernels' arithmetic in fp32 torch with their rounding points -> dqkv [B * S, 3 D] of dtype.
    mode "mfma" (attn_bwd_dq3_kernel / attn_bwd_dkv3_kernel): p = exp2(s scale log2e - lse log2e); P and the unscaled dS = p (dP -
    delta) rounded to bf16 for the MFMA; the accumulators times scale (x rowscale) rounded; the rotation on the rounded pair with
    the table rounded to bf16, rounded again.  mode "plain" (attn_plain_bwd_*): p = exp(s scale - lse), nothing rounded but the
    store.  `wrong`: one of WRONG_EVENT."""
    assert wrong is None or wrong in WRONG_EVENT
    q, k, v = split(qkv, B, S, H, F32)
    dO, of = heads(do, B, S, H, F32), heads(o_unrounded if wrong == "delta_unrounded_o" else o, B, S, H, F32)
    dev = qkv.device
    i = torch.arange(S, device=dev)[:, None]
    j = torch.arange(S, device=dev)[None, :]
    inwave = (i % 128) // 32 == WAVE
    vis = j <= i
    if wrong == "mask_off_by_one_wave":
        vis = vis | (inwave & (j == i + 1))
    elif wrong == "drop_diag_wave":
        vis = vis & ~(inwave & (j == i))
    elif wrong == "drop_half_masked_tile":
        vis = vis & ~((j >= i // 64 * 64) & (j < i // 64 * 64 + 32))
    vis_kv = vis
    if wrong == "drop_last_q_tile" and S % 64:
        vis_kv = vis & (i < S // 64 * 64)
    s = torch.matmul(q, k.transpose(-1, -2))
    L = lse.to(F32)[..., None]
    if mode == "mfma":
        p = torch.exp2(s * torch.tensor(scale * LOG2E, dtype=F32) - L * torch.tensor(LOG2E, dtype=F32))
    else:
        p = torch.exp(s * scale - L)
    delta = (dO * of).sum(-1, keepdim=True)
    ds = p * (torch.matmul(dO, v.transpose(-1, -2)) - delta)        # unscaled
    if mode == "mfma":
        ds = ds.to(BF16).to(F32)
        if wrong != "p_not_rounded":
            p = p.to(BF16).to(F32)
    T = lambda x: x.transpose(-1, -2)
    dq = torch.matmul(ds * vis, k)
    dk = torch.matmul(T(ds * vis_kv), q)
    dv = torch.matmul(T(p * vis_kv), dO)
    Sp = (S + 63) // 64 * 64
    if wrong == "pad_rows_counted" and Sp > S:   # the pad query rows are copies of row S - 1 (the loads clamp) that see every key
        dk = dk + (Sp - S) * ds[:, :, S - 1, :, None] * q[:, :, S - 1:S]
        dv = dv + (Sp - S) * p[:, :, S - 1, :, None] * dO[:, :, S - 1:S]
    sc = torch.tensor(scale, dtype=F32)
    if wrong == "ds_scaled_twice":
        sc = sc * sc
    rs = None if rowscale is None else rowscale.to(F32)[:, None]
    outs = []
    for nm, acc in (("dq", dq), ("dk", dk), ("dv", dv)):
        f = None if nm == "dv" else sc
        x = rows(acc)
        if wrong == "rowscale_after_rounding" and rs is not None:
            x = ((x * f) if f is not None else x).to(dtype).to(F32) * rs
        else:
            if f is not None and rs is not None:
                x = x * (f * rs)                # (the kernel forms -scale * rowscale first)
            elif f is not None:
                x = x * f
            elif rs is not None:
                x = x * rs
        x = x.to(dtype)
        if cos is not None and nm != "dv":
            shift = 1 if wrong == "rot_pos_off_by_one" else 0
            sign = -1.0 if wrong == "rot_wrong_sign" else 1.0
            x1, x2 = _pair(x.to(F32), B, S, H)
            c = cos[shift:shift + S].to(dtype).to(F32)[None, :, None, :]
            sn = sign * sin[shift:shift + S].to(dtype).to(F32)[None, :, None, :]
            x = torch.cat((x1 * c + x2 * sn, x2 * c - x1 * sn), -1).reshape(x.shape).to(dtype)
        outs.append(x)
    return torch.cat(outs, -1)


def rope_table(hd, npos, device="cpu", theta=10000.0):
    """engine.RopeTable's values: fp32 cos / sin [npos, hd / 2]"""
    inv_freq = 1.0 / (theta ** (torch.arange(0, hd, 2, dtype=torch.int64).float() / hd))
    ang = torch.arange(npos).float()[:, None] * inv_freq[None, :]
    return ang.cos().contiguous().to(device), ang.sin().contiguous().to(device)


def event_check(dqkv, G, D, bound_fn):
    """{name: worst err/bound} of dqkv [M, 3 D] against the grads() dict G under bound_fn(name, g, R, F, RA) -> bound"""
    out = {}
    for n, nm in enumerate(("dq", "dk", "dv")):
        g, R, F, RA = G[nm]
        got = dqkv[:, n * D:(n + 1) * D].to(F64)
        bnd = bound_fn(nm, g, R, F, RA)
        err = (got - g).abs()
        ratio = torch.where(err > 0, err / bnd, torch.zeros_like(err))     # (0 / 0: an exact result is inside a zero bound)
        ratio = torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, float("inf")))
        out[nm] = ratio.max().item()
    return out


# ---------------------------------------------------------------------------------------------------------- token level
def tok_inputs(family, N, T, H, dtype, seed, device="cpu"):
    """-> (qkv [N * T, 3 * H * 256], dO [N * T, H * 256]) of `dtype`"""
    g = torch.Generator().manual_seed(seed)
    D = H * THD
    qkv = torch.randn((N * T, 3 * D), generator=g)
    do = torch.randn((N * T, D), generator=g)
    if family != "gauss":
        u = torch.randn((N, T + 1, H, THD), generator=g)
        k = 1.5 * u[:, :T]
        q = k if family == "diag" else 1.5 * u[:, 1:]
        qkv[:, :D], qkv[:, D:2 * D] = q.reshape(N * T, D), k.reshape(N * T, D)
    return qkv.to(dtype).to(device), do.to(dtype).to(device)


def _tok_heads(x, N, T, H, dt):
    return x.to(dt).view(N, T, H, THD).transpose(1, 2)          # [N, H, T, 256]


def _tok_rows(x):
    N, H, T, _ = x.shape
    return x.transpose(1, 2).reshape(N * T, H * THD)


def _tok_rot(x, c, s, dirn):
    """rope4: partners (e, e + 128); c, s [T, 128] broadcast over [N, H, T, .]"""
    x1, x2 = x[..., :128], x[..., 128:]
    sn = dirn * s
    return torch.cat((x1 * c - x2 * sn, x2 * c + x1 * sn), -1)


def _tok_absrot(x, c, s):
    x1, x2 = x[..., :128], x[..., 128:]
    return torch.cat((x1 * c + x2 * s, x2 * c + x1 * s), -1)


class Tok64:
    """float64 token-level attention (hd = 256, T <= 8) on the exact inputs, with the carriers of its bounds.
    cos / sin (fp32 [>= T, 128]): q, k are rotated by the table rounded to `dtype` and the result is rounded to `dtype`, as the
    kernels do (shared exactly: module docstring); the gradient is the one with respect to the UNROTATED q, k."""

    def __init__(self, qkv, do, N, T, H, dtype, scale=TSCALE, cos=None, sin=None):
        D = H * THD
        q, k, v = (_tok_heads(qkv[:, i * D:(i + 1) * D], N, T, H, F64) for i in range(3))
        dO = _tok_heads(do, N, T, H, F64)
        qa, ka = q.abs(), k.abs()
        self.rot = cos is not None
        if self.rot:
            self.c, self.s = rd(cos[:T].to(F64), dtype), rd(sin[:T].to(F64), dtype)
            qa, ka = _tok_absrot(qa, self.c.abs(), self.s.abs()), _tok_absrot(ka, self.c.abs(), self.s.abs())
            q, k = rd(_tok_rot(q, self.c, self.s, 1.0), dtype), rd(_tok_rot(k, self.c, self.s, 1.0), dtype)
        m = tril(T, qkv.device)
        sc = (torch.matmul(q, k.transpose(-1, -2)) * scale).masked_fill(~m, float("-inf"))
        p = torch.softmax(sc, -1)
        a = torch.matmul(qa, ka.transpose(-1, -2)) * scale
        w = 1.0 + 2.0 * a.masked_fill(~m, 0.0).amax(-1, keepdim=True)        # 1 + 2 dmax_i   [N, H, T, 1]
        self.dims, self.dtype = (N, T, H), dtype
        self.o = _tok_rows(torch.matmul(p, v))
        self.o_R = _tok_rows(torch.matmul(p, v.abs()))
        self.o_X = _tok_rows(w * torch.matmul(p, v.abs()))
        dp = torch.matmul(dO, v.transpose(-1, -2))
        adp = torch.matmul(dO.abs(), v.abs().transpose(-1, -2))
        dsum = (p * dp).sum(-1, keepdim=True)
        ds = p * (dp - dsum) * scale
        G = p * (adp + (p * adp).sum(-1, keepdim=True)) * scale
        Tt = lambda x: x.transpose(-1, -2)
        mm = torch.matmul
        self.g = {"dq": mm(ds, k), "dk": mm(Tt(ds), q), "dv": mm(Tt(p), dO)}
        self.R = {"dq": mm(ds.abs(), ka), "dk": mm(Tt(ds.abs()), qa), "dv": mm(Tt(p), dO.abs())}
        self.X = {"dq": w * mm(G, ka), "dk": mm(Tt(w * G), qa), "dv": mm(Tt(w * p), dO.abs())}
        if self.rot:
            c, s = self.c, self.s
            for nm in ("dq", "dk"):
                self.g[nm] = _tok_rot(self.g[nm], c, s, -1.0)
                self.R[nm] = _tok_absrot(self.R[nm], c.abs(), s.abs())
                self.X[nm] = _tok_absrot(self.X[nm], c.abs(), s.abs())

    def fwd_ratio(self, o):
        bnd = f32_bound(self.o_R, self.o_X, self.dtype, "tok_fwd", TOK_DEPTH)
        return _ratio(o.to(F64), self.o, bnd)

    def bwd_ratios(self, dqkv, rowscale=None):
        N, T, H = self.dims
        D = H * THD
        out = {}
        for n, nm in enumerate(("dq", "dk", "dv")):
            g, R, X = (_tok_rows(x) for x in (self.g[nm], self.R[nm], self.X[nm]))
            bnd = f32_bound(R, X, self.dtype, "tok_bwd", TOK_DEPTH)
            if rowscale is not None:
                g, bnd = scale_rows(g, rowscale), scale_rows(bnd, rowscale.abs())
            out[nm] = _ratio(dqkv[:, n * D:(n + 1) * D].to(F64), g, bnd)
        return out


def _ratio(got, ref, bnd):
    err = (got - ref).abs()
    ratio = torch.where(err > 0, err / bnd, torch.zeros_like(err))
    return torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, float("inf"))).max().item()


WRONG_TOK = ("key_i_plus_1_visible", "t_treated_as_8")


def restate_tok(qkv, do, N, T, H, dtype, scale=TSCALE, cos=None, sin=None, rowscale=None, wrong=None):
    """tokattn_fwd_kernel / tokattn_bwd_kernel in fp32 torch with their rounding points (rnd<T> of the table and of the rotated
    q, k; stp<T> of o, dq, dk, dv) -> (o [N * T, D], dqkv [N * T, 3 D]) of dtype.  `wrong`: one of WRONG_TOK ("t_treated_as_8":
    the sequences are read as octets -- rows of the next sequences take the places of positions T .. 7, zeros behind the last)."""
    assert wrong is None or wrong in WRONG_TOK
    D = H * THD
    Tn = T
    if wrong == "t_treated_as_8" and T < 8:
        rows_ = torch.arange(N, device=qkv.device)[:, None] * T + torch.arange(8, device=qkv.device)[None, :]
        pad = lambda x: torch.cat((x, torch.zeros((8, x.shape[1]), dtype=x.dtype, device=x.device)))[rows_.reshape(-1)]
        qkv, do, Tn = pad(qkv), pad(do), 8
    q, k, v = (_tok_heads(qkv[:, i * D:(i + 1) * D], N, Tn, H, F32) for i in range(3))
    dO = _tok_heads(do, N, Tn, H, F32)
    if cos is not None:
        c, s = cos[:Tn].to(dtype).to(F32), sin[:Tn].to(dtype).to(F32)
        q, k = _tok_rot(q, c, s, 1.0).to(dtype).to(F32), _tok_rot(k, c, s, 1.0).to(dtype).to(F32)
    m = tril(Tn, qkv.device)
    if wrong == "key_i_plus_1_visible":
        m = torch.ones(Tn, Tn, dtype=torch.bool, device=qkv.device).tril(1)
    sc = (torch.matmul(q, k.transpose(-1, -2)) * scale).masked_fill(~m, float("-inf"))
    p = torch.exp(sc - sc.amax(-1, keepdim=True))
    p = p * (1.0 / p.sum(-1, keepdim=True))
    o = torch.matmul(p, v)
    dp = torch.matmul(dO, v.transpose(-1, -2))
    ds = p * (dp - (p * dp).sum(-1, keepdim=True)) * scale
    Tt = lambda x: x.transpose(-1, -2)
    dq, dk, dv = torch.matmul(ds, k), torch.matmul(Tt(ds), q), torch.matmul(Tt(p), dO)
    if cos is not None:
        dq, dk = _tok_rot(dq, c, s, -1.0), _tok_rot(dk, c, s, -1.0)
    out = torch.cat([_tok_rows(x) for x in (dq, dk, dv)], -1)
    o = _tok_rows(o)
    if Tn != T:
        keep = (torch.arange(N, device=qkv.device)[:, None] * 8 + torch.arange(T, device=qkv.device)[None, :]).reshape(-1)
        out, o = out[keep], o[keep]
    if rowscale is not None:
        out = out * rowscale.to(F32)[:, None]
    return o.to(dtype), out.to(dtype)


# ------------------------------------------------------------------------------------------------------- A_f32, measured
def measure_a_f32():
    """{op: largest |fp32 restatement - ref64| / X} on this file's own inputs (CPU, against float64, never against a HIP kernel)"""
    worst = {"plain_fwd": 0.0, "plain_bwd": 0.0, "tok_fwd": 0.0, "tok_bwd": 0.0}
    for S in PLAIN_S:
        for fam in FAMILIES:
            qkv, do = event_inputs(fam, 1, S, 1, F32, 7000 + S)
            ref = fwd64(qkv, 1, S, 1)
            worst["plain_fwd"] = max(worst["plain_fwd"], _ratio(restate_plain_fwd(qkv, 1, S, 1, F32)[0].to(F64), ref[0], ref[4]))
            o, lse, _ = restate_fwd(qkv, 1, S, 1, F32)
            got = restate_bwd(qkv, o, do, lse, 1, S, 1, F32, "plain")
            G = Bwd64(qkv, do, 1, S, 1, lse=lse).grads(o)
            r = event_check(got, G, HD, lambda nm, g, R, F, RA: R + RA + F)
            worst["plain_bwd"] = max(worst["plain_bwd"], *r.values())
    for T in range(1, 9):
        for fam in FAMILIES:
            for rope in (False, True):
                cos, sin = rope_table(THD, 8) if rope else (None, None)
                qkv, do = tok_inputs(fam, 3, T, 3, F32, 7100 + T)
                o, dqkv = restate_tok(qkv, do, 3, T, 3, F32, cos=cos, sin=sin)
                ref = Tok64(qkv, do, 3, T, 3, F32, cos=cos, sin=sin)
                worst["tok_fwd"] = max(worst["tok_fwd"], _ratio(o.to(F64), ref.o, ref.o_X))
                for n, nm in enumerate(("dq", "dk", "dv")):
                    r = _ratio(dqkv[:, n * 3 * THD:(n + 1) * 3 * THD].to(F64), _tok_rows(ref.g[nm]), _tok_rows(ref.X[nm]))
                    worst["tok_bwd"] = max(worst["tok_bwd"], r)
    return worst
