"""The definition of the 8-bit event-level K/V cache, in torch on the CPU: the single statement the kernels of
attention_kvq.hip are held to, bit for bit.  Test infrastructure only.

Q(x) of a 64-element row x (bf16 values read as fp32):
    amax = max_e |x_e|;  s = amax / 448 as an IEEE fp32 division, s = 1 when amax == 0;
    y_e = clamp(x_e / s, -448, 448), an IEEE fp32 division;  code_e = y_e rounded to nearest even in e4m3fn, subnormals kept.
D(code, s)_e = float(code_e) * s.  The clamp keeps the conversion away from any overflow rule; the NaN codes 0x7F / 0xFF never appear.

Also here: a float64 single-query attention over exactly dequantized values (the reference of the decode bound), a torch restatement of
the decode step in the kernel's operation order (fp32), and the named wrong variants the bound must reject."""
from __future__ import annotations

import torch

FP8_MAX = 448.0
F8 = torch.float8_e4m3fn

# the decode kernel's loop constants (attention_kvq.hip): 4 lanes per key, 16 keys per wave and round, 4 waves, UNR rounds per step
LPK, KPW, WAVES, UNR = 4, 16, 4, 4
ROUND = WAVES * KPW          # keys per round of the block
STEP = ROUND * UNR           # keys per step (one register set)
CYCLE = 2 * STEP             # keys per two-set cycle


def quantize(x: torch.Tensor, rounding: str = "nearest"):
    """x [..., 64] (any float dtype; read as fp32) -> (codes uint8 [..., 64], s fp32 [...]).  ``rounding="truncate"`` is the named
    wrong variant: the quotient's magnitude rounded towards zero."""
    x = x.float()
    amax = x.abs().amax(-1)
    s = torch.where(amax == 0, torch.ones_like(amax), amax / torch.tensor(FP8_MAX, dtype=torch.float32))
    y = (x / s[..., None]).clamp(-FP8_MAX, FP8_MAX)
    c = y.to(F8)
    if rounding == "truncate":
        over = c.float().abs() > y.abs()
        bits = c.view(torch.uint8)
        c = torch.where(over, bits - 1, bits).view(F8)  # (one code towards zero: the magnitude bits are ordered)
    else:
        assert rounding == "nearest"
    return c.view(torch.uint8).clone(), s


def code_values(codes: torch.Tensor) -> torch.Tensor:
    """uint8 codes -> their e4m3fn values as fp32 (exact)"""
    return codes.contiguous().view(F8).float()


def dequantize(codes: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """D(code, s) in fp32: float(code) * s, one IEEE multiply"""
    return code_values(codes) * s.float()[..., None]


def dequantize64(codes: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """D(code, s) exactly (float64: a 4-bit significand times a 24-bit one)"""
    return code_values(codes).double() * s.double()[..., None]


def attend64(q: torch.Tensor, k8, v8, sc, n: int) -> torch.Tensor:
    """single-query attention in float64 over the exactly dequantized rows [0, n) of one (row, head): q [64] (rotated, scaled),
    k8 / v8 uint8 [>= n, 64], sc fp32 [>= n, 2] -> [64] float64"""
    k = dequantize64(k8[:n], sc[:n, 0])
    v = dequantize64(v8[:n], sc[:n, 1])
    p = torch.softmax(k @ q.double(), 0)
    return p @ v


WRONG = ("scales swapped", "scale of j + 1", "truncation", "new row unquantized", "ks in the maximum only", "last cached key skipped")


def decode_step(q: torch.Tensor, k8, v8, sc, pos: int, k_new: torch.Tensor, v_new: torch.Tensor, wrong: str = ""):
    """The fp8 decode step of one (row, head) restated in fp32 in the kernel's operation order: the new row (k_new, v_new: bf16
    values, k rotated) is quantized into row ``pos`` of k8 / v8 / sc IN PLACE, then lane group g of wave w walks keys
    w * 16 + g + 64 r (r = 0, 1, ...) of the cached rows [0, pos) with an online softmax -- score_j = (sum_e q_e float(kcode_je)) ks_j,
    acc_e = acc_e a + (p_j vs_j) float(vcode_je) -- the new row goes to group 0 of wave 0 last, and the groups, then the waves, are
    merged.  q [64] fp32 (rotated, rounded to bf16, scaled).  -> o [64] fp32 (unrounded).  ``wrong``: one of WRONG."""
    assert wrong in WRONG + ("",)
    f32 = torch.float32
    kc, ks = quantize(k_new, "truncate" if wrong == "truncation" else "nearest")
    vc, vs = quantize(v_new, "truncate" if wrong == "truncation" else "nearest")
    k8[pos], v8[pos], sc[pos, 0], sc[pos, 1] = kc, vc, ks, vs
    K, V = code_values(k8[:pos + 1]), code_values(v8[:pos + 1])
    KS, VS = sc[:pos + 1, 0].clone(), sc[:pos + 1, 1].clone()
    if wrong == "scales swapped":
        KS, VS = VS, KS
    if wrong == "scale of j + 1" and pos >= 1:
        KS[:pos], VS[:pos] = sc[1:pos + 1, 0], sc[1:pos + 1, 1]
    if wrong == "new row unquantized":
        K[pos], V[pos], KS[pos], VS[pos] = k_new.float(), v_new.float(), 1.0, 1.0
    ncached = pos - 1 if wrong == "last cached key skipped" else pos
    q = q.to(f32)
    raw = K @ q                                   # (the per-lane partial sums and the two DPP additions: fp32 either way)
    score = raw * KS
    pscore = raw if wrong == "ks in the maximum only" else score   # what the exponent subtracts the maximum from
    # the per-group online softmax, vectorised over the 64 groups: group (w, g) owns keys j with j % 64 == w * 16 + g
    G = ROUND
    m = torch.full((G,), -float("inf"), dtype=f32)
    l = torch.zeros(G, dtype=f32)
    acc = torch.zeros(G, 64, dtype=f32)

    def take(idx, grp):
        nm = torch.maximum(m[grp], score[idx])
        a, p = torch.exp(m[grp] - nm), torch.exp(pscore[idx] - nm)
        l[grp] = l[grp] * a + p
        acc[grp] = acc[grp] * a[:, None] + (p * VS[idx])[:, None] * V[idx]
        m[grp] = nm

    for r0 in range(0, max(ncached, 0), G):
        idx = torch.arange(r0, min(r0 + G, ncached))
        take(idx, idx - r0)
    take(torch.tensor([pos]), torch.tensor([0]))  # the new row: lane group 0 of wave 0
    # merge: groups of a wave by xor 1, 2, 4, 8 of the group index, then the four waves
    m, l, acc = m.view(WAVES, KPW), l.view(WAVES, KPW), acc.view(WAVES, KPW, 64)
    x = 1
    while x < KPW:
        perm = torch.arange(KPW) ^ x
        om, ol, oacc = m[:, perm], l[:, perm], acc[:, perm]
        nm = torch.maximum(m, om)
        a = torch.where(m == -float("inf"), torch.zeros_like(m), torch.exp(m - nm))
        b = torch.where(om == -float("inf"), torch.zeros_like(m), torch.exp(om - nm))
        a, b = torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0)
        l = l * a + ol * b
        acc = acc * a[..., None] + oacc * b[..., None]
        m = nm
        x <<= 1
    wm, wl, wacc = m[:, 0], l[:, 0], acc[:, 0]
    gm = wm.max()
    f = torch.where(wm == -float("inf"), torch.zeros_like(wm), torch.exp(wm - gm))
    return (wacc * f[:, None]).sum(0) / (wl * f).sum()


def decode_lengths(lmax: int) -> list:
    """cached-row counts at the edges of the kernel's loop: keys per round, per step and per two-set cycle, each +-1, plus 0 (a free
    row attends to its own key alone) and lmax - 1"""
    ns = {0, 1, lmax - 1}
    for c in (KPW, ROUND, STEP, CYCLE):
        ns |= {c - 1, c, c + 1}
    return sorted(n for n in ns if 0 <= n <= lmax - 1)
