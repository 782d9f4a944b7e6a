"""The definition of the log-likelihoods the decode pool reports, in torch on the CPU: the single statement the LOGP
forms of the fused sampler (loss_optim.hip, mh_sample_top_p_k_rows_logp / mh_sample_top_p_k_seeded_logp), ``DecodePool.logprobs`` and
``MIDIModel.score`` are held to.  Test infrastructure only.

For a logits row z[0:V] and an id c:

    logp(z, c) = z_c - log sum_{v < V} exp(z_v)

the values read as stored (bf16 or fp32); padding columns V..ldl-1 never enter.  It is the MODEL's log-probability: temperature,
top-p, top-k, the grammar mask, the ban mask, the seed and the row have no part in it.  For an event e (8 tokens, e_0 the event id)

    ll(e) = sum_{i = 0..arity(e_0)} logp(z_i, e_i)

EOS counts position 0 only; positions past the arity hold the pad id and count nothing (ignore_index = pad of the training loss).

Also here: ``logp64`` (float64, the reference), ``kernel_order`` (an fp32 restatement of the statistics pass of the sampler in its
own operation order), the bound ``bound`` with its derivation, the row kinds the bound was checked on, and the named wrong kernels
the bound must reject.

THE BOUND.  u = 2^-24 (fp32 unit roundoff), m = max_v z_v, s = sum_v exp(z_v - m) in [1, V]:

    B(z, c) = u ( |z_c - m| + 1.5 (ln V + 2) + 24 + 4 (1 + ln s) )

The kernel computes (z_c - mx) - log(tot), where tot is its fp32 sum of exp(z_v - mx) and mx = m exactly (a maximum rounds nothing).
  * |z_c - m|: z_c - m is one fp32 subtraction (relative error u, the operands are exact) and the final subtraction rounds a result of
    magnitude <= |z_c - m| + ln s once more; the ln s share is in the last term.
  * 1.5 (ln V + 2): every exponential's argument z_v - m' is a rounded fp32 difference (m' the maximum the thread, the wave or the
    block holds at that point) and the partial sums are rescaled by exp(m' - m''), whose arguments are rounded differences too.  An
    argument error of u |z_v - m| moves term v relatively by that much, and the terms enter the sum with weight p_v = exp(z_v - m) / s:
    sum_v p_v (m - z_v) = ln s - H(p) + ... <= ln V.  Three roundings of that kind lie on the path of a value (thread, wave, block),
    each over a part of the distance m - z_v: 1.5 ln V covers them with the +2 for the rescale factors of the three levels.
  * 24: the depth of the summation tree -- 14 values a thread, 6 butterfly levels, 4 wave partials -- each addition one relative u
    on a sum of positive terms, so the relative error of tot is at most 24 u, an absolute error of 24 u in its logarithm.
  * 4 (1 + ln s): expf and logf of the LOGP code are the accurate library functions (1 ulp each, 2 u relative): 2 u relative on
    every term is 2 u on tot and on the log's argument, i.e. 2 u absolute; the log's own error is 2 u ln s; the final subtraction
    rounds the ln s share of the result once more (u ln s); the rest is slack.
Derived, never fitted: checked on the CPU against ``kernel_order`` with torch's fp32 exp / log on ROW_KINDS x SIZES x CHOICES, worst
error 0.46 of the bound on the rows of tests/test_logp_bounds_host.py (which asserts < 1); the GPU's worst fraction is in DESIGN 7.12.
"""
from __future__ import annotations

import math

import torch

U = 2.0 ** -24
NZ, THREADS, LANES, WAVES = 14, 256, 64, 4   # the statistics pass: 14 values a thread and batch, 256 threads, 4 waves of 64
BATCH = NZ * THREADS                         # 3584 ids a batch

SIZES = (64, 257, 3406, 3585, 7169)
ROW_KINDS = ("gauss3", "gauss30", "equal", "spike90", "near50", "uniform100")
CHOICES = ("first", "last", "argmax", "argmin")


def make_row(kind: str, V: int, seed: int = 0) -> torch.Tensor:
    """a bf16-valued fp32 row [V] of the named kind (exactly representable in either activation dtype)"""
    g = torch.Generator().manual_seed(1000 * seed + V)
    if kind == "gauss3":
        z = torch.randn(V, generator=g) * 3
    elif kind == "gauss30":
        z = torch.randn(V, generator=g) * 30
    elif kind == "equal":
        z = torch.full((V,), 1.25)
    elif kind == "spike90":
        z = torch.randn(V, generator=g)
        z[int(torch.randint(V, (1,), generator=g))] = 90.0
    elif kind == "near50":
        z = 50 + torch.randn(V, generator=g) * 0.01
    elif kind == "uniform100":
        z = -100 * torch.rand(V, generator=g)
    else:
        raise KeyError(kind)
    return z.bfloat16().float()


def choose(z: torch.Tensor, how: str) -> int:
    return {"first": 0, "last": z.numel() - 1, "argmax": int(z.argmax()), "argmin": int(z.argmin())}[how]


def logp64(z: torch.Tensor, c, V: int = None) -> torch.Tensor:
    """z [..., >= V] (any float dtype, read as stored), c int64 [...] (or an int) -> float64 [...]: z_c - log sum_{v < V} exp(z_v)"""
    V = z.shape[-1] if V is None else V
    zd = z[..., :V].double()
    c = torch.as_tensor(c, dtype=torch.int64).expand(zd.shape[:-1])
    return zd.gather(-1, c[..., None])[..., 0] - torch.logsumexp(zd, dim=-1)


def stats64(z: torch.Tensor, V: int = None):
    """-> (m, s) float64 of the row: max and sum exp(z - m)"""
    V = z.shape[-1] if V is None else V
    zd = z[..., :V].double()
    m = zd.amax(-1)
    return m, (zd - m[..., None]).exp().sum(-1)


def bound(z: torch.Tensor, c, V: int = None) -> torch.Tensor:
    """B(z, c), float64 [...] (the module docstring has the derivation)"""
    V = z.shape[-1] if V is None else V
    m, s = stats64(z, V)
    c = torch.as_tensor(c, dtype=torch.int64).expand(m.shape)
    zc = z[..., :V].double().gather(-1, c[..., None])[..., 0]
    return U * ((zc - m).abs() + 1.5 * (math.log(V) + 2) + 24 + 4 * (1 + s.log()))


def event_ll(logp_tokens, event, arity, eos_id: int) -> float:
    """ll of one event from its 8 per-token values: positions 0..arity(e_0), EOS position 0 alone"""
    e0 = int(event[0])
    n = 1 if e0 == eos_id else 1 + int(arity[e0])
    return float(sum(float(x) for x in logp_tokens[:n]))


def kernel_order(z: torch.Tensor, c: int, V: int = None, dtype=torch.float32, rescale: bool = True, batches: int = None,
                 temp: float = None) -> torch.Tensor:
    """one row z [>= V] through the statistics pass in the kernel's order, in ``dtype`` arithmetic (fp32: the restatement; float64
    with a flag changed: a named wrong kernel).  Thread t of 256 holds ids base + t + 256 i, i < 14, of each batch of 3584:
    batch max, running (m, s) rescaled when the max grows, 14 sequential additions; wave: max, s exp(m - wm), xor butterfly 32..1;
    block: max of the 4 partials, their rescaled sum in wave order; (z_c - mx) - log(tot).
    ``rescale=False``: the running sum is NOT rescaled when a later batch raises the maximum.  ``batches``: only that many batches
    are read.  ``temp``: the statistics are taken on z / temp (the chosen logit stays raw)."""
    V = z.shape[-1] if V is None else V
    zf = z[:V].to(dtype)
    zs = zf / temp if temp is not None else zf
    nb = (V + BATCH - 1) // BATCH
    pad = torch.full((nb * BATCH,), -math.inf, dtype=dtype)
    pad[:V] = zs
    vals = pad.view(nb, NZ, THREADS)
    ninf = torch.tensor(-math.inf, dtype=dtype)
    m = torch.full((THREADS,), -math.inf, dtype=dtype)
    s = torch.zeros(THREADS, dtype=dtype)
    for b in range(nb if batches is None else min(nb, batches)):
        cm = vals[b].amax(0)
        grow = cm > m
        if rescale:
            s = torch.where(grow, s * torch.where(grow, m - cm, torch.zeros_like(m)).exp(), s)
        m = torch.where(grow, cm, m)
        live = m > ninf
        for i in range(NZ):
            s = torch.where(live, s + torch.where(live, vals[b, i] - m, ninf).exp(), s)
    m, s = m.view(WAVES, LANES), s.view(WAVES, LANES)
    wm = m.amax(1)
    live = m > ninf
    v = torch.where(live, s * torch.where(live, m - wm[:, None], ninf).exp(), torch.zeros_like(s))
    lane = torch.arange(LANES)
    o = LANES // 2
    while o > 0:
        v = v + v[:, lane ^ o]
        o >>= 1
    ws = v[:, 0]
    mx = wm.amax()
    tot = torch.zeros((), dtype=dtype)
    for w in range(WAVES):
        tot = tot + ws[w] * (wm[w] - mx).exp()
    return (zf[c] - mx) - tot.log()


# ---- the named wrong kernels: (z [ldl], c, V, ctx) -> float64.  ctx: "mask" (bool [V], the candidates), "temp"
def _lse(x):
    return torch.logsumexp(x.double(), dim=-1)


WRONG = {
    # the denominator over the grammar-masked candidates only
    "lse_candidates": lambda z, c, V, ctx: z[c].double() - _lse(z[:V][ctx["mask"]]),
    # the statistics of the sampler's own pass (z / temp) under the raw chosen logit
    "stats_on_temp": lambda z, c, V, ctx: kernel_order(z, c, V, dtype=torch.float64, temp=ctx["temp"]),
    # the probability under the temperature distribution
    "temp_distribution": lambda z, c, V, ctx: z[c].double() / ctx["temp"] - _lse(z[:V].double() / ctx["temp"]),
    # the padding columns V..ldl-1 in the sum
    "padding_included": lambda z, c, V, ctx: z[c].double() - _lse(z),
    # only the first batch of 3584 ids
    "second_batch_dropped": lambda z, c, V, ctx: kernel_order(z, c, V, dtype=torch.float64, batches=1),
    # the running sum kept as it is when a later batch raises the maximum
    "maxima_not_rescaled": lambda z, c, V, ctx: kernel_order(z, c, V, dtype=torch.float64, rescale=False),
    # the largest logit in place of the chosen id's
    "argmax_logit": lambda z, c, V, ctx: z[:V].double().amax() - _lse(z[:V]),
}
