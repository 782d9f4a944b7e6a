"""Shared by the tests of the 8-bit K/V cache: the decode bound, random decode cases for it, and the fork / hold scenarios on an fp8 pool
(modelled on fork_common.py).  Every function runs on what it is given (the CPU restatement / stand-ins or the kernels) and asserts."""
import numpy as np
import torch

import fork_common as fc
import ragged_common as rc
import ref_kvq

# |o - o64| <= C_REL |o64| + C_ABS max|v^| -- o64: float64 attention over the exactly dequantized rows, the new row included; v^ the
# dequantized values of the pair's keys.
#   C_REL = 2^-8: the bf16 rounding of the output.
#   C_ABS: test_cache_attention_gpu.py gives the bf16-cache kernel 2e-6 for its fp32 arithmetic (scores over 64 products, __expf, the
#   online rescale, the merges).  This kernel runs the same arithmetic plus two fp32 multiplies per key:
#     * score_j = raw_j ks_j: one more rounding of the score, |d score_j| <= 2^-24 |score_j|.  A score moved by d moves its weight by
#       the factor e^d, and weights moved by factors within e^+-d move the normalised output by at most 2 d max|v^|: with
#       |score_j| <= S_MAX that is 2 S_MAX 2^-24 max|v^|;
#     * p_j vs_j: a relative 2^-24 on one term of the sum, at most 2^-24 max|v^| in all.
#   The cases below keep |score| <= S_MAX = 32 (random: <= 8; the one-hot probe: 30).
S_MAX = 32.0
C_REL = 2.0 ** -8
C_ABS = 2e-6 + (2 * S_MAX + 1) * 2.0 ** -24   # 5.87e-6
SCALE = 0.125


def bound_ratio(o: torch.Tensor, o64: torch.Tensor, vmax: float) -> float:
    """the largest |o - o64| / (C_REL |o64| + C_ABS vmax) over the elements (<= 1: inside the bound; NaN / inf -> inf)"""
    err = (o.double() - o64).abs()
    if not torch.isfinite(err).all():
        return float("inf")
    return float((err / (C_REL * o64.abs() + C_ABS * vmax)).max())


def random_case(n_cached: int, lmax: int, seed: int):
    """one (row, head): codes of rows [0, n_cached) random without the NaN codes, scales 2^-6 .. 2^6, rows at or past n_cached NaN
    codes and NaN scales; the new row's k (rotated) and v as bf16; q [64] fp32 = a bf16 vector times SCALE times a power of two that
    keeps every |score| <= 8.  -> (q, k8, v8, sc, k_new, v_new)"""
    g = torch.Generator().manual_seed(seed)
    k8 = torch.randint(0, 256, (lmax, 64), generator=g, dtype=torch.int32)
    v8 = torch.randint(0, 256, (lmax, 64), generator=g, dtype=torch.int32)
    for t in (k8, v8):
        t[(t & 0x7F) == 0x7F] -= 1
        t[n_cached:] = 0x7F
    k8, v8 = k8.to(torch.uint8), v8.to(torch.uint8)
    sc = torch.exp2(torch.rand((lmax, 2), generator=g) * 12 - 6).float()
    sc[n_cached:] = float("nan")
    k_new = (torch.randn(64, generator=g) * 3).bfloat16()
    v_new = (torch.randn(64, generator=g) * 3).bfloat16()
    q = torch.randn(64, generator=g).bfloat16().float()
    kq, ks = ref_kvq.quantize(k_new)
    keys = torch.cat([ref_kvq.dequantize64(k8[:n_cached], sc[:n_cached, 0]), ref_kvq.dequantize64(kq, ks)[None]])
    top = float((keys @ q.double()).abs().max()) * SCALE
    q = q * SCALE * 2.0 ** -max(0, int(np.ceil(np.log2(max(top, 1e-30) / 8))))
    return q, k8, v8, sc, k_new, v_new


def check_restatement(n_cached: int, lmax: int, seed: int, wrong: str = "") -> float:
    """the restatement (or a named wrong variant of it) on a random case, its output rounded to bf16 -> bound_ratio"""
    q, k8, v8, sc, k_new, v_new = random_case(n_cached, lmax, seed)
    o = ref_kvq.decode_step(q, k8, v8, sc, n_cached, k_new, v_new, wrong).bfloat16()
    if wrong in ("truncation",):  # (the reference attends to what a CORRECT append leaves in the cache)
        k8[n_cached], sc[n_cached, 0] = ref_kvq.quantize(k_new)
        v8[n_cached], sc[n_cached, 1] = ref_kvq.quantize(v_new)
    o64 = ref_kvq.attend64(q, k8, v8, sc, n_cached + 1)
    vmax = float(ref_kvq.dequantize64(v8[:n_cached + 1], sc[:n_cached + 1, 1]).abs().max())
    return bound_ratio(o, o64, vmax)


# ---- an fp8 pool: the scenarios of fork_common.py, on decode_pool(..., kv_dtype="fp8")
class _Fp8Pools:
    """``m`` with decode_pool defaulting to kv_dtype="fp8": fork_common's scenarios name no cache dtype"""

    def __init__(self, m):
        self._m = m

    def __getattr__(self, name):
        return getattr(self._m, name)

    def decode_pool(self, *a, **k):
        k.setdefault("kv_dtype", "fp8")
        return self._m.decode_pool(*a, **k)


def child_repeats_parent(m, orc, tok, capacity):
    ses = fc.child_repeats_parent(_Fp8Pools(m), orc, tok, capacity)
    assert ses.kv_dtype == "fp8"
    return ses


def held_then_forked_equals_uninterrupted(m, orc, tok, capacity, length, alone):
    ses = fc.held_then_forked_equals_uninterrupted(_Fp8Pools(m), orc, tok, capacity, length, alone)
    assert ses.kv_dtype == "fp8"
    return ses


def siblings_equal_lone_requests(m, orc, tok, capacity):
    ses = fc.siblings_equal_lone_requests(_Fp8Pools(m), orc, tok, capacity)
    assert ses.kv_dtype == "fp8"
    return ses


def alone_equals_beside_neighbours(m, orc, tok, capacity):
    """a seeded fp8 pool gives a request the same ids alone (row 0) as beside two neighbours, in row 2"""
    x, p, q = rc.prompts(orc, tok, (6, 9, 4), seed0=580)
    with m.decode_pool(fc.ROWS, capacity, seeded=True, kv_dtype="fp8") as pool:
        rid = pool.submit(x, max_len=20, seed=41, **fc.KW)
        fc.drain(pool)
        lone = pool.result(rid)
        ses = pool.ses
    with m.decode_pool(fc.ROWS, capacity, seeded=True, kv_dtype="fp8") as pool:
        pool.submit(p, max_len=26, seed=1, **fc.KW)
        pool.step()   # (the neighbours run first: the request is admitted alone, as above, two steps later)
        pool.submit(q, max_len=23, seed=2, **fc.KW)
        pool.step()
        rid = pool.submit(x, max_len=20, seed=41, **fc.KW)
        pool.step()
        assert pool.requests[rid].row == 2 and pool.ses is ses
        fc.drain(pool)
        got = pool.result(rid)
    assert lone.shape == (20, 8) and fc.same(got, lone), np.argwhere(got != lone)[:4]
    return ses
