"""CPU proof that the bounds of tests/test_streamers_gpu.py bite: the GPU test's own bound functions (tests/ref_streamers.py),
applied at its own inputs (the small shapes; for the large ones a 1/64 slice from the same generator), reject named wrong
kernels restated in torch and accept emu_ops.  Also re-measures what ref_streamers.py records: the fp32 emulation's error
ratios behind every A_f32, the share of elements on which the bf16 AdamW emulation differs from the float64 reference, how far
the AdamW value test's inputs move each output, and the sampler rows whose draw fp32 summation order may decide."""
import math

import pytest
import torch

import emu_ops as emu
import ref_streamers as R
from ref_streamers import BF16, F32, F64, NVEC

DTYPES = [F32, BF16]


def test_recorded_a_f32_ratios_still_hold():
    got = R.measure_a_f32(emu)
    assert set(got) == set(R.A_TABLE)
    for op, ratio in got.items():
        assert ratio <= R.A_TABLE[op][0], f"{op}: the fp32 emulation is {ratio:.3e} sum|terms| from float64, recorded {R.A_TABLE[op][0]:.1e}"
        assert ratio >= R.A_TABLE[op][0] / 8, f"{op}: recorded ratio {R.A_TABLE[op][0]:.1e} is far above the measured {ratio:.3e}"


def test_recorded_adamw_difference_share_still_holds():
    assert R.measure_adamw_diff(emu) <= R.ADAMW_DIFF_MEASURED
    assert R.ADAMW_DIFF_CAP == max(2 * R.ADAMW_DIFF_MEASURED, 1e-4)


# ----------------------------------------------------------------------------------------------------------------- AdamW
def adamw_sizes(dtype):
    N = NVEC[dtype]
    return (256 * N + 3, (8192 * 256 * N + 256 * N + 5) // 64)


def run_adamw(ins, hyper, coef, mutant=None):
    """emu_ops.adamw, or a named wrong kernel -> {p, m, v}"""
    p, g, m, v = (t.clone() for t in ins)
    lr, b1, b2, eps, wd, bc1, bc2 = hyper
    if mutant == "wd ignored":
        wd = 0.0
    if mutant == "bias corrections swapped":
        bc1, bc2 = bc2, bc1
    c = None if (coef is None or mutant == "coef ignored") else torch.tensor([coef])
    emu.adamw(p, g, m, v, lr, b1, b2, eps, wd, bc1, bc2, c)
    if mutant == "m not written":
        m = ins[2].clone()
    if mutant == "v not written":
        v = ins[3].clone()
    if mutant == "last tail element skipped":
        p[-1], m[-1], v[-1] = ins[0][-1], ins[2][-1], ins[3][-1]
    return {"p": p, "m": m, "v": v}


ADAMW_MUTANTS = ["m not written", "v not written", "wd ignored", "coef ignored", "bias corrections swapped", "last tail element skipped"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_adamw_bound_accepts_the_emulation_and_rejects_wrong_kernels(dtype):
    for n in adamw_sizes(dtype):
        ins = R.adamw_inputs(n, dtype, 28)
        for hyper, coef in ((R.ADAMW_HYPER, R.ADAMW_COEF), (R.ADAMW_STEP1, R.ADAMW_COEF)):
            ref = R.adamw_ref(*ins, hyper, coef, dtype)
            good = run_adamw(ins, hyper, coef)
            assert R.adamw_bad(good, ref, dtype) == 0
            for mut in ADAMW_MUTANTS:
                assert R.adamw_bad(run_adamw(ins, hyper, coef, mut), ref, dtype) > 0, (n, mut)


@pytest.mark.parametrize("dtype", DTYPES)
def test_adamw_value_inputs_move_every_output_by_eight_bounds(dtype):
    """the update of p, the change of m and the change of v each exceed the element's bound 8 x on >= 99 % of elements"""
    for n in adamw_sizes(dtype):
        ins = R.adamw_inputs(n, dtype, 28)
        ref = R.adamw_ref(*ins, R.ADAMW_HYPER, R.ADAMW_COEF, dtype)
        for k, old in (("p", ins[0]), ("m", ins[2]), ("v", ins[3])):
            r64, terms = ref[k]
            bnd = R.ulp(r64, BF16) if dtype == BF16 else R.bound(terms, F32, 1, R.a_f32("adamw"))
            share = float(((r64 - old.to(F64)).abs() >= 8 * bnd).double().mean())
            assert share >= 0.99, (k, n, share)


# --------------------------------------------------------------------------------------------------------------- SwiGLU
def swiglu_shapes(dtype):
    return ((1, 8), (3, 8), (5, 24), ((64600 if dtype == BF16 else 32300) // 64, 520))


@pytest.mark.parametrize("dtype", DTYPES)
def test_swiglu_bounds_accept_the_emulation_and_reject_wrong_kernels(dtype):
    rej = {"silu x 1.01": 0, "no g (1 - sig) term": 0, "halves swapped fwd": 0, "halves swapped bwd": 0}
    for i, (M, I) in enumerate(swiglu_shapes(dtype)):
        gu, da = R.swiglu_inputs(M, I, dtype, 24 + 2 * i)
        a64, ta = R.swiglu_fwd_ref(gu, dtype)
        d64, td = R.swiglu_bwd_ref(gu, da)
        fb, bb = R.swiglu_fwd_bound(ta, gu, dtype), R.swiglu_bwd_bound(td, gu, dtype)
        a, d = torch.empty((M, I), dtype=dtype), torch.empty((M, 2 * I), dtype=dtype)
        assert R.bad(emu.swiglu_fwd(gu, a), a64, fb) == 0 and R.bad(emu.swiglu_bwd(gu, da, d), d64, bb) == 0
        g, u, dv = gu[:, :I].float(), gu[:, I:].float(), da.float()
        sig = torch.sigmoid(g)
        n1 = R.bad((((g * sig) * 1.01).to(dtype).float() * u).to(dtype), a64, fb)
        n2 = R.bad(torch.cat([(dv * u * sig).to(dtype), (dv * g * sig).to(dtype)], 1), d64, bb)
        sw = torch.cat([gu[:, I:], gu[:, :I]], 1)
        n3 = R.bad(emu.swiglu_fwd(sw, a), a64, fb)
        n4 = R.bad(emu.swiglu_bwd(sw, da, d), d64, bb)
        for k, n in zip(rej, (n1, n2, n3, n4)):
            rej[k] += n
        if M * I >= 100:
            assert min(n1, n2, n3, n4) > 0, (M, I, n1, n2, n3, n4)
    assert all(n > 0 for n in rej.values()), rej


def test_swiglu_bound_at_the_gate_list_accepts_the_emulation():
    for dtype in DTYPES:
        g = torch.tensor(R.SWIGLU_GATES).to(dtype)
        gu = torch.cat([g, torch.full_like(g, 1.5)])[None, :]
        da = torch.ones((1, g.numel()), dtype=dtype)
        a, d = torch.empty((1, g.numel()), dtype=dtype), torch.empty((1, 2 * g.numel()), dtype=dtype)
        a64, ta = R.swiglu_fwd_ref(gu, dtype)
        d64, td = R.swiglu_bwd_ref(gu, da)
        assert R.bad(emu.swiglu_fwd(gu, a), a64, R.swiglu_fwd_bound(ta, gu, dtype)) == 0
        assert R.bad(emu.swiglu_bwd(gu, da, d), d64, R.swiglu_bwd_bound(td, gu, dtype)) == 0


# -------------------------------------------------------------------------------------------------------------- RMSNorm
def rms_shapes(dtype):
    N = NVEC[dtype]
    return [(3, 8), (3, 504), (3, 520), (3, 64 * N), (3, 64 * N * 2), ((4096 + 5) // 64 + 1, 64 * N * 4), (3, 4096)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_rmsnorm_bounds_accept_the_emulation_and_reject_wrong_kernels(dtype):
    for M, D in rms_shapes(dtype):
        x, w, dy, dres = R.rms_inputs(M, D, dtype, 13)
        r64, y64, ty = R.rmsnorm_fwd_ref(x, w, dtype)
        y, rstd = torch.empty((M, D), dtype=dtype), torch.empty(M)
        emu.rmsnorm_fwd(x, w, y, rstd, R.RMS_EPS)
        assert R.bad(rstd, r64, R.rstd_bound(r64, D, dtype)) == 0 and R.bad(y, y64, R.rmsnorm_fwd_bound(ty, D, dtype)) == 0
        # rstd from D + 8 columns
        xf = x.float()
        r_bad = torch.rsqrt(xf.pow(2).sum(-1) / (D + 8) + R.RMS_EPS)
        y_bad = (w.float() * (xf * r_bad[:, None]).to(dtype).float()).to(dtype)
        assert R.bad(r_bad, r64, R.rstd_bound(r64, D, dtype)) > 0, (M, D)
        assert D > 512 or R.bad(y_bad, y64, R.rmsnorm_fwd_bound(ty, D, dtype)) > 0, (M, D)
        # backward
        dx64, tx, dw64, tw = R.rmsnorm_bwd_ref(x, w, rstd, dy, dres, dtype)
        bx, bw = R.rmsnorm_bwd_bound(tx, D, dtype), R.dw_bound(dw64, tw, M, dtype)
        dx, dw = torch.empty((M, D), dtype=dtype), torch.zeros(D, dtype=dtype)
        emu.rmsnorm_bwd(x, w, rstd, dy, dres, dx, dw, False)
        assert R.bad(dx, dx64, bx) == 0 and R.bad(dw, dw64, bw) == 0
        xh = xf * rstd[:, None]
        dw_bad = (dy[:-1].float() * xh[:-1].to(dtype).float()).sum(0).to(dtype)
        assert R.bad(dw_bad, dw64, bw) > 0, ("dw missing one row", M, D)
        emu.rmsnorm_bwd(x, w, rstd, dy, None, dx, dw, False)
        assert R.bad(dx, dx64, bx) > 0, ("dres not added", M, D)
        gw = dy.float() * w.float()
        c_bad = (dy.float() * xh).mean(-1, keepdim=True)
        dx_bad = (rstd[:, None] * (gw - xh * c_bad) + dres.float()).to(dtype)
        assert R.bad(dx_bad, dx64, bx) > 0, ("w not applied in dot", M, D)
        # the folded form
        f64_, tf = R.folded_bwd_ref(x, rstd, dy, dres)
        assert R.bad(emu.rmsnorm_bwd_folded(x, rstd, dy, dres, dx), f64_, R.rmsnorm_bwd_bound(tf, D, dtype)) == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_dw_census_is_exact_and_sees_one_row(dtype):
    M, D = 4096 + 5, 64 * NVEC[dtype]
    x, dy, counts = R.census_rows(M, D, dtype, 19)
    want = counts * R.rd(x[0].to(F64) * 0.75, dtype)
    dx, dw = torch.empty_like(x), torch.zeros(D)
    emu.rmsnorm_bwd(x, torch.ones(D, dtype=dtype), torch.full((M,), 0.75), dy, None, dx, dw, False)
    assert torch.equal(dw.to(F64), want)
    for drop in (0, M // 2, M - 1):   # one row dropped / doubled
        contrib = (dy[drop].float() * (x[drop].float() * 0.75).to(dtype).float()).to(F64)
        assert not torch.equal(want - contrib, want) and not torch.equal(want + contrib, want)


# ----------------------------------------------------------------------------------------------------------------- RoPE
@pytest.mark.parametrize("dtype", DTYPES)
def test_rope_bound_accepts_the_emulation_and_rejects_wrong_kernels(dtype):
    M, S, pos0 = 7, 5, 3
    N = NVEC[dtype]
    for hd in (16, 32, 64, 256):
        for H in (1, 3):
            cos_t, sin_t = R.rope_tables(hd, pos0 + S + 1)
            qkv = R.randn((M, 3 * H * hd), dtype, 17)
            D2 = 2 * H * hd
            o64, t = R.rope_ref(qkv, cos_t, sin_t, S, pos0, H, hd, 1, dtype)
            bnd = R.rope_bound(t[:, :D2], dtype)
            assert R.bad(emu.rope_(qkv.clone(), cos_t, sin_t, S, pos0, H, hd, 1)[:, :D2], o64[:, :D2], bnd) == 0
            muts = {"dir flipped": dict(direction=-1), "position off by one": dict(direction=1, pos_shift=1)}
            if hd // 2 > N:
                muts["pair partner i + hd/2 - N"] = dict(direction=1, partner_shift=N)
            for name, kw in muts.items():
                wrong = R.rope_ref(qkv, cos_t, sin_t, S, pos0, H, hd, dtype=dtype, **kw)[0].to(dtype)
                assert R.bad(wrong[:, :D2], o64[:, :D2], bnd) > 0, (name, hd, H)


# -------------------------------------------------------------------------------------------------------- masked softmax
@pytest.mark.parametrize("dtype", DTYPES)
def test_softmax_bound_accepts_the_emulation_and_rejects_wrong_kernels(dtype):
    for B in (1, 3, 5):
        for V in (40, 64, 65, 3406):
            logits, lo, hi, fm = R.softmax_inputs(B, V, dtype, 36)
            for temp in (0.5, 1.0, 1.3):
                p64, zm = R.softmax_ref(logits, lo, hi, fm, V, temp, dtype)
                bnd = R.softmax_bound(p64, zm, V)
                assert R.bad(emu.masked_softmax(logits, lo, hi, fm, torch.empty((B, V)), V, temp), p64, bnd) == 0
                mask = (p64 > 0).float()
                e = torch.exp((logits[:, :V].float() / temp).to(dtype).float() - (logits[:, :V].float() / temp).to(dtype).float().max(-1, keepdim=True).values)
                wrong = e * mask / (e * mask).sum(-1, keepdim=True).clamp_min(1e-30)
                assert R.bad(wrong, p64, bnd) > 0, ("denominator over the mask only", B, V, temp)
                if temp != 1.0:
                    wrong = emu.masked_softmax(logits, lo, hi, fm, torch.empty((B, V)), V, 1.0)
                    assert R.bad(wrong, p64, bnd) > 0, ("temperature ignored", B, V, temp)


# ------------------------------------------------------------------------------------------------------------ reductions
def test_census_inputs_see_one_dropped_or_doubled_element():
    """the census results are asserted exactly; in fp32, as the kernels add, a dropped or doubled element always changes them"""
    for n in (1, 3, 7, 9, 1023, 1025, 7169, 100003, 1024 * 256 * 8 + 256 * 8 + 3):
        ones = torch.ones(n)
        pat, want, want_sq = R.census_pattern(n)
        assert float(ones.sum()) == n and float(pat.sum()) == want and float((pat * pat).sum()) == want_sq
        for i in {0, n // 2, n - 1}:
            keep = torch.ones(n, dtype=torch.bool)
            keep[i] = False
            assert float(ones[keep].sum()) != n and float(ones.sum() + ones[i]) != n
            assert float(pat[keep].sum()) != want and float(pat.sum() + pat[i]) != want
            assert float((pat[keep] ** 2).sum()) != want_sq and float((pat ** 2).sum() + pat[i] ** 2) != want_sq


def test_reduction_bounds_accept_torch_sums():
    for n in (1, 1025, 7169, 100003):
        x = R.randn((n,), F32, 90)
        assert abs(float(x.sum()) - float(x.to(F64).sum())) <= R.reduction_bound(float(x.to(F64).abs().sum()), R.sum_depth(n))
        for dtype in DTYPES:
            g = R.randn((n,), dtype, 80, 0.01)
            want = float((g.to(F64) ** 2).sum())
            assert abs(float(g.float().pow(2).sum()) - want) <= R.reduction_bound(want, R.sumsq_depth(n, dtype))
            assert abs(0.999 * want - want) > R.reduction_bound(want, R.sumsq_depth(n, dtype))   # (a 0.1 % error is far outside)


# --------------------------------------------------------------------------------------------------------------- sampler
def sampler_cases():
    for dtype in DTYPES:
        for tmax in (2, 8, 32):
            for top_k in (1, 20, 64):
                yield R.sampler_case(tmax, dtype, 100 + tmax, top_k=top_k)
        yield R.sampler_case(8, dtype, 131, V=3600)


def test_sampler_rows_decided_by_summation_order_are_rare():
    """at most 2 % of the GPU test's rows may be left to fp32 summation order (here: none may, a launch has 6 to 8 rows)"""
    rows = undecided = 0
    for case in sampler_cases():
        u = R.sampler_undecided(case, emu)
        want = R.sampler_emulate(case, emu)
        rows += case["B"]
        undecided += int(u.sum())
        lo, hi = case["lo_tab"][:, 1], case["hi_tab"][:, 1].clamp(max=case["V"])
        assert bool(((want >= lo) & (want < hi)).all())
        assert int(want[0]) == int(lo[0]) and int(want[1]) == int(hi[1]) - 1
        assert int(want[2]) == int(lo[2]) + (int(case["hi_tab"][2, 1]) - int(lo[2])) // 2
        assert int(case["hi_tab"][-1, 1]) > case["V"] and all(int(x) % 64 for x in lo)
    assert undecided <= 0.02 * rows, (undecided, rows)
