"""The flat-buffer and row streamers of csrc/loss_optim.hip and csrc/elementwise.hip at their boundaries: AdamW (native and
master), the gradient norm and the scalar reductions, SwiGLU, RMSNorm forward / backward with its column sums, RoPE, the
cast and copy movers, the masked softmax and the fused sampler.

Every value-producing kernel is held to a float64 torch reference of the operation on the exact values the kernel reads,
rounded where the kernel's comments say rnd<T>, under a bound derived from the kernel's rounding points (tests/ref_streamers.py
holds references, bounds and their derivation; tests/test_streamer_bounds_host.py proves on the CPU that the same bounds
reject named wrong kernels).  emu_ops is the second witness.  Reductions also get census inputs whose result is exact in
fp32, data movement is compared bit for bit, and buffers carry NaN / integer sentinels past what a kernel may write.
Shapes are the smallest that reach each boundary of the launcher named in the test's docstring; N is the 16-byte vector
width (8 bf16, 4 fp32)."""
import math

import pytest
import torch

import emu_mixed
import emu_ops as emu
import ref_streamers as R
from ref_streamers import BF16, F32, F64, NVEC

pytestmark = pytest.mark.gpu

DTYPES = [F32, BF16]
NAN = float("nan")
PAD = 64   # sentinel elements behind (and, for offset slices, before) every written range


@pytest.fixture(scope="module")
def ops():
    import midi_model_amd.ops as real
    return real


@pytest.fixture(scope="module")
def call():
    """the C-ABI itself, for entry points ops.py only wraps together with others (mh_colsum, mh_sumsq's alignment refusal)"""
    from midi_model_amd.lib import lib
    return lib().call


def MH(dtype):
    from midi_model_amd.lib import MH_BF16, MH_F32
    return MH_BF16 if dtype == BF16 else MH_F32


def stream():
    return torch.cuda.current_stream().cuda_stream


def rnd(shape, dtype, seed, scale=1.0):
    return R.randn(shape, dtype, seed, scale, "cpu")


def grnd(shape, dtype, seed, scale=1.0):
    """seeded normal values drawn on the device"""
    return R.randn(shape, dtype, seed, scale, "cuda")


def bits(t):
    """the raw bits of a tensor: NaN sentinels compare equal, -0 and +0 do not"""
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def padded(t, before=0):
    """-> (buffer, view): `t` copied into a NaN-filled buffer with `before` sentinels in front and PAD behind"""
    n = t.numel()
    buf = torch.full((before + n + PAD,), NAN, dtype=t.dtype, device="cuda")
    buf[before:before + n] = t.reshape(-1)
    return buf, buf[before:before + n].view(t.shape)


def sentinels_intact(buf, before, n):
    return bool(torch.isnan(buf[:before]).all()) and bool(torch.isnan(buf[before + n:]).all())


def assert_bound(got, ref, bnd, what):
    n = R.bad(got, ref, bnd)
    assert n == 0, f"{what}: {n} of {ref.numel()} outside the bound, worst {R.worst(got, ref, bnd):.2f} bounds"


# ---------------------------------------------------------------------------------------------------------------- AdamW
def _adamw_case(ops, dtype, n, hyper, coef, seed, before=0):
    """one launch on NaN-fenced buffers -> asserts the bound, the fences, the read-only gradient and (fp32) the second witness;
    bf16: returns (elements whose bits differ from emu_ops.adamw, elements) for the caller's share -- a share is a statement
    about many elements, so the launches of one test are pooled (a buffer of nine elements cannot resolve 3.6 %)"""
    ins = R.adamw_inputs(n, dtype, seed, "cuda")
    bufs, views = zip(*[padded(t, before) for t in ins])
    coef_dev = None if coef is None else torch.tensor([coef], device="cuda")
    ops.adamw(*views, *hyper, coef_dev)
    torch.cuda.synchronize()
    ref = R.adamw_ref(*ins, hyper, coef, dtype)
    got = {"p": views[0], "m": views[2], "v": views[3]}
    assert R.adamw_bad(got, ref, dtype) == 0, (n, hyper, coef)
    e = [t.clone() for t in ins]
    emu.adamw(*e, *hyper, coef_dev)            # (plain torch: runs on the device tensors)
    emu_out = {"p": e[0], "m": e[2], "v": e[3]}
    if dtype != BF16:
        assert R.adamw_bad(emu_out, ref, dtype) == 0
    for b in bufs:
        assert sentinels_intact(b, before, n), "wrote outside its range"
    assert same_bits(views[1], ins[1]), "the gradient is read-only"
    dead = torch.arange(n, device="cuda") % R.ADAMW_DEAD == R.ADAMW_DEAD - 1
    if bool(dead.any()):   # g = m = v = 0: finite, moments stay 0, only the decay applied (exactly nothing when wd = 0)
        assert bool((views[2][dead] == 0).all()) and bool((views[3][dead] == 0).all()) and bool(torch.isfinite(views[0][dead]).all())
        if hyper[4] == 0:
            assert torch.equal(views[0][dead], ins[0][dead])
    return round(R.adamw_diff_share(got, emu_out) * 3 * n), 3 * n


def _assert_share(counts, dtype):
    """the pooled share of elements that differ from the emulation at all (bf16; see ref_streamers.ADAMW_DIFF_CAP)"""
    differ, total = (sum(c) for c in zip(*counts))
    assert dtype != BF16 or differ <= R.ADAMW_DIFF_CAP * total, (differ, total)


@pytest.mark.parametrize("dtype", DTYPES)
def test_adamw_vector_body_tail_and_options(ops, dtype):
    """mh_adamw: blocks = min(max(ceil(n / 4 / 256), 1), 8192), the vector body covers n / N elements, block 0 the n % N tail.
    n in {1, N - 1, N, N + 1, 256 N - 1, 256 N + 3}: tail only, body only, body + tail, one and two blocks; each with the clip
    coefficient given / absent, weight decay on / off, and the first step's bias corrections (0.1, 0.01).
    Bound (ref_streamers.adamw_bad): bf16 -- the float64 reference rounds at every rnd<T>, one bf16 ulp per output and at most
    ADAMW_DIFF_CAP of the elements differing from emu_ops.adamw at all; fp32 -- (2^-24 + A_f32) sum|terms| per output."""
    N = NVEC[dtype]
    no_wd = R.ADAMW_HYPER[:4] + (0.0,) + R.ADAMW_HYPER[5:]
    counts = []
    for i, n in enumerate((1, N - 1, N, N + 1, 256 * N - 1, 256 * N + 3)):
        counts.append(_adamw_case(ops, dtype, n, R.ADAMW_HYPER, R.ADAMW_COEF, 28 + i))
        counts.append(_adamw_case(ops, dtype, n, no_wd, None, 40 + i))
        counts.append(_adamw_case(ops, dtype, n, R.ADAMW_STEP1, R.ADAMW_COEF, 50 + i))
    _assert_share(counts, dtype)   # (over the 18 launches: 3 x 3 x 4123 elements in bf16)


@pytest.mark.parametrize("dtype", DTYPES)
def test_adamw_second_grid_pass(ops, dtype):
    """n = 8192 * 256 * N + 256 * N + 5: the grid is capped at 8192 blocks of 256 lanes, so the lanes of the first block take a
    second grid-stride trip over the 256 vectors past the first pass, and block 0 a 5-element tail (8.4 M fp32 / 16.8 M bf16
    elements; reference and emulation on the device)"""
    _assert_share([_adamw_case(ops, dtype, 8192 * 256 * NVEC[dtype] + 256 * NVEC[dtype] + 5, R.ADAMW_HYPER, R.ADAMW_COEF, 60)], dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_adamw_offset_slice_and_alignment_refusal(ops, dtype):
    """a slice of a larger buffer at a 16-byte multiple works and leaves the elements before it alone; one element off is
    refused by MH_REQUIRE ("16-byte aligned"), nothing written"""
    N = NVEC[dtype]
    _assert_share([_adamw_case(ops, dtype, 256 * N + 3, R.ADAMW_HYPER, R.ADAMW_COEF, 61, before=3 * N)], dtype)
    ins = R.adamw_inputs(64 + 1, dtype, 62, "cuda")
    views = [t[1:] for t in ins]
    before = [t.clone() for t in ins]
    with pytest.raises(RuntimeError, match="aligned"):
        ops.adamw(*views, *R.ADAMW_HYPER, None)
    torch.cuda.synchronize()
    assert all(same_bits(a, b) for a, b in zip(ins, before))


def test_adamw_master_and_grad_fold_past_the_grid_cap_and_tiny(ops):
    """mh_adamw_master / mh_grad_fold_f32: blocks = min(max(ceil(n / 8 / 256), 1), 2048), eight elements per lane and trip.
    n = 2048 * 256 * 8 + 256 * 8 + 5 (second grid pass + tail) and n in {1, 7, 9} (tail only / body + one), NaN fences.
    adamw_master is held to float64 under (2^-24 + A_f32) sum|terms| and to emu_mixed.adamw_master -- the kernel's fp32
    operations in its order -- within 10 x 2^-24 sum|terms| (p's chain is ten fp32 operations, each free to round the other way
    once a multiply-add pair is contracted), p_lo to the bf16 rounding of the kernel's own
    p32 bit for bit; grad_fold is exact."""
    import midi_model_amd.mixed as mixed
    hyper = (1e-3, 0.9, 0.99, 1e-8, 0.01, 1 - 0.9 ** 3, 1 - 0.99 ** 3)
    for n in (1, 7, 9, 2048 * 256 * 8 + 256 * 8 + 5):
        p, g, m, v = (t.float() for t in R.adamw_inputs(n, F32, 70, "cuda"))
        (bp, vp), (bg, vg), (bm, vm), (bv, vv) = (padded(t) for t in (p, g, m, v))
        blo, vlo = padded(torch.zeros(n, dtype=BF16, device="cuda"))
        coef = torch.tensor([0.5], device="cuda")
        mixed.adamw_master(vp, vlo, vg, vm, vv, *hyper, coef)
        torch.cuda.synchronize()
        ep, em, ev, elo = p.clone(), m.clone(), v.clone(), torch.zeros(n, dtype=BF16, device="cuda")
        # (the emulation forms its scalars as CPU fp32 tensors; .item() keeps them fp32 values on any device)
        emu_mixed.adamw_master(ep, elo, g, em, ev, *hyper, coef.cpu())
        ref = R.adamw_ref(p, g, m, v, hyper, 0.5, F32)
        for name, got, want in (("p", vp, ep), ("m", vm, em), ("v", vv, ev)):
            assert_bound(got, want.to(F64), 10 * R.U24 * ref[name][1] + R.TINY, f"adamw_master {name} n={n}")
            assert_bound(got, ref[name][0], R.bound(ref[name][1], F32, 1, R.a_f32("adamw")), f"adamw_master {name} vs float64 n={n}")
        assert same_bits(vlo, vp.to(BF16)) and same_bits(vg, g)
        for b in (bp, bg, bm, bv, blo):
            assert sentinels_intact(b, 0, n)
        for dtype in DTYPES:
            src = grnd((n,), dtype, 71)
            base = grnd((n,), F32, 72)
            bd, vd = padded(base)
            mixed.grad_fold(src, vd, True)
            assert same_bits(vd, base + src.float()) and sentinels_intact(bd, 0, n)
            mixed.grad_fold(src, vd, False)
            assert same_bits(vd, src.float()) and sentinels_intact(bd, 0, n)


# ----------------------------------------------------------------------------------------------------- sumsq, clip_coef
def _sumsq(ops, g, accumulate=False, start=None):
    out = torch.full((3,), NAN, device="cuda")
    if start is not None:
        out[1] = start
    ops.sumsq(g, torch.empty(1024, device="cuda"), out[1:2], accumulate)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[0])) and bool(torch.isnan(out[2]))
    return out[1].item()


@pytest.mark.parametrize("dtype", DTYPES)
def test_sumsq_census_values_accumulate_and_refusal(ops, call, dtype):
    """mh_sumsq: 1024 blocks x 256 lanes over n / N vectors (grid-stride beyond 1024 * 256 vectors), block 0 the tail, then one
    block folds the 1024 partials.  n in {1, N - 1, N + 1} (tail only, body + tail) and 1024 * 256 * N + 256 * N + 3 (second
    pass + tail).  Census: all ones give exactly n, the 1, 2, 3 pattern its closed form (every partial sum an integer below
    2^24).  Values: |got - sum64| <= (depth + 2) 2^-24 sum64 with ref_streamers.sumsq_depth.  accumulate = 1 chained over
    three buffers against the float64 total; the buffer behind n is NaN (an over-read shows); a misaligned pointer is refused."""
    N = NVEC[dtype]
    ns = (1, N - 1, N + 1, 1024 * 256 * N + 256 * N + 3)
    total64, chain, depth = 0.0, None, 0
    for i, n in enumerate(ns):
        _, ones = padded(torch.ones(n, dtype=dtype, device="cuda"))
        assert _sumsq(ops, ones) == float(n)
        pat, _, want_sq = R.census_pattern(n, "cuda")
        _, pat = padded(pat.to(dtype))
        assert _sumsq(ops, pat) == float(want_sq)
        _, g = padded(grnd((n,), dtype, 80 + i, 0.01))
        want = float((g.to(F64) ** 2).sum())
        got = _sumsq(ops, g)
        assert abs(got - want) <= R.reduction_bound(want, R.sumsq_depth(n, dtype)), (n, got, want)
        if i >= 1:   # the chain: accumulate = 0 into the first, accumulate = 1 over the next two
            chain = _sumsq(ops, g, accumulate=chain is not None, start=chain)
            total64 += want
            depth = max(depth, R.sumsq_depth(n, dtype)) + 1
    assert abs(chain - total64) <= R.reduction_bound(total64, depth), (chain, total64)
    buf = torch.ones(64 + 1, dtype=dtype, device="cuda")
    with pytest.raises(RuntimeError, match="unaligned"):
        ops.sumsq(buf[1:], torch.empty(1024, device="cuda"), torch.zeros(1, device="cuda"), False)


def test_clip_coef_edges(ops):
    """mh_clip_coef: norm = sqrt(sumsq), coef = min(1, max_norm / (norm + 1e-6)), three fp32 operations: each output within
    4 x 2^-24 of float64.  sumsq = 0 gives norm 0 and coef exactly 1; norm == max_norm gives a coef just below 1; norm >> max_norm"""
    for ss, max_norm in ((0.0, 1.0), (4.0, 2.0), (1e12, 1.0), (0.3, 1.0)):
        out = torch.full((4,), NAN, device="cuda")
        ops.clip_coef(torch.tensor([ss], device="cuda"), max_norm, out[1:2], out[2:3])
        torch.cuda.synchronize()
        norm64 = math.sqrt(float(torch.tensor(ss, dtype=F32)))
        coef64 = min(1.0, max_norm / (norm64 + float(torch.tensor(1e-6, dtype=F32))))
        coef, norm = out[1].item(), out[2].item()
        assert abs(norm - norm64) <= 4 * R.U24 * norm64 and abs(coef - coef64) <= 4 * R.U24 * coef64, (ss, coef, norm)
        assert bool(torch.isnan(out[0])) and bool(torch.isnan(out[3]))
        if ss == 0.0:
            assert coef == 1.0 and norm == 0.0
        if ss == 4.0:
            assert norm == 2.0 and coef < 1.0


# -------------------------------------------------------------------------------------------------- sum_f32, count_valid
SUM_NS = (1, 1023, 1024, 1025, 7168, 7169, 8191, 8192, 8193, 8192 * 3 + 7169, 100003)


def test_sum_f32_census_and_values(ops):
    """mh_sum_f32: one block of 1024 lanes; the eight-deep unrolled loop runs while i + 7 * 1024 < n (from n = 7169), a
    one-deep loop takes the rest.  n straddles one lane-row (1023 / 1024 / 1025), the unrolled loop's entry (7168 / 7169), its
    second trip (8191 / 8192 / 8193), three trips + a remainder that itself would have entered it, and a large odd n.  All ones
    give exactly n, the integer pattern its closed form; random values stay within (depth + 2) 2^-24 sum|x| of float64."""
    for n in SUM_NS:
        out = torch.full((3,), NAN, device="cuda")
        _, ones = padded(torch.ones(n, device="cuda"))
        ops.sum_f32(ones, out[1:2])
        assert out[1].item() == float(n), n
        pat, want, _ = R.census_pattern(n, "cuda")
        _, pat = padded(pat)
        ops.sum_f32(pat, out[1:2])
        assert out[1].item() == float(want), n
        _, x = padded(grnd((n,), F32, 90))
        ops.sum_f32(x, out[1:2])
        want64 = float(x.to(F64).sum())
        assert abs(out[1].item() - want64) <= R.reduction_bound(float(x.to(F64).abs().sum()), R.sum_depth(n)), n
        assert bool(torch.isnan(out[0])) and bool(torch.isnan(out[2]))


def test_count_valid_exact_and_range(ops):
    """mh_count_valid: the same two loops over int64 targets with an fp32 counter: exact for every n below 2^24, which the
    launcher enforces (n = 2^24 - 1 accepted and exact, 2^24 refused).  All rows ignored: count 0, inv 1."""
    g = torch.Generator(device="cuda").manual_seed(91)
    for n in SUM_NS + ((1 << 24) - 1,):
        t = torch.randint(0, 5, (n + PAD,), generator=g, device="cuda")
        t[n:] = 1   # (valid targets behind the range: an over-read would count them)
        out = torch.full((4,), NAN, device="cuda")
        ops.count_valid(t[:n], 0, out[1:2], out[2:3])
        want = int((t[:n] != 0).sum())
        assert out[1].item() == float(want) and out[2].item() == float(torch.tensor(1.0) / torch.tensor(float(max(want, 1)))), n
        assert bool(torch.isnan(out[0])) and bool(torch.isnan(out[3]))
        t[:n] = 0
        ops.count_valid(t[:n], 0, out[1:2], out[2:3])
        assert out[1].item() == 0.0 and out[2].item() == 1.0, n
    with pytest.raises(RuntimeError, match="out of range"):
        ops.count_valid(torch.zeros(1 << 24, dtype=torch.int64, device="cuda"), 0, out[1:2], out[2:3])


# --------------------------------------------------------------------------------------------------------------- SwiGLU
def _swiglu_case(ops, dtype, M, I, seed, witness=True):
    gu, da = R.swiglu_inputs(M, I, dtype, seed, "cuda")
    ba, a = padded(torch.empty((M, I), dtype=dtype, device="cuda"))
    bd, d = padded(torch.empty((M, 2 * I), dtype=dtype, device="cuda"))
    gu0 = gu.clone()
    ops.swiglu_fwd(gu, a)
    ops.swiglu_bwd(gu, da, d)
    torch.cuda.synchronize()
    a64, ta = R.swiglu_fwd_ref(gu, dtype)
    assert_bound(a, a64, R.swiglu_fwd_bound(ta, gu, dtype), f"swiglu fwd {M}x{I}")
    d64, td = R.swiglu_bwd_ref(gu, da)
    assert_bound(d, d64, R.swiglu_bwd_bound(td, gu, dtype), f"swiglu bwd {M}x{I}")
    assert sentinels_intact(ba, 0, M * I) and sentinels_intact(bd, 0, 2 * M * I) and same_bits(gu, gu0)
    if witness:
        ea, ed = torch.empty_like(a), torch.empty_like(d)
        emu.swiglu_fwd(gu, ea)
        emu.swiglu_bwd(gu, da, ed)
        assert R.bad(ea, a64, R.swiglu_fwd_bound(ta, gu, dtype)) == 0 and R.bad(ed, d64, R.swiglu_bwd_bound(td, gu, dtype)) == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_swiglu_small_shapes_and_refusal(ops, dtype):
    """mh_swiglu_fwd / _bwd: items = M * I / N, blocks = min(ceil(M * (I / 4) / 256), 16384).  (1, 8): one item (fp32: two);
    (3, 8), (5, 24): rows of one and three items, the item -> (row, column) split.  I = 12 is refused (I % 8).
    Bounds: forward (3 E_T bf16 / 1 E_T fp32 + A_f32) |silu(g) u| with silu rounded to T in the reference as in the kernel;
    backward (E_T + A_f32) sum|terms| with d gate's terms |d u sig| (1 + |g (1 - sig)|) (the factor cancels near g = -1.278)."""
    for i, (M, I) in enumerate(((1, 8), (3, 8), (5, 24))):
        _swiglu_case(ops, dtype, M, I, 24 + 2 * i)
    gu = grnd((2, 24), dtype, 30)
    with pytest.raises(RuntimeError, match="bad shape"):
        ops.swiglu_fwd(gu, torch.empty((2, 12), dtype=dtype, device="cuda"))
    with pytest.raises(RuntimeError, match="bad shape"):
        ops.swiglu_bwd(gu, grnd((2, 12), dtype, 31), torch.empty_like(gu))


@pytest.mark.parametrize("dtype", DTYPES)
def test_swiglu_second_grid_pass(ops, dtype):
    """(M, 520) with M * 520 / N just past the 16384 * 256 items of the capped grid: M = 64600 (bf16, 65 items per row) /
    32300 (fp32, 130): the last rows are written by a lane's second grid-stride trip.  float64 on the device."""
    _swiglu_case(ops, dtype, 64600 if dtype == BF16 else 32300, 520, 32, witness=False)


@pytest.mark.parametrize("dtype", DTYPES)
def test_swiglu_gate_saturation(ops, dtype):
    """mh_sigmoid = v_rcp_f32(1 + v_exp_f32(-g log2 e)): for g <= -88.7 the exponential overflows to +inf and the reciprocal
    gives 0, for large g it underflows and the reciprocal gives 1.  Gates from a fixed list (the dtype's neighbours of +-0,
    +-1e-30, +-1e-3, +-1, -1.278, +-8, +-20, +-87, +-88.5, +-89, +-200), up = 1.5, d a = 1: every output finite and within the
    bound; silu(-200) == 0 (either sign), silu(200) u == 300 exactly; the backward's gate factor 0 at -200 and 1 at +200."""
    gates = torch.tensor(R.SWIGLU_GATES).to(dtype)
    I = 24
    assert gates.numel() <= I
    g = torch.zeros(I, dtype=dtype)
    g[:gates.numel()] = gates
    gu = torch.cat([g, torch.full((I,), 1.5, dtype=dtype)])[None, :].cuda()
    a, d = torch.empty((1, I), dtype=dtype, device="cuda"), torch.empty((1, 2 * I), dtype=dtype, device="cuda")
    ops.swiglu_fwd(gu, a)
    ops.swiglu_bwd(gu, torch.ones((1, I), dtype=dtype, device="cuda"), d)
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(d).all())
    a64, ta = R.swiglu_fwd_ref(gu, dtype)
    assert_bound(a, a64, R.swiglu_fwd_bound(ta, gu, dtype), "swiglu fwd, gate list")
    d64, td = R.swiglu_bwd_ref(gu, torch.ones((1, I), dtype=dtype, device="cuda"))
    assert_bound(d, d64, R.swiglu_bwd_bound(td, gu, dtype), "swiglu bwd, gate list")
    ip, im = R.SWIGLU_GATES.index(200.0), R.SWIGLU_GATES.index(-200.0)
    assert a[0, im].item() == 0.0 and a[0, ip].item() == 300.0
    assert d[0, im].item() == 0.0 and d[0, ip].item() == 1.5          # d gate = d a * up * factor
    assert d[0, I + im].item() == 0.0 and d[0, I + ip].item() == 200.0  # d up = d a * silu(g)


# -------------------------------------------------------------------------------------------------------------- RMSNorm
def rms_dims(dtype, backward):
    """every dispatch class of mh_rmsnorm_fwd / _bwd / _bwd_folded: the register forms NCH = 1, 2, 4 (D = 64 N NCH), the
    generic form below the smallest register size (8, 8 * 63), NCH = 3, D no multiple of 64 N (520, 768), D = 4096 (the
    backward's [4][D] fp32 LDS accumulator is exactly 64 KiB) and, for the backward, 4104 and 8192 (above 64 KiB)"""
    N = NVEC[dtype]
    ds = {8, 8 * 63, 520, 768, 64 * N * 3, 4096} | {64 * N * k for k in (1, 2, 4)}
    if backward:
        ds |= {4104, 8192}
    return sorted(ds)


RMS_CASES = [(dt, D, M) for dt in DTYPES for D in rms_dims(dt, True) for M in (1, 3, 4096 + 5)]


@pytest.mark.parametrize("dtype,D,M", RMS_CASES, ids=[f"{'bf16' if dt == BF16 else 'fp32'}-D{D}-M{M}" for dt, D, M in RMS_CASES])
def test_rmsnorm_forward_backward_every_dispatch_class(ops, dtype, D, M):
    """mh_rmsnorm_fwd (grid min(ceil(M / 4), 65536), a wave per row), mh_row_rstd(x), mh_rmsnorm_bwd (grid
    mh_rmsnorm_bwd_blocks(M) = min(ceil(M / 4), 1024): with M = 4096 + 5 every wave walks a second row and accumulates dw over
    both, at each NCH class) + mh_colsum, mh_rmsnorm_bwd_folded.  Row 1 (M >= 3) is all zeros in x and dy: rstd = rsqrt(eps), y = 0,
    dx = dres exactly.  dres given / None, dw fresh / accumulated.
    Bounds (ref_streamers): rstd -- half the sum's (depth + 2) 2^-24 + one ulp for v_rsq_f32 + the store; y -- (3 E_T bf16 /
    2 E_T fp32 + A_f32 + rstd's) |w xhat| with xhat rounded to T in the reference as in the kernel; dx -- (E_T + A_f32 +
    (depth + 2) 2^-24) (|r g w| + |r xhat| mean|g w xhat| + |dres|); dw -- (dw_depth + 2) 2^-24 sum_m |dy rnd(xhat)| + E_out
    |dw| with the kernel's own rstd as the shared input."""
    fwd = D in rms_dims(dtype, False)
    x, w, dy, dres = R.rms_inputs(M, D, dtype, 13, "cuda")
    z = 1 if M >= 3 else None   # the all-zero row
    if z is not None:
        x[z] = 0
        dy[z] = 0
    if fwd:
        by, y = padded(torch.empty((M, D), dtype=dtype, device="cuda"))
        br, rstd = padded(torch.empty(M, device="cuda"))
        ops.rmsnorm_fwd(x, w, y, rstd, R.RMS_EPS)
        br2, rstd2 = padded(torch.empty(M, device="cuda"))
        ops.row_rstd(rstd2, D, R.RMS_EPS, x=x)
        torch.cuda.synchronize()
        r64, y64, ty = R.rmsnorm_fwd_ref(x, w, dtype)
        assert_bound(rstd, r64, R.rstd_bound(r64, D, dtype), "rstd")
        assert_bound(rstd2, r64, R.rstd_bound(r64, D, dtype), "row_rstd")
        assert_bound(y, y64, R.rmsnorm_fwd_bound(ty, D, dtype), "y")
        assert z is None or bool((y[z] == 0).all())
        assert sentinels_intact(by, 0, M * D) and sentinels_intact(br, 0, M) and sentinels_intact(br2, 0, M)
        if M <= 3:   # second witness
            ey, er = torch.empty_like(y), torch.empty_like(rstd)
            emu.rmsnorm_fwd(x, w, ey, er, R.RMS_EPS)
            assert R.bad(ey, y64, R.rmsnorm_fwd_bound(ty, D, dtype)) == 0 and R.bad(er, r64, R.rstd_bound(r64, D, dtype)) == 0
        del r64, y64, ty
    else:
        rstd = R.rstd_ref(x).to(F32)
    # ---- backward: dres given, fresh dw in the activation dtype; then dres = None accumulating into the same dw
    bx, dx = padded(torch.empty((M, D), dtype=dtype, device="cuda"))
    bw, dw = padded(torch.zeros(D, dtype=dtype, device="cuda"))
    ops.rmsnorm_bwd(x, w, rstd, dy, dres, dx, dw, False)
    torch.cuda.synchronize()
    dx64, tx, dw64, tw = R.rmsnorm_bwd_ref(x, w, rstd, dy, dres, dtype)
    assert_bound(dx, dx64, R.rmsnorm_bwd_bound(tx, D, dtype), "dx")
    assert_bound(dw, dw64, R.dw_bound(dw64, tw, M, dtype), "dw")
    assert z is None or torch.equal(dx[z], dres[z]), "an all-zero row: dx = dres"
    if M <= 3:
        edx, edw = torch.empty_like(dx), torch.zeros_like(dw)
        emu.rmsnorm_bwd(x, w, rstd, dy, dres, edx, edw, False)
        assert R.bad(edx, dx64, R.rmsnorm_bwd_bound(tx, D, dtype)) == 0 and R.bad(edw, dw64, R.dw_bound(dw64, tw, M, dtype)) == 0
    del dx64, tx
    dw1 = dw.clone()
    ops.rmsnorm_bwd(x, w, rstd, dy, None, dx, dw, True)
    torch.cuda.synchronize()
    dx64, tx, _, _ = R.rmsnorm_bwd_ref(x, w, rstd, dy, None, dtype)
    assert_bound(dx, dx64, R.rmsnorm_bwd_bound(tx, D, dtype), "dx (no dres)")
    acc64 = dw64 + dw1.to(F64)
    assert_bound(dw, acc64, R.dw_bound(acc64, tw + dw1.to(F64).abs(), M, dtype), "dw (accumulated)")
    assert sentinels_intact(bx, 0, M * D) and sentinels_intact(bw, 0, D)
    del dx64, tx
    # ---- the folded form (t = dy)
    ops.rmsnorm_bwd_folded(x, rstd, dy, dres, dx)
    torch.cuda.synchronize()
    f64_, tf = R.folded_bwd_ref(x, rstd, dy, dres)
    assert_bound(dx, f64_, R.rmsnorm_bwd_bound(tf, D, dtype), "folded dx")
    ops.rmsnorm_bwd_folded(x, rstd, dy, None, dx)
    torch.cuda.synchronize()
    f64_, tf = R.folded_bwd_ref(x, rstd, dy, None)
    assert_bound(dx, f64_, R.rmsnorm_bwd_bound(tf, D, dtype), "folded dx (no dres)")
    assert sentinels_intact(bx, 0, M * D)


CENSUS_CASES = [(dt, D) for dt in DTYPES for D in rms_dims(dt, True)]


@pytest.mark.parametrize("dtype,D", CENSUS_CASES, ids=[f"{'bf16' if dt == BF16 else 'fp32'}-D{D}" for dt, D in CENSUS_CASES])
def test_rmsnorm_bwd_dw_census(ops, dtype, D):
    """the exact probe of mh_rmsnorm_bwd's dw at M = 4096 + 5 (a second row per wave) for every class: every row of x the same
    row, rstd = 0.75, dy[m, c] = 1 where c == m mod D, an fp32 dw: dw[c] = (rows with m == c mod D) * rnd<T>(0.75 x[c]) with
    every partial sum exact in fp32 -- one dropped or doubled row changes it"""
    M = 4096 + 5
    x, dy, counts = R.census_rows(M, D, dtype, 19, "cuda")
    w = torch.ones(D, dtype=dtype, device="cuda")
    rstd = torch.full((M,), 0.75, device="cuda")
    dx, dw = torch.empty_like(x), torch.full((D,), NAN, device="cuda")
    ops.rmsnorm_bwd(x, w, rstd, dy, None, dx, dw, False)
    torch.cuda.synchronize()
    want = counts * R.rd(x[0].to(F64) * 0.75, dtype)
    assert torch.equal(dw.to(F64), want), int((dw.to(F64) != want).sum())


@pytest.mark.parametrize("dtype", DTYPES)
def test_rmsnorm_bwd_refuses_rows_longer_than_its_lds(ops, dtype):
    """D = 8200 is above the [4][D] fp32 accumulator the backward may ask for: refused by MH_REQUIRE, nothing launched"""
    M, D = 3, 8200
    x, w, dy, _ = R.rms_inputs(M, D, dtype, 13, "cuda")
    with pytest.raises(RuntimeError, match="bad shape"):
        ops.rmsnorm_bwd(x, w, torch.ones(M, device="cuda"), dy, None, torch.empty_like(x), torch.zeros(D, dtype=dtype, device="cuda"), False)


@pytest.mark.parametrize("dtype", DTYPES)
def test_rmsnorm_fwd_second_grid_pass(ops, dtype):
    """mh_rmsnorm_fwd's grid is capped at 65536 blocks of four rows: at M = 262144 + 5 (smallest register-form D = 64 N) the
    last five rows are a wave's second trip.  The kernel is row-local: those rows equal, bit for bit, a launch on the last 64
    rows alone; float64 on the 256 rows around the boundary."""
    D, M = 64 * NVEC[dtype], 262144 + 5
    x = grnd((M, D), dtype, 14, 2.0)
    w = (1 + 0.5 * grnd((D,), F32, 15)).to(dtype)
    by, y = padded(torch.empty((M, D), dtype=dtype, device="cuda"))
    br, rstd = padded(torch.empty(M, device="cuda"))
    ops.rmsnorm_fwd(x, w, y, rstd, R.RMS_EPS)
    lo = M - 64
    y2, r2 = torch.empty((64, D), dtype=dtype, device="cuda"), torch.empty(64, device="cuda")
    ops.rmsnorm_fwd(x[lo:], w, y2, r2, R.RMS_EPS)
    torch.cuda.synchronize()
    assert same_bits(y[lo:], y2) and same_bits(rstd[lo:], r2)
    sl = slice(M - 256, M)
    r64, y64, ty = R.rmsnorm_fwd_ref(x[sl], w, dtype)
    assert_bound(rstd[sl], r64, R.rstd_bound(r64, D, dtype), "rstd, second pass")
    assert_bound(y[sl], y64, R.rmsnorm_fwd_bound(ty, D, dtype), "y, second pass")
    assert sentinels_intact(by, 0, M * D) and sentinels_intact(br, 0, M)


@pytest.mark.parametrize("out_dtype", DTYPES)
def test_colsum_exact_on_integer_partials(call, out_dtype):
    """mh_colsum: nblk <= 32 rows are added by stage B alone; above, stage A folds ceil(nblk / 32) rows per range (grid y =
    ceil(nblk / rows_per)) into the range's first row, 64 columns per block, then stage B (256 columns per block) adds the
    first rows.  nblk in {1, 31, 32, 33, 63, 64, 65, 1024, 1025} x D in {1, 63, 64, 65, 300, 1024}, integer partials (every
    sum exact in fp32), fp32 and bf16 outputs, fresh and accumulated; the partials behind nblk rows are NaN"""
    for nblk in (1, 31, 32, 33, 63, 64, 65, 1024, 1025):
        for D in (1, 63, 64, 65, 300, 1024):
            r, c = torch.arange(nblk, device="cuda")[:, None], torch.arange(D, device="cuda")[None, :]
            part = (((r * 3 + c * 5) % 7) - 3).float()
            want = part.to(F64).sum(0)
            for acc in (0, 1):
                _, pv = padded(part)
                old = ((torch.arange(D, device="cuda") % 5) - 2).to(out_dtype)
                bo, out = padded(old)
                call("mh_colsum", pv.data_ptr(), nblk, out.data_ptr(), D, acc, MH(out_dtype), stream())
                torch.cuda.synchronize()
                exp = (want + (old.to(F64) if acc else 0)).to(F32).to(out_dtype)
                assert torch.equal(out, exp), (nblk, D, acc)
                assert sentinels_intact(bo, 0, D)


def test_row_rstd_from_parts(ops):
    """mh_row_rstd(parts): 64 rows per workgroup, the D / 64 parts of a row spread over four waves and folded through LDS.
    D in {64, 1024} (one part: three waves idle; sixteen), M in {1, 63, 65} (a partial workgroup, a second one).  A part
    count that is not D / 64 is refused."""
    for D in (64, 1024):
        for M in (1, 63, 65):
            parts = grnd((D // 64, M), F32, 21).abs() * 64
            br, rstd = padded(torch.empty(M, device="cuda"))
            ops.row_rstd(rstd, D, R.RMS_EPS, parts=parts)
            torch.cuda.synchronize()
            r64 = torch.rsqrt(parts.to(F64).sum(0) / D + R.RMS_EPS)
            assert_bound(rstd, r64, R.rstd_bound(r64, D, F32), f"row_rstd(parts) D={D} M={M}")
            assert sentinels_intact(br, 0, M)
    with pytest.raises(RuntimeError, match="nparts"):
        ops.row_rstd(torch.empty(4, device="cuda"), 128, R.RMS_EPS, parts=torch.ones((3, 4), device="cuda"))


# ----------------------------------------------------------------------------------------------------------------- RoPE
@pytest.mark.parametrize("dtype", DTYPES)
def test_rope_head_dims_directions_and_round_trip(ops, dtype):
    """mh_rope: items = M * 2 * H * (hd / 2 / N), an item rotates N pairs (i, i + hd / 2) of one head of q or k.  hd in {16, 32,
    64, 256} (hd = 16: one fp32 item per half head; bf16 needs hd / 2 >= 8) x H in {1, 3}, M = 7 rows of sequences of S = 5
    (M no multiple of S), pos0 = 3, both directions.  Bound: (E_T + A_f32) (|x1 c| + |x2 s|), cos / sin rounded to T in the
    reference as in the kernel.  The V third keeps its bits.  dir = -1 after dir = +1: against the float64 composition of
    the two rotations (which restores (c^2 + s^2) x: the rounded tables are not exactly unit length), within the backward
    bound plus the forward bounds of the pair carried through."""
    M, S, pos0 = 7, 5, 3
    for hd in (16, 32, 64, 256):
        for H in (1, 3):
            cos_t, sin_t = R.rope_tables(hd, pos0 + S, "cuda")
            qkv = grnd((M, 3 * H * hd), dtype, 17)
            D = H * hd
            for direction in (1, -1):
                bq, out = padded(qkv.clone())
                ops.rope_(out, cos_t, sin_t, S, pos0, H, hd, direction)
                torch.cuda.synchronize()
                o64, t = R.rope_ref(qkv, cos_t, sin_t, S, pos0, H, hd, direction, dtype)
                assert_bound(out[:, :2 * D], o64[:, :2 * D], R.rope_bound(t[:, :2 * D], dtype), f"rope hd={hd} H={H} dir={direction}")
                assert same_bits(out[:, 2 * D:], qkv[:, 2 * D:]) and sentinels_intact(bq, 0, qkv.numel())
                e = emu.rope_(qkv.clone().cpu(), cos_t.cpu(), sin_t.cpu(), S, pos0, H, hd, direction).cuda()
                assert R.bad(e[:, :2 * D], o64[:, :2 * D], R.rope_bound(t[:, :2 * D], dtype)) == 0
                if direction == 1:
                    fwd, fwd64, bf = out.clone(), o64, R.rope_bound(t, dtype)
            ops.rope_(fwd, cos_t, sin_t, S, pos0, H, hd, -1)
            torch.cuda.synchronize()
            b64, tb = R.rope_ref(fwd64, cos_t, sin_t, S, pos0, H, hd, -1, dtype)
            v = bf[:, :2 * D].reshape(M, 2 * H, 2, hd // 2)
            carried = (v + v.flip(2)).reshape(M, 2 * D)    # |c| e1 + |s| e2 <= e1 + e2 for the pair
            assert_bound(fwd[:, :2 * D], b64[:, :2 * D], R.rope_bound(tb[:, :2 * D], dtype) + carried, f"rope round trip hd={hd} H={H}")
            assert same_bits(fwd[:, 2 * D:], qkv[:, 2 * D:])
    with pytest.raises(RuntimeError, match="bad shape"):
        ops.rope_(grnd((2, 3 * 8), dtype, 18), cos_t, sin_t, 2, 0, 1, 8, 1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_rope_second_grid_pass(ops, dtype):
    """grid = min(ceil(items / 256), 16384); H = 16, hd = 64: 2 * 16 * (32 / N) items per row, so rows from 16384 * 256 /
    per_row = 32768 (bf16) / 16384 (fp32) on belong to a second grid-stride trip.  M = that + 3, S = M (the position is the
    row).  The rows from 64 before the boundary on equal, bit for bit, a launch on those rows alone with pos0 moved; float64
    on the same rows."""
    H, hd = 16, 64
    per_row = 2 * H * (hd // 2 // NVEC[dtype])
    M = 16384 * 256 // per_row + 3
    cos_t, sin_t = R.rope_tables(hd, M, "cuda")
    qkv = grnd((M, 3 * H * hd), dtype, 19)
    lo = M - 3 - 64
    part = qkv[lo:].clone()
    bq, out = padded(qkv.clone())
    ops.rope_(out, cos_t, sin_t, M, 0, H, hd, 1)
    ops.rope_(part, cos_t, sin_t, M, lo, H, hd, 1)
    torch.cuda.synchronize()
    assert same_bits(out[lo:], part) and sentinels_intact(bq, 0, qkv.numel())
    o64, t = R.rope_ref(qkv[lo:], cos_t, sin_t, M, lo, H, hd, 1, dtype)
    assert_bound(part[:, :2 * H * hd], o64[:, :2 * H * hd], R.rope_bound(t[:, :2 * H * hd], dtype), "rope second pass")
    assert same_bits(out[:, 2 * H * hd:], qkv[:, 2 * H * hd:])
    o64, t = R.rope_ref(qkv[:64], cos_t, sin_t, M, 0, H, hd, 1, dtype)
    assert_bound(out[:64, :2 * H * hd], o64[:, :2 * H * hd], R.rope_bound(t[:, :2 * H * hd], dtype), "rope first rows")


# ---------------------------------------------------------------------------------------------------------- cast, copy
def _ties(n, device="cuda"):
    """fp32 values exactly half way between two neighbouring bf16 values, both parities of the lower one's last bit"""
    g = torch.Generator(device=device).manual_seed(23)
    lo_bits = torch.randint(0x3c00, 0x4200, (n,), generator=g, device=device, dtype=torch.int32)
    lo_v = (lo_bits << 16).view(F32)
    hi_v = ((lo_bits + 1) << 16).view(F32)
    src = (lo_v + hi_v) / 2
    even = torch.where(lo_bits % 2 == 0, lo_v, hi_v)
    neg = torch.arange(n, device=device) % 4 == 2
    return torch.where(neg, -src, src), torch.where(neg, -even, even)


@pytest.mark.parametrize("dtype", DTYPES)
def test_cast_from_f32_bit_for_bit(ops, dtype):
    """mh_cast_from_f32: grid min(ceil(n / 256), 4096), one element per lane and trip.  n in {1, 255, 257} (a partial block, a
    second block) and 4096 * 256 + 3 (second grid-stride trip).  Bit for bit: random values, exact bf16 ties of both parities
    (round to even), and accumulate = 1 (one fp32 add, then the rounding)."""
    for n in (1, 255, 257, 4096 * 256 + 3):
        src, even = _ties(n)
        src[1::2] = grnd((n,), F32, 22)[1::2]
        bd, dst = padded(torch.zeros(n, dtype=dtype, device="cuda"))
        ops.cast_from_f32(src, dst, False)
        torch.cuda.synchronize()
        assert same_bits(dst, src.to(dtype)) and sentinels_intact(bd, 0, n)
        if dtype == BF16:
            assert torch.equal(dst[0::2].float(), even[0::2]), "ties go to the even neighbour"
        old = grnd((n,), dtype, 24)
        bd, dst = padded(old)
        ops.cast_from_f32(src, dst, True)
        torch.cuda.synchronize()
        assert same_bits(dst, (src + old.float()).to(dtype)) and sentinels_intact(bd, 0, n)


@pytest.mark.parametrize("dtype", DTYPES)
def test_copy_rows_strided_bit_for_bit(ops, dtype):
    """mh_copy_rows: grid min(ceil(M / 4), 65536), a wave per row, 16-byte chunks.  D in {8, 8 * 63, 1024} x M in {1, 5} and
    (M, D) = (262144 + 3, 8) (second grid-stride trip), source and destination rows inside wider rows (ld = D + 16, the row at
    column 8): the 8-element gaps on both sides of every destination row keep their NaN.  accumulate: the fp32 sum rounded
    once, which equals the float64 sum rounded through fp32 -- bit for bit."""
    for M, D in ((1, 8), (5, 8), (1, 504), (5, 504), (1, 1024), (5, 1024), (262144 + 3, 8)):
        ld = D + 16
        src_w = grnd((M, ld), dtype, 25)
        for acc in (False, True):
            dst_w = torch.full((M, ld), NAN, dtype=dtype, device="cuda")
            old = grnd((M, D), dtype, 26)
            if acc:
                dst_w[:, 8:8 + D] = old
            ops.copy_rows(src_w.view(-1)[8:], ld, dst_w.view(-1)[8:], ld, M, D, acc)
            torch.cuda.synchronize()
            want = src_w[:, 8:8 + D]
            if acc:
                want = R.rd(want.to(F64) + old.to(F64), dtype).to(dtype)
            assert same_bits(dst_w[:, 8:8 + D], want), (M, D, acc)
            assert bool(torch.isnan(dst_w[:, :8]).all()) and bool(torch.isnan(dst_w[:, 8 + D:]).all())


# -------------------------------------------------------------------------------------------------------- masked softmax
@pytest.mark.parametrize("dtype", DTYPES)
def test_masked_softmax_rows_widths_and_temperatures(ops, dtype):
    """mh_masked_softmax: grid ceil(B / 4), a wave per row, columns lane + 64 k.  B in {1, 3, 5} (a partial block, a second
    block) x V in {40, 64, 65, 3406} (less than a wave, exactly one pass, one column into the second) x temp in {0.5, 1, 1.3};
    row kinds by b % 3: first-mask row, range row, empty range (all zeros); row 0's logits reach +-80 before the temperature.
    Against float64 on rnd<T>(logit / temp) under ref_streamers.softmax_bound; exact zeros outside the mask."""
    for B in (1, 3, 5):
        for V in (40, 64, 65, 3406):
            logits, lo, hi, fm = R.softmax_inputs(B, V, dtype, 36, "cuda")
            for temp in (0.5, 1.0, 1.3):
                bp, probs = padded(torch.empty((B, V), device="cuda"))
                ops.masked_softmax(logits, lo, hi, fm, probs, V, temp)
                torch.cuda.synchronize()
                p64, zm = R.softmax_ref(logits, lo, hi, fm, V, temp, dtype)
                assert_bound(probs, p64, R.softmax_bound(p64, zm, V), f"masked softmax B={B} V={V} temp={temp}")
                assert bool((probs[p64 == 0] == 0).all()) and sentinels_intact(bp, 0, B * V)
                if B >= 3:
                    assert bool((probs[2] == 0).all())
                e = emu.masked_softmax(logits.cpu(), lo.cpu(), hi.cpu(), fm.cpu(), torch.empty((B, V)), V, temp).cuda()
                assert R.bad(e, p64, R.softmax_bound(p64, zm, V)) == 0


# --------------------------------------------------------------------------------------------------------------- sampler
def _sampler_launch(ops, case):
    c = case
    buf = torch.full((c["B"] + 2,), -7, dtype=torch.int64, device="cuda")
    ops.sample_top_p_k(c["logits"].cuda(), c["fm"].cuda(), c["lo_tab"].cuda(), c["hi_tab"].cuda(), c["ev"].cuda(), 1, c["q"].cuda(),
                       buf[1:1 + c["B"]], c["V"], c["temp"], c["top_p"], c["top_k"], first_span=(0, 0), max_range=c["max_range"],
                       ban_mask=c["ban"].cuda())
    torch.cuda.synchronize()
    assert buf[0].item() == -7 and buf[-1].item() == -7
    return buf[1:1 + c["B"]].cpu()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("top_k", [1, 20, 64])
@pytest.mark.parametrize("tmax", [2, 8, 32])
def test_sampler_instantiation_boundaries(ops, dtype, top_k, tmax):
    """mh_sample_top_p_k picks its instantiation by the longest range of the position: span <= 128 -> 2 candidates per lane on
    one wave, <= 512 -> 8 over four waves (ranked by counting), else 32 (top_k arg-max rounds).  One launch per instantiation
    with synthetic range tables (ref_streamers.sampler_case): rows of {1, 2, 63, 64, 65, 127, 128} / {129, 191, 192, 193, 256,
    257, 511, 512} / {513, 1023, 1024, 1025, 2047, 2048} ids at `lo` that are no multiple of 64, the last range clipped at V,
    rows with fewer candidates than top_k, a ban mask that leaves one candidate, rows peaked at the lowest / highest id of
    their range (every other probability is 0: ties at zero).  Ids equal emu_ops.sample_top_p_k's on the same Exp(1) noise,
    except on rows the emulation itself marks as decided by fp32 summation order (the host test caps those at 2 %)."""
    case = R.sampler_case(tmax, dtype, 100 + tmax, top_k=top_k)
    got = _sampler_launch(ops, case)
    want = R.sampler_emulate(case, emu)
    decided = ~R.sampler_undecided(case, emu)
    assert torch.equal(got[decided], want[decided]), (got.tolist(), want.tolist())
    lo, hi = case["lo_tab"][:, 1], case["hi_tab"][:, 1].clamp(max=case["V"])
    assert bool(((got >= lo) & (got < hi)).all()), "an id outside the row's range"
    assert got[0].item() == int(lo[0]) and got[1].item() == int(hi[1]) - 1, "the peaked rows"
    assert got[2].item() == int(lo[2]) + R.SAMPLER_LENGTHS[tmax][2] // 2, "the one id the ban mask leaves"


@pytest.mark.parametrize("dtype", DTYPES)
def test_sampler_vocabulary_past_one_batch(ops, dtype):
    """the softmax statistics run over the whole vocabulary in batches of 14 x 256 = 3584 ids: V = 3600 takes a second batch
    (the online maximum / sum rescale between batches)"""
    case = R.sampler_case(8, dtype, 131, V=3600)
    got = _sampler_launch(ops, case)
    want = R.sampler_emulate(case, emu)
    decided = ~R.sampler_undecided(case, emu)
    assert torch.equal(got[decided], want[decided]), (got.tolist(), want.tolist())
