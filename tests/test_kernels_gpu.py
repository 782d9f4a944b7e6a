"""Per-kernel parity on the MI355X: every C-ABI entry point (through midi_model_amd.ops -> libmidihip.so)
against the CPU restatement of the same op (tests/emu_ops.py) on identical seeded inputs, in fp32
(verification mode, tight tolerance) and bf16 (production mode, inputs pre-rounded to bf16 so the check
measures the kernel and not the input rounding).  Shapes cover ragged / non-multiple-of-tile sizes, single
rows, padding and ignore-index edge cases."""
import contextlib
import math

import numpy as np
import pytest
import torch

import emu_ops as emu

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]


def tol(dtype, k=1.0):
    return (dict(rtol=2e-4 * k, atol=2e-5 * k) if dtype == torch.float32 else dict(rtol=2e-2 * k, atol=2e-2 * k))


@pytest.fixture(scope="module")
def ops():
    import midi_model_amd.ops as real
    return real


@pytest.fixture(params=[0, 1, 2], ids=["gemm128", "gemmpp256", "gemmpp256k32"])
def gemm_variant(request, ops):
    """run the GEMM tests against the projection kernels: gemm.hip, gemm_pp256.hip as shipped (K-step-64 main loop for two
    row-major operands, K-step-32 ping-pong loop otherwise), gemm_pp256.hip with the K-step-32 loop everywhere"""
    with (ops.ab_library() if request.param == 0 else contextlib.nullcontext()):  # the 128x128 bf16 kernel: A/B library only
        ops.set_option("gemm", min(request.param, 1))
        ops.set_option("gemm_k64", 0 if request.param == 2 else 1)
        yield request.param
        ops.set_option("gemm", 1)
        ops.set_option("gemm_k64", 1)


def test_production_library_refuses_the_ab_only_forms(ops):
    """the first-form attention kernels, the 128x128 bf16 GEMM and the wrong-by-design ablation builds are not in
    libmidihip.so: selecting one is an error at the call, not a silent substitution"""
    from midi_model_amd.lib import lib
    assert lib().cdll.mh_ab_builds() == 0
    a, b = torch.ones((64, 64), dtype=torch.bfloat16, device="cuda"), torch.ones((64, 64), dtype=torch.bfloat16, device="cuda")
    c = torch.empty((64, 64), dtype=torch.bfloat16, device="cuda")
    try:
        ops.set_option("gemm", 0)
        with pytest.raises(RuntimeError, match="A/B test library"):
            ops.gemm_nt(a, b, c)
        ops.set_option("gemm", 1)
        ops.set_option("gemm_ablate", 4)
        with pytest.raises(RuntimeError, match="A/B test"):
            ops.gemm_nt(a, b, c)
        ops.set_option("gemm_ablate", 0)
        ops.gemm_nt(a, b, c)
        assert (c.float() == 64).all()
        ops.set_option("attn_v3", 0)
        qkv = torch.zeros((64, 192), dtype=torch.bfloat16, device="cuda")
        o, lse = torch.empty((64, 64), dtype=torch.bfloat16, device="cuda"), torch.zeros(64, device="cuda")
        with pytest.raises(RuntimeError, match="A/B test"):
            ops.attn_fwd(qkv, o, lse, 1, 64, 1, 0.125)
        with pytest.raises(RuntimeError, match="A/B"):
            ops.attn_bwd(qkv, o, o, lse, torch.empty_like(qkv), 1, 64, 1, 0.125)
    finally:
        ops.set_option("gemm", 1)
        ops.set_option("gemm_ablate", 0)
        ops.set_option("attn_v3", V3_DEFAULT)


def rnd(shape, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(shape, generator=g)).to(dtype)


def cmp(got, want, dtype, k=1.0, what=""):
    got, want = got.detach().float().cpu(), want.detach().float().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    t = tol(dtype, k)
    err = (got - want).abs()
    bad = err > (t["atol"] + t["rtol"] * want.abs())
    assert not bad.any(), (f"{what}: {int(bad.sum())}/{bad.numel()} off, max abs err {err.max().item():.3e} "
                           f"(ref max {want.abs().max().item():.3e}), first bad idx {bad.nonzero()[0].tolist()}")


# ------------------------------------------------------------------------------------------------ GEMM
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (256, 384, 256), (257, 200, 96), (1, 1024, 1024), (1000, 72, 8),
                                   (64, 3406, 256), (640, 1024, 4096)])
def test_gemm_nt(ops, gemm_variant, dtype, M, N, K):
    """workload shapes against the fp32 emulation.  The bf16 tolerance (2e-2 K / 256, absolute and relative) is wide enough for
    a dropped K-step or a bf16 intermediate to pass, and the fp32 mode runs the 128x128 kernel, not the production one: the
    bit-exact checks at the tile, K-loop and split-K edges are in test_gemm_gpu.py"""
    a, b = rnd((M, K), dtype, 1), rnd((N, K), dtype, 2)
    want = emu.gemm_nt(a, b, torch.empty((M, N), dtype=dtype))
    out = torch.full((M, N), float("nan"), dtype=dtype, device="cuda")
    ops.gemm_nt(a.cuda(), b.cuda(), out)
    # fp32 accumulation-order noise grows like sqrt(K) * |a||b|; outputs have std sqrt(K)
    cmp(out, want, dtype, k=max(1.0, K / 256), what=f"gemm {M}x{N}x{K}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ta,tb", [(False, True), (True, False), (True, True)])
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (200, 136, 100), (1024, 256, 2051), (72, 1000, 333)])
def test_gemm_contraction_major_operands(ops, gemm_variant, dtype, ta, tb, M, N, K):
    """dgrad / wgrad operand forms: A stored [K,M] and/or B stored [K,N] (bf16: LDS transpose reads, any K;
    fp32: re-layout fallback).  Row lengths M, N are multiples of 8 as every model dimension is."""
    Kn = (K + 7) // 8 * 8  # a non-transposed operand must be readable/zero up to the next multiple of 8
    a = rnd((K, M), dtype, 41) if ta else torch.cat([rnd((M, K), dtype, 41), torch.zeros((M, Kn - K), dtype=dtype)], 1)
    b = rnd((K, N), dtype, 42) if tb else torch.cat([rnd((N, K), dtype, 42), torch.zeros((N, Kn - K), dtype=dtype)], 1)
    want = emu.gemm_nt(a, b, torch.empty((M, N), dtype=dtype), K=K, ta=ta, tb=tb)
    for sk in (1, 3):
        out = torch.full((M, N), float("nan"), dtype=dtype, device="cuda")
        ops.gemm_nt(a.cuda(), b.cuda(), out, K=K, ta=ta, tb=tb, splitk=sk)
        cmp(out, want, dtype, k=max(1.0, K / 256), what=f"gemm ta={ta} tb={tb} {M}x{N}x{K} splitk={sk}")


@pytest.fixture(params=[1, 2, 4], ids=["mb1", "mb2", "mb4"])
def skinny_mb(request, ops):
    """the three row tilings of mh_gemm_skinny (16-row activation blocks per workgroup)"""
    ops.set_option("skinny_mb", request.param)
    yield request.param
    ops.set_option("skinny_mb", 0)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("M,N,K", [(64, 3072, 1024), (1, 1024, 1024), (5, 3406, 1024), (64, 1024, 4096), (33, 2048, 256),
                                   (64, 4096, 1024), (16, 1024, 1024), (17, 1024, 1024), (48, 3072, 1024)])
def test_gemm_skinny(ops, skinny_mb, mode, M, N, K):
    """decode-step projection (mh_gemm_skinny, bf16 only): plain + residual into a narrowed output view (logits layout),
    and the fused gate|up -> SwiGLU epilogue against gemm -> swiglu_fwd on the CPU"""
    dtype = torch.bfloat16
    a = rnd((M, K), dtype, 11)
    w = rnd((2 * N if mode == 1 else N, K), dtype, 12, 0.05)
    r = None if mode == 1 else rnd((M, N), dtype, 13)
    want = emu.gemm_skinny(a, w, torch.empty((M, N), dtype=dtype), mode=mode, res=r)
    buf = torch.zeros((M, N + 24), dtype=dtype, device="cuda")
    ops.gemm_skinny(a.cuda(), w.cuda(), buf[:, :N], mode=mode, res=None if r is None else r.cuda())
    cmp(buf[:, :N], want, dtype, k=max(1.0, K / 512), what=f"gemm_skinny mode={mode} {M}x{N}x{K}")
    assert (buf[:, N:] == 0).all()
    # row scaling by rsqrt(mean(a^2) + eps): RMSNorm with its weight folded into w
    want = emu.gemm_skinny(a, w, torch.empty((M, N), dtype=dtype), mode=mode, res=r, norm_eps=1e-6)
    out = torch.empty((M, N), dtype=dtype, device="cuda")
    ops.gemm_skinny(a.cuda(), w.cuda(), out, mode=mode, res=None if r is None else r.cuda(), norm_eps=1e-6)
    cmp(out, want, dtype, k=max(1.0, K / 512), what=f"gemm_skinny rstd mode={mode} {M}x{N}x{K}")
    # embedding lookup folded in: rows of A (and of the residual) picked from tables by id
    g = torch.Generator().manual_seed(3)
    table, rtable = rnd((50, K), dtype, 15), (None if mode == 1 else rnd((50, N), dtype, 16))
    ids = torch.randint(0, 50, (M,), generator=g)
    want = emu.gemm_skinny(table, w, torch.empty((M, N), dtype=dtype), mode=mode, res=rtable, norm_eps=1e-6, row_ids=ids, res_ids=ids)
    ops.gemm_skinny(table.cuda(), w.cuda(), out, mode=mode, res=None if rtable is None else rtable.cuda(), norm_eps=1e-6,
                    row_ids=ids.cuda(), res_ids=None if rtable is None else ids.cuda())
    cmp(out, want, dtype, k=max(1.0, K / 512), what=f"gemm_skinny gathered rows mode={mode} {M}x{N}x{K}")
    with pytest.raises(RuntimeError):
        ops.gemm_skinny(torch.zeros((65, K), dtype=dtype, device="cuda"), w.cuda(), torch.zeros((65, N), dtype=dtype, device="cuda"), mode=mode)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_epilogue_views_splitk(ops, gemm_variant, dtype):
    M, N, K = 300, 520, 2048 + 64
    a, b, r = rnd((M, K), dtype, 3), rnd((N, K), dtype, 4), rnd((M, N), dtype, 5)
    # residual epilogue into a separate buffer
    want = emu.gemm_nt(a, b, torch.empty((M, N), dtype=dtype), beta=1.0, res=r, alpha=0.5)
    out = torch.empty((M, N), dtype=dtype, device="cuda")
    ops.gemm_nt(a.cuda(), b.cuda(), out, beta=1.0, res=r.cuda(), alpha=0.5)
    cmp(out, want, dtype, k=4, what="gemm residual")
    # accumulate in place + forced split-K
    acc = r.clone().cuda()
    ops.gemm_nt(a.cuda(), b.cuda(), acc, beta=1.0, splitk=5)
    cmp(acc, emu.gemm_nt(a, b, r.clone(), beta=1.0), dtype, k=4, what="gemm split-K accumulate")
    # output is a narrowed view of a padded buffer (the logits layout), K limited by the argument
    buf = torch.zeros((M, 576), dtype=dtype, device="cuda")
    ops.gemm_nt(a.cuda(), b.cuda(), buf[:, :N], K=1024)
    cmp(buf[:, :N], emu.gemm_nt(a, b, torch.empty((M, N), dtype=dtype), K=1024), dtype, k=3, what="gemm view")
    assert (buf[:, N:] == 0).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("R,C", [(64, 64), (100, 37), (1000, 1024), (8, 3406)])
def test_transpose(ops, dtype, R, C):
    x = rnd((R, C), dtype, 6)
    out = ops.transpose(x.cuda())
    assert out.shape == (C, (R + 7) // 8 * 8)
    assert torch.equal(out[:, :R].cpu(), x.T) and (out[:, R:] == 0).all()


@pytest.fixture(params=[0, 1], ids=["k32", "k64"])
def main_loop(request, ops):
    """the two main loops of gemm_pp256_kernel behind the fused-epilogue entry points"""
    ops.set_option("gemm_k64", request.param)
    yield request.param
    ops.set_option("gemm_k64", 1)


def test_gemm_main_loops_agree_bit_for_bit(ops):
    """both main loops add the same 32-deep MFMA products in the same order: identical bits, ragged shapes included
    (row-major x row-major and the dgrad form with B stored [K, N])"""
    dt = torch.bfloat16
    for (M, N, K, tb) in [(512, 512, 1024, False), (300, 520, 2048 + 72, False), (1000, 3406, 1024, False), (256, 256, 64, False),
                          (257, 264, 8, False), (512, 512, 1024, True), (300, 520, 2048 + 72, True), (1000, 1024, 3406, True),
                          (257, 264, 40, True), (640, 4096, 1024, True)]:
        a = rnd((M, K), dt, 81).cuda()
        if K % 8:
            a = torch.cat([a, torch.zeros((M, 8 - K % 8), dtype=dt, device="cuda")], 1)
        b = (rnd((K, N), dt, 82) if tb else rnd((N, K), dt, 82)).cuda()
        outs = []
        for v in (0, 1):
            ops.set_option("gemm_k64", v)
            o = torch.full((M, N), float("nan"), dtype=dt, device="cuda")
            ops.gemm_nt(a, b, o, K=K, tb=tb, splitk=1)
            outs.append(o)
        ops.set_option("gemm_k64", 1)
        for o in outs[1:]:
            assert torch.equal(outs[0], o), (M, N, K, (outs[0].float() - o.float()).abs().max().item())


@pytest.mark.parametrize("M,I,K", [(256, 128, 64), (300, 640, 1024), (1000, 4096, 1024), (77, 1024, 264)])
def test_gemm_swiglu(ops, main_loop, M, I, K):
    """gate|up projection with the SwiGLU forward as its epilogue == mh_gemm_nt followed by mh_swiglu_fwd (both sides share
    the main loop and the tile order: a fault there cancels, and only the loose comparison with the emulation remains; the
    product itself is held to an exact reference in test_gemm_gpu.py)"""
    dt = torch.bfloat16
    x, w = rnd((M, K), dt, 64, 0.5), rnd((2 * I, K), dt, 65, 0.5)
    assert ops.swiglu_fused_ok(x.cuda(), I)
    gu = torch.full((M, 2 * I), 7.0, dtype=dt, device="cuda")
    a = torch.full((M, I), 7.0, dtype=dt, device="cuda")
    ops.gemm_swiglu(x.cuda(), w.cuda(), gu, a)
    gu2 = torch.empty((M, 2 * I), dtype=dt, device="cuda")
    ops.gemm_nt(x.cuda(), w.cuda(), gu2, splitk=1)  # (same accumulation order as the unsplit fused launch)
    a2 = torch.empty((M, I), dtype=dt, device="cuda")
    ops.swiglu_fwd(gu2, a2)
    assert torch.equal(gu, gu2), "gate|up differs from the plain projection"
    assert torch.equal(a, a2), "activation differs from mh_swiglu_fwd on the same gate|up"
    gr, ar = torch.empty((M, 2 * I), dtype=dt), torch.empty((M, I), dtype=dt)
    emu.gemm_swiglu(x, w, gr, ar)
    cmp(gu, gr, dt, k=max(1.0, K / 256), what="gemm_swiglu gate|up vs emulation")
    cmp(a, ar, dt, k=max(2.0, K / 128), what="gemm_swiglu activation vs emulation")


@pytest.mark.parametrize("B,S,H,K", [(1, 256, 4, 64), (2, 150, 2, 256), (3, 100, 16, 1024), (1, 77, 1, 264), (2, 2048, 16, 1024)])
def test_gemm_rope(ops, main_loop, B, S, H, K):
    """q|k|v projection with the rotary embedding as its epilogue == mh_gemm followed by mh_rope (bit for bit; both sides
    share the main loop), and the emulation ON THE KERNEL'S OWN PRODUCT within the bf16 tolerance; pos0 = 0 and S <= M only
    (pos0 > 0, S = 1, S > M and the product against an exact reference: test_gemm_gpu.py)"""
    from midi_model_amd.engine import RopeTable
    dt = torch.bfloat16
    M, D = B * S, H * 64
    x, w = rnd((M, K), dt, 71, 0.5), rnd((3 * D, K), dt, 72, 0.5)
    tab = RopeTable(64, 10000.0, "cuda", S)
    assert ops.rope_fused_ok(x.cuda(), 64)
    fused = torch.full((M, 3 * D), 7.0, dtype=dt, device="cuda")
    ops.gemm_rope(x.cuda(), w.cuda(), fused, tab.fused(), S, 0, 64)
    two = torch.empty((M, 3 * D), dtype=dt, device="cuda")
    ops.gemm_nt(x.cuda(), w.cuda(), two, splitk=1)
    plain = two.clone()
    ops.rope_(two, tab.cos, tab.sin, S, 0, H, 64, +1)
    assert torch.equal(fused[:, 2 * D:], plain[:, 2 * D:]), "v differs from the plain projection"
    assert torch.equal(fused, two), f"fused differs from mh_gemm + mh_rope: {(fused.float() - two.float()).abs().max().item()}"
    ref = emu.rope_(plain.cpu().clone(), tab.cos.cpu(), tab.sin.cpu(), S, 0, H, 64, +1)
    cmp(fused, ref, dt, what="gemm_rope vs emulation")

@pytest.mark.parametrize("M,N,K,res", [(512, 1024, 1024, True), (1000, 256, 4096, True), (260, 1024, 512, False)])
def test_gemm_rowss(ops, M, N, K, res):
    """mh_gemm_rowss (the producer side of the folded RMSNorm): C is bit-identical to mh_gemm_nt's, and rowss[n / 64, m] is the
    sum of squares of the STORED bf16 chunk C[m, 64 (n/64) .. + 64) (fp32 accumulation: rtol 1e-5 against torch's)."""
    a, b = rnd((M, K), torch.bfloat16, 1), rnd((N, K), torch.bfloat16, 2, 0.05)
    r = rnd((M, N), torch.bfloat16, 3) if res else None
    want = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
    ops.gemm_nt(a.cuda(), b.cuda(), want, beta=1.0 if res else 0.0, res=r.cuda() if res else None, splitk=1)  # (the same single-slice sum)
    got = torch.empty_like(want)
    parts = torch.full((N // 64, M), float("nan"), device="cuda")
    ops.gemm_rowss(a.cuda(), b.cuda(), got, parts, res=r.cuda() if res else None)
    assert torch.equal(got, want)
    ss = want.float().pow(2).view(M, N // 64, 64).sum(-1).t()
    assert torch.isfinite(parts).all()
    torch.testing.assert_close(parts, ss, rtol=2e-5, atol=1e-6)
    rs = torch.empty((M,), device="cuda")
    ops.row_rstd(rs, N, 1e-6, parts=parts)
    torch.testing.assert_close(rs, torch.rsqrt(want.float().pow(2).mean(-1) + 1e-6), rtol=2e-5, atol=0)
    rs2 = torch.empty((M,), device="cuda")
    ops.row_rstd(rs2, N, 1e-6, x=want)
    torch.testing.assert_close(rs2, rs, rtol=2e-5, atol=0)


@pytest.mark.parametrize("M", [512, 1028])
def test_gemm_scaled_epilogues(ops, M):
    """mh_gemm_rope_scaled / mh_gemm_swiglu_scaled (the consumer side): every row of the fp32 product is multiplied by rowscale[m]
    BEFORE the epilogue rounds and rotates / applies SwiGLU -- against the same arithmetic spelled out in torch (fp32 product of
    the bf16 operands, scale, round, then mh_rope / mh_swiglu_fwd, which the unscaled fused epilogues equal bit for bit).  A bf16
    rounding of the scaled product can differ from the kernel's by one step where fp32 summation order moves a value across a
    rounding boundary: compared within two bf16 ulps of the value's magnitude, and exactly on > 99 % of the elements."""
    import midi_model_amd as mm
    from midi_model_amd.engine import RopeTable
    K, H, hd, I, S = 1024, 4, 64, 1024, 128
    x = rnd((M, K), torch.bfloat16, 11).cuda()
    sc = (0.5 + torch.rand((M,), generator=torch.Generator().manual_seed(5))).cuda()
    # q|k|v + RoPE
    wq = rnd((3 * H * hd, K), torch.bfloat16, 12, 0.05).cuda()
    rope = RopeTable(hd, 10000.0, torch.device("cuda"), S)
    got = torch.empty((M, 3 * H * hd), dtype=torch.bfloat16, device="cuda")
    ops.gemm_rope(x, wq, got, rope.fused(), S, 0, hd, rowscale=sc)
    want = (sc[:, None] * (x.float() @ wq.float().t())).to(torch.bfloat16)
    ops.rope_(want, rope.cos, rope.sin, S, 0, H, hd, +1)
    tol = 2.0 ** -7 * want.float().abs() + 2.0 ** -8 * want.float().abs().amax(-1, keepdim=True)
    assert ((got.float() - want.float()).abs() <= tol).all() and (got == want).float().mean() > 0.99
    # gate|up + SwiGLU, forward-only form (gate|up not written)
    wg = rnd((2 * I, K), torch.bfloat16, 13, 0.05).cuda()
    act = torch.empty((M, I), dtype=torch.bfloat16, device="cuda")
    ops.gemm_swiglu(x, wg, None, act, rowscale=sc)
    gu = (sc[:, None] * (x.float() @ wg.float().t())).to(torch.bfloat16)
    want = torch.empty_like(act)
    ops.swiglu_fwd(gu, want)
    tol = 2.0 ** -6 * want.float().abs() + 2.0 ** -8 * want.float().abs().amax(-1, keepdim=True)
    assert ((act.float() - want.float()).abs() <= tol).all() and (act == want).float().mean() > 0.98
    # rowscale = 1: the scaled forms ARE the unscaled ones
    one = torch.ones((M,), device="cuda")
    a1, a0 = torch.empty_like(act), torch.empty_like(act)
    ops.gemm_swiglu(x, wg, None, a1, rowscale=one)
    ops.gemm_swiglu(x, wg, None, a0)
    assert torch.equal(a1, a0)



@pytest.mark.parametrize("M,I,K", [(256, 256, 64), (300, 520, 1024), (1000, 4096, 1024), (77, 1024, 264)])
def test_gemm_dswiglu(ops, main_loop, M, I, K):
    """down_proj dgrad with the SwiGLU backward as its epilogue == mh_gemm followed by mh_swiglu_bwd"""
    dt = torch.bfloat16
    dx, wd, gu = rnd((M, K), dt, 61, 0.5), rnd((K, I), dt, 62, 0.5), rnd((M, 2 * I), dt, 63, 2.0)
    assert ops.dswiglu_ok(dx.cuda(), I)
    fused = torch.full((M, 2 * I), 7.0, dtype=dt, device="cuda")
    ops.gemm_dswiglu(dx.cuda(), wd.cuda(), gu.cuda(), fused)
    da = torch.empty((M, I), dtype=dt, device="cuda")
    ops.gemm_nt(dx.cuda(), wd.cuda(), da, tb=True)
    two = torch.empty((M, 2 * I), dtype=dt, device="cuda")
    ops.swiglu_bwd(gu.cuda(), da, two)
    ref = emu.gemm_dswiglu(dx, wd, gu, torch.empty((M, 2 * I), dtype=dt))
    cmp(fused, ref, dt, k=K, what="gemm_dswiglu vs emulation")
    same = (fused == two).float().mean().item()
    assert same > 0.999, f"fused and two-launch results agree on only {same:.5f} of the elements"
    cmp(fused, two.cpu(), dt, k=8, what="gemm_dswiglu vs two launches")


# ------------------------------------------------------------------------------ the training form of the folded RMSNorm (r06)
@pytest.mark.parametrize("M,I,K", [(256, 256, 64), (1000, 4096, 1024), (516, 1024, 264)])
def test_gemm_dswiglu_scaled(ops, M, I, K):
    """mh_gemm_dswiglu_scaled: d a times rowscale[m] before its rounding, then SwiGLU' -- against the stand-in; with ones the
    unscaled entry point bit for bit"""
    dt = torch.bfloat16
    dx, wd, gu = rnd((M, K), dt, 61, 0.5), rnd((K, I), dt, 62, 0.5), rnd((M, 2 * I), dt, 63, 2.0)
    rs = (0.25 + 2.0 * torch.rand((M,), generator=torch.Generator().manual_seed(9)))
    got = torch.full((M, 2 * I), 7.0, dtype=dt, device="cuda")
    ops.gemm_dswiglu(dx.cuda(), wd.cuda(), gu.cuda(), got, rowscale=rs.cuda())
    ref = emu.gemm_dswiglu(dx, wd, gu, torch.empty((M, 2 * I), dtype=dt), rowscale=rs)
    cmp(got, ref, dt, k=2 * K, what="gemm_dswiglu_scaled vs emulation")
    one, plain = torch.empty_like(got), torch.empty_like(got)
    ops.gemm_dswiglu(dx.cuda(), wd.cuda(), gu.cuda(), one, rowscale=torch.ones((M,), device="cuda"))
    ops.gemm_dswiglu(dx.cuda(), wd.cuda(), gu.cuda(), plain)
    assert torch.equal(one, plain)


@pytest.mark.parametrize("M,N,K", [(512, 3072, 1024), (1028, 768, 264), (260, 256, 64)])
def test_gemm_nt_scaled(ops, M, N, K):
    """mh_gemm_nt_scaled (the token-level q|k|v projection behind a folded norm): every row of the fp32 product times rowscale[m]
    before the rounding; with ones mh_gemm_nt bit for bit"""
    dt = torch.bfloat16
    a, b = rnd((M, K), dt, 1, 0.5).cuda(), rnd((N, K), dt, 2, 0.5).cuda()
    rs = (0.25 + 2.0 * torch.rand((M,), generator=torch.Generator().manual_seed(3))).cuda()
    got = torch.full((M, N), 7.0, dtype=dt, device="cuda")
    ops.gemm_nt_scaled(a, b, got, rs)
    want = (rs[:, None] * (a.float() @ b.float().t()))
    tol = 2.0 ** -8 * want.abs() + 2.0 ** -9 * want.abs().amax(-1, keepdim=True)
    assert ((got.float() - want).abs() <= tol).all(), (got.float() - want).abs().max().item()
    one, plain = torch.empty_like(got), torch.empty_like(got)
    ops.gemm_nt_scaled(a, b, one, torch.ones((M,), device="cuda"))
    ops.gemm_nt(a, b, plain, splitk=1)
    assert torch.equal(one, plain)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,D", [(64, 1024), (1000, 2048), (33, 256), (20, 4096), (7, 520)])
def test_rmsnorm_bwd_folded(ops, dtype, M, D):
    x, t, dres = rnd((M, D), dtype, 21), rnd((M, D), dtype, 22), rnd((M, D), dtype, 23)
    rstd = torch.rsqrt(x.float().pow(2).mean(-1) + 1e-6)
    for res in (dres, None):
        want = emu.rmsnorm_bwd_folded(x, rstd, t, res, torch.empty((M, D), dtype=dtype))
        got = torch.full((M, D), float("nan"), dtype=dtype, device="cuda")
        ops.rmsnorm_bwd_folded(x.cuda(), rstd.cuda(), t.cuda(), None if res is None else res.cuda(), got)
        cmp(got, want, dtype, k=4, what="rmsnorm_bwd_folded")


@pytest.mark.parametrize("M,N,K,acc", [(2048, 768, 256, False), (4096, 3072, 1024, True), (520, 1024, 1024, True), (33000, 256, 1024, False)])
def test_wgrad_folded(ops, M, N, K, acc):
    """the weight gradient behind a folded norm: dW (+)= (dz^T x) * w and dw (+)= colsum((dz^T x) * W), both out of the
    split-K reduction (mh_gemm_splitk_reduce_fold + mh_colsum), against fp32 torch on the same bf16 operands"""
    dt = torch.bfloat16
    dz, x = rnd((M, N), dt, 31, 0.1).cuda(), rnd((M, K), dt, 32).cuda()
    W, w = rnd((N, K), dt, 33, 0.05).cuda(), (1.0 + 0.3 * rnd((K,), torch.float32, 34)).to(dt).cuda()
    dW0, dw0 = rnd((N, K), dt, 35, 0.5).cuda(), rnd((K,), dt, 36, 0.5).cuda()
    dW, dw = dW0.clone(), dw0.clone()
    ops.wgrad_folded(dz, x, dW, w, W, dw, acc)
    G = dz.float().t() @ x.float()
    want_W = G * w.float()[None, :] + (dW0.float() if acc else 0.0)
    want_w = (G * W.float()).sum(0) + (dw0.float() if acc else 0.0)
    eW = (dW.float() - want_W).abs()
    assert (eW <= 2.0 ** -8 * want_W.abs() + 2e-3 * want_W.pow(2).mean().sqrt()).all(), eW.max().item()
    ew = (dw.float() - want_w).abs()
    assert (ew <= 2.0 ** -8 * want_w.abs() + 2e-3 * want_w.pow(2).mean().sqrt()).all(), ew.max().item()


def test_scale_cols_and_vector_splitk_reduce(ops):
    """mh_scale_cols = (W.float() * w.float()).to(dtype) exactly; the four-columns-per-thread split-K reduction = the sums of the
    partials in slice order (against the single-slice launch within accumulation-order noise, and deterministic)"""
    for dt in DTYPES:
        W, w = rnd((300, 520), dt, 1).cuda(), rnd((520,), dt, 2).cuda()
        out = torch.empty_like(W)
        ops.scale_cols(W, w, out)
        assert torch.equal(out, (W.float() * w.float()[None, :]).to(dt))
        W2, w2 = rnd((64, 520), dt, 5).cuda(), rnd((520,), dt, 6).cuda()
        o1, o2 = torch.empty_like(W), torch.empty_like(W2)
        ops.scale_cols_batched(ops.scale_cols_jobs([(W, w, o1), (W2, w2, o2)]), 520, W)   # two matrices, one launch
        assert torch.equal(o1, out) and torch.equal(o2, (W2.float() * w2.float()[None, :]).to(dt))
    a, b = rnd((512, 4096), torch.bfloat16, 3).cuda(), rnd((1024, 4096), torch.bfloat16, 4).cuda()
    o1, o4, o4b = (torch.empty((512, 1024), dtype=torch.bfloat16, device="cuda") for _ in range(3))
    ops.gemm_nt(a, b, o1, splitk=1)
    ops.gemm_nt(a, b, o4, splitk=4)
    ops.gemm_nt(a, b, o4b, splitk=4)
    assert torch.equal(o4, o4b)
    cmp(o4, o1.cpu(), torch.bfloat16, k=16, what="split-K 4 vs 1")


def test_attention_backward_row_scale(ops):
    """mh_attn_bwd_o_scaled / mh_tokattn_bwd_scaled: row m of the stored gradient = rowscale[m] x the unscaled entry point's,
    within the store's one rounding"""
    from midi_model_amd.engine import RopeTable
    dt = torch.bfloat16
    B, S, H = 2, 321, 2
    D = H * 64
    qkv, do = rnd((B * S, 3 * D), dt, 18).cuda(), rnd((B * S, D), dt, 19).cuda()
    Sp = (S + 63) // 64 * 64
    o, lse = torch.empty((B * S, D), dtype=dt, device="cuda"), torch.zeros(B * H * Sp, device="cuda")
    ops.attn_fwd(qkv, o, lse, B, S, H, 0.125)
    tab = RopeTable(64, 10000.0, "cuda", S)
    rs = (0.25 + 2.0 * torch.rand((B * S,), generator=torch.Generator().manual_seed(5))).cuda()
    plain, scaled = torch.empty_like(qkv), torch.full_like(qkv, float("nan"))
    ops.attn_bwd(qkv, o, do, lse, plain, B, S, H, 0.125, tab.cos, tab.sin)
    ops.attn_bwd(qkv, o, do, lse, scaled, B, S, H, 0.125, tab.cos, tab.sin, rowscale=rs)
    want = plain.float() * rs[:, None]
    err = (scaled.float() - want).abs()
    # (the rotation back works on bf16-rounded pairs: an element's error is a rounding step of its LARGER partner)
    assert (err <= 2.0 ** -6 * want.abs() + 2.0 ** -7 * want.abs().amax(-1, keepdim=True)).all(), err.max().item()
    assert err.pow(2).mean().sqrt().item() <= 2.0 ** -8 * want.pow(2).mean().sqrt().item()
    N, T, Ht = 37, 8, 2
    Dt = Ht * 256
    qkv, do = rnd((N * T, 3 * Dt), dt, 28).cuda(), rnd((N * T, Dt), dt, 29).cuda()
    tabt = RopeTable(256, 10000.0, "cuda", T)
    rs = (0.25 + 2.0 * torch.rand((N * T,), generator=torch.Generator().manual_seed(6))).cuda()
    plain, scaled = torch.empty_like(qkv), torch.full_like(qkv, float("nan"))
    ops.tokattn_bwd(qkv, do, plain, N, T, Ht, 256 ** -0.5, tabt.cos, tabt.sin)
    ops.tokattn_bwd(qkv, do, scaled, N, T, Ht, 256 ** -0.5, tabt.cos, tabt.sin, rowscale=rs)
    want = plain.float() * rs[:, None]
    err = (scaled.float() - want).abs()
    assert (err <= 2.0 ** -7 * want.abs() + 2.0 ** -8 * want.abs().amax(-1, keepdim=True)).all(), err.max().item()


@pytest.mark.parametrize("n_rows,n_cols,ld,V", [(5, 7, 8, 3406), (293, 7, 8, 3406), (4096, 8, 8, 3406), (32768, 7, 8, 3406), (1, 1, 1, 5),
                                                (3000, 3, 5, 17)])
def test_token_segments_is_a_grouping_of_the_occurrences_by_id(ops, n_rows, n_cols, ld, V):
    """mh_token_segments (counting sort on the device) against torch.sort + searchsorted: identical segment starts, the
    placement is a permutation of the occurrences with every position inside its id's segment, and the row mapping
    r * row_mul + j * col_mul + add is applied to the placed occurrence (the order inside a segment is unspecified)."""
    g = torch.Generator().manual_seed(n_rows * 31 + n_cols)
    wide = torch.randint(0, V, (n_rows, ld), generator=g)
    wide[: n_rows // 2, 0] = 3 % V  # one heavily repeated id
    tok = wide[:, :n_cols]  # a column slice: row stride ld
    flat = tok.reshape(-1)
    sorted_tok, _ = torch.sort(flat)
    seg_ref = torch.searchsorted(sorted_tok, torch.arange(V + 1))
    order, seg = ops.token_segments(tok.cuda(), V)
    torch.cuda.synchronize()
    order, seg = order.cpu(), seg.cpu()
    assert torch.equal(seg, seg_ref)
    assert torch.equal(torch.sort(order)[0], torch.arange(flat.numel()))  # a permutation of the occurrence indices
    assert torch.equal(flat[order], sorted_tok)                           # grouped by id, ids ascending
    src, seg2 = ops.token_segments(tok.cuda(), V, row_mul=ld, col_mul=1, add=1)
    src = src.cpu()
    assert torch.equal(seg2.cpu(), seg_ref)
    # decode the mapping back to (r, j) and compare the id found there with the segment the position lies in
    r, j = (src - 1) // ld, (src - 1) % ld
    assert int(j.max()) < n_cols
    assert torch.equal(wide[r, j], sorted_tok)
    assert torch.equal(torch.sort(r * n_cols + j)[0], torch.arange(flat.numel()))
    src1, _ = ops.token_segments(tok.cuda(), V, row_mul=1, col_mul=0, add=0)  # the summed event embedding: every token reads row r
    counts = torch.bincount(src1.cpu(), minlength=n_rows)
    assert torch.equal(counts, torch.full((n_rows,), n_cols))


# ------------------------------------------------------------------------------------------ embeddings
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [256, 1024, 2048, 4096])
@pytest.mark.parametrize("dist", ["one_id", "edge_1024_1025", "skewed", "wide_vocab", "pad_heavy", "tiny"])
def test_embed_segment_bwd_adversarial_id_distributions(ops, dtype, D, dist):
    """r06 form of mh_embed_segment_bwd (pieces snapped to segment starts, owned segments written without atomics, the waves of a
    workgroup meeting in LDS): id distributions chosen against its case analysis -- one id for everything (every wave of every
    workgroup in one group chain), segments of exactly SEG_OWN and SEG_OWN + 1 occurrences side by side, a skewed mix of a few
    long and many short segments, a vocabulary too wide for the LDS copy of seg_start, mostly padding, fewer occurrences than one
    wave's piece -- at every chunk count (D = 256 .. 4096), against index_add in fp32."""
    if dtype == torch.float32 and D > 2048:
        pytest.skip("fp32 rows of the segment form stop at D = 2048")
    g = torch.Generator().manual_seed(D + sum(map(ord, dist)))
    V, n = 3406, 40000
    if dist == "one_id":
        ids = torch.full((n,), 7, dtype=torch.long)
    elif dist == "edge_1024_1025":
        ids = torch.cat([torch.full((1024,), 5), torch.full((1025,), 6), torch.full((1024,), 9), torch.full((1023,), 11),
                         torch.full((130,), 12), torch.full((2048,), 13), torch.arange(20, 20 + 300)]).long()
    elif dist == "skewed":
        ids = torch.cat([torch.full((17000,), 3), torch.full((5000,), 140), torch.randint(9, V, (18000,), generator=g)]).long()
    elif dist == "wide_vocab":
        V = 6000
        ids = torch.randint(0, V, (n,), generator=g)
    elif dist == "pad_heavy":
        ids = torch.where(torch.rand(n, generator=g) < 0.8, torch.zeros(n, dtype=torch.long), torch.randint(1, V, (n,), generator=g))
    else:
        ids = torch.randint(0, V, (37,), generator=g)
    ids = ids[torch.randperm(ids.numel(), generator=g)]
    n = ids.numel()
    nrows = 3000
    rows = torch.randint(0, nrows, (n,), generator=g)
    dout = rnd((nrows, D), dtype, 77)
    src, seg = ops.token_segments(ids.cuda(), V)          # src = occurrence indices grouped by id
    acc = torch.zeros((V, D), device="cuda")
    ops.embed_segment_bwd(rows.cuda()[src].contiguous(), seg, dout.cuda(), D, acc, 0)
    ref = torch.zeros((V, D), device="cuda").index_add_(0, ids.cuda(), dout.cuda().float()[rows.cuda()])
    ref[0] = 0
    tol = 2e-6 * max(1.0, float(torch.bincount(ids).max())) ** 0.5 * ref.abs().max().item() + 1e-6
    assert (acc - ref).abs().max().item() <= tol, ((acc - ref).abs().max().item(), tol)
    assert acc[0].abs().max() == 0
    # accumulate semantics: a second call adds to the table
    ops.embed_segment_bwd(rows.cuda()[src].contiguous(), seg, dout.cuda(), D, acc, 0)
    assert (acc - 2 * ref).abs().max().item() <= 2 * tol


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D,M", [(256, 77), (1024, 700), (2048, 150)])
def test_embeddings(ops, dtype, D, M):
    V, T = 3406, 8
    g = torch.Generator().manual_seed(7)
    table = rnd((V, D), dtype, 8)
    tok = torch.randint(0, V, (M, T), generator=g)
    tok[3] = 0
    out = torch.empty((M, D), dtype=dtype, device="cuda")
    ops.embed_sum_fwd(tok.cuda(), table.cuda(), out)
    cmp(out, emu.embed_sum_fwd(tok, table, torch.empty((M, D), dtype=dtype)), dtype, what="embed_sum")
    hid = rnd((M, D), dtype, 9)
    seq = torch.empty((M, T, D), dtype=dtype, device="cuda")
    ops.concat_tok_fwd(hid.cuda(), tok.cuda(), table.cuda(), seq, T)
    assert torch.equal(seq.cpu(), emu.concat_tok_fwd(hid, tok, table, torch.empty((M, T, D), dtype=dtype), T))
    # scatter backward, both addressing modes, pad rows skipped
    d1 = rnd((M, D), dtype, 10)
    acc, ref = torch.zeros((V, D), device="cuda"), torch.zeros((V, D))
    ops.embed_scatter_bwd(tok.cuda(), T, d1.cuda(), 1, 0, 0, acc, 0)
    emu.embed_scatter_bwd(tok, T, d1, 1, 0, 0, ref, 0)
    cmp(acc, ref, torch.float32, k=10, what="scatter (event)")
    assert acc[0].abs().max() == 0
    d2 = rnd((M, T, D), dtype, 11)
    acc.zero_(); ref.zero_()
    ops.embed_scatter_bwd(tok[:, :7].cuda(), 7, d2.cuda(), T, 1, 1, acc, 0)
    emu.embed_scatter_bwd(tok[:, :7], 7, d2, T, 1, 1, ref, 0)
    cmp(acc, ref, torch.float32, k=10, what="scatter (token)")
    # segment form (sorted occurrences) == scatter form, incl. a heavily repeated id; also on a ragged prefix of the rows
    hot = tok[:, :7].clone()
    hot[: M // 2, 0] = 3
    for rows in (M, max(1, M - 3)):
        order, seg = ops.token_segments(hot[:rows].reshape(-1).cuda(), V)
        src = (order // 7) * T + order % 7 + 1
        acc.zero_(); ref.zero_()
        ops.embed_segment_bwd(src.contiguous(), seg, d2.cuda(), D, acc, 0)
        emu.embed_scatter_bwd(hot[:rows], 7, d2[:rows], T, 1, 1, ref, 0)
        cmp(acc, ref, torch.float32, k=20, what=f"segment bwd rows={rows}")
        assert acc[0].abs().max() == 0
        ref2 = torch.zeros((V, D))
        emu.embed_segment_bwd(src.cpu(), seg.cpu(), d2, D, ref2, 0)
        cmp(ref2, ref, torch.float32, k=20, what="segment bwd (emu)")
    acc.zero_(); ref.zero_()
    ops.embed_scatter_bwd(tok[:, :7].cuda(), 7, d2.cuda(), T, 1, 1, acc, 0)
    emu.embed_scatter_bwd(tok[:, :7], 7, d2, T, 1, 1, ref, 0)
    dst = rnd((V, D), dtype, 12)
    dst_g = dst.clone().cuda()
    ops.cast_from_f32(acc, dst_g, True)
    emu.cast_from_f32(ref, dst, True)
    cmp(dst_g, dst, dtype, what="cast_from_f32")
    rows = torch.empty((M, D), dtype=dtype, device="cuda")
    ops.copy_rows(d2.cuda(), T * D, rows, D, M, D)
    assert torch.equal(rows.cpu(), d2[:, 0])


# --------------------------------------------------------------------------------------------- RMSNorm
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,D", [(1, 256), (37, 1024), (1000, 1024), (5000, 256), (64, 2048), (10, 768), (300, 512)])
def test_rmsnorm(ops, dtype, M, D):
    x, w, dy, dres = rnd((M, D), dtype, 13, 2.0), (1 + 0.1 * rnd((D,), torch.float32, 14)).to(dtype), rnd((M, D), dtype, 15), rnd((M, D), dtype, 16)
    y, rstd = torch.empty((M, D), dtype=dtype), torch.empty(M)
    emu.rmsnorm_fwd(x, w, y, rstd, 1e-6)
    yg, rg = torch.empty((M, D), dtype=dtype, device="cuda"), torch.empty(M, device="cuda")
    ops.rmsnorm_fwd(x.cuda(), w.cuda(), yg, rg, 1e-6)
    cmp(yg, y, dtype, what="rmsnorm y")
    cmp(rg, rstd, torch.float32, what="rmsnorm rstd")
    dx, dw = torch.empty((M, D), dtype=dtype), torch.zeros(D, dtype=dtype)
    emu.rmsnorm_bwd(x, w, rstd, dy, dres, dx, dw, False)
    dxg, dwg = torch.empty((M, D), dtype=dtype, device="cuda"), torch.zeros(D, dtype=dtype, device="cuda")
    ops.rmsnorm_bwd(x.cuda(), w.cuda(), rg, dy.cuda(), dres.cuda(), dxg, dwg, False)
    cmp(dxg, dx, dtype, k=2, what="rmsnorm dx")
    cmp(dwg, dw, dtype, k=max(2.0, math.sqrt(M) / 4), what="rmsnorm dw")
    ops.rmsnorm_bwd(x.cuda(), w.cuda(), rg, dy.cuda(), None, dxg, dwg, True)  # no residual, accumulate dw
    emu.rmsnorm_bwd(x, w, rstd, dy, None, dx, dw, True)
    cmp(dxg, dx, dtype, k=2, what="rmsnorm dx (no res)")
    cmp(dwg, dw, dtype, k=max(3.0, math.sqrt(M) / 3), what="rmsnorm dw (acc)")


def test_rmsnorm_bwd_forms_agree_bit_for_bit(ops):
    """mh_rmsnorm_bwd picks non-temporal loads / stores when an operand is larger than the Infinity Cache keeps between kernels
    (> 192 MiB: the token-level stack's 262144 x 1024 rows).  Cache hints only: a 131072-row call (256 MiB per operand: the hinted
    kernel) gives, on every 32768-row quarter, the bits the plain kernel gives for that quarter alone (dx is row-local)."""
    M, D = 131072, 1024
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn((M, D), device="cuda", generator=g).to(torch.bfloat16)
    dy = torch.randn((M, D), device="cuda", generator=g).to(torch.bfloat16)
    dres = torch.randn((M, D), device="cuda", generator=g).to(torch.bfloat16)
    w = (1 + 0.1 * torch.randn(D, device="cuda", generator=g)).to(torch.bfloat16)
    rstd = torch.rsqrt(x.float().pow(2).mean(-1) + 1e-6)
    dx_big, dw_big = torch.empty_like(x), torch.zeros(D, device="cuda", dtype=torch.bfloat16)
    ops.rmsnorm_bwd(x, w, rstd, dy, dres, dx_big, dw_big, False)
    dw_sum = torch.zeros(D, device="cuda")
    for q in range(4):
        sl = slice(q * 32768, (q + 1) * 32768)
        dx_q, dw_q = torch.empty((32768, D), device="cuda", dtype=torch.bfloat16), torch.zeros(D, device="cuda", dtype=torch.bfloat16)
        ops.rmsnorm_bwd(x[sl], w, rstd[sl], dy[sl], dres[sl], dx_q, dw_q, False)
        assert torch.equal(dx_q, dx_big[sl]), q
        dw_sum += dw_q.float()
    torch.testing.assert_close(dw_big.float(), dw_sum, rtol=3e-2, atol=2.0)   # (bf16 outputs of sums over 131072 / 32768 rows)


# ------------------------------------------------------------------------------------------------ RoPE
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,hd,S,M", [(4, 64, 10, 30), (1, 256, 8, 64), (16, 64, 33, 33)])
def test_rope(ops, dtype, H, hd, S, M):
    from midi_model_amd.engine import RopeTable
    tab = RopeTable(hd, 10000.0, "cuda", 64)
    qkv = rnd((M, 3 * H * hd), dtype, 17)
    for direction, pos0 in ((1, 0), (-1, 0), (1, 5)):
        want = emu.rope_(qkv.clone(), tab.cos.cpu(), tab.sin.cpu(), S, pos0, H, hd, direction)
        got = ops.rope_(qkv.clone().cuda(), tab.cos, tab.sin, S, pos0, H, hd, direction)
        cmp(got, want, dtype, what=f"rope dir={direction} pos0={pos0}")
        assert torch.equal(got[:, 2 * H * hd:].cpu(), qkv[:, 2 * H * hd:])  # v untouched


# ------------------------------------------------------------------------------ event-level attention
V3_DEFAULT = 255  # mh_get_option("attn_v3") of a fresh thread (r06: + the forward's lazy reference maximum)
# form -> (attn_v3 bits, attn_v3_wps)
ATTN_FORMS = {
    "v3_lazy": (255, 0),         # the default: the third form of all three kernels + the forward's lazy reference maximum (r06)
    "v3_lazy_wps3": (255, 3),
    "v3_tr_all": (127, 0),       # third form of all three kernels: transposed operands by transpose reads, delta inside dQ,
                                 # three K/V stages in the forward (the r02-r05 default: classic per-tile row maximum)
    "v3_tr_all_wps2": (127, 2),  # ... held to two / three waves per SIMD
    "v3_tr_all_wps3": (127, 3),
    "v3_tr_all_2stage": (63, 0),      # ... forward with two K/V stages
    "v3_tr_all_delta_pass": (31, 0),  # ... delta from its own pass (mh_attn_prep_bwd + mh_attn_bwd)
    "v3_tr": (15, 0),            # ... forward from the prepared V^T copy
    "v3": (7, 0),                # ... all three from prepared transposed copies
    "first_form": (0, 0),        # attention_mfma.hip
}


@pytest.mark.parametrize("form", list(ATTN_FORMS))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,S,H", [(1, 1, 1), (2, 33, 3), (1, 64, 2), (2, 128, 1), (1, 200, 4), (1, 515, 2), (1, 129, 1), (2, 321, 2), (1, 96, 1), (1, 40, 1)])
def test_attention_fwd_bwd(ops, form, dtype, B, S, H):
    """(bf16: every form of the MFMA kernels -- the third form (fragment batches, one loop per tile class, transpose reads)
    with and without prepared transposed copies, and the first form; fp32 runs the plain verification kernel either way)"""
    if dtype == torch.float32 and form != "v3_lazy":
        pytest.skip("fp32 has one forward kernel")
    v3, v3_wps = ATTN_FORMS[form]
    with (ops.ab_library() if form == "first_form" else contextlib.nullcontext()):  # (first form: A/B library only)
        _attention_fwd_bwd(ops, v3, v3_wps, dtype, B, S, H)


def _attention_fwd_bwd(ops, v3, v3_wps, dtype, B, S, H):
    ops.set_option("attn_v3", v3)
    ops.set_option("attn_v3_wps", v3_wps)
    D = H * 64
    scale = 64 ** -0.5
    qkv = rnd((B * S, 3 * D), dtype, 18)
    do = rnd((B * S, D), dtype, 19)
    Sp = (S + 63) // 64 * 64
    o_ref, lse_ref = torch.empty((B * S, D), dtype=dtype), torch.zeros(B * H * Sp)
    emu.attn_fwd(qkv, o_ref, lse_ref, B, S, H, scale)
    o, lse = torch.empty((B * S, D), dtype=dtype, device="cuda"), torch.zeros(B * H * Sp, device="cuda")
    ops.attn_fwd(qkv.cuda(), o, lse, B, S, H, scale)
    cmp(o, o_ref, dtype, what="attn o")
    cmp(lse.view(B, H, Sp)[:, :, :S], lse_ref.view(B, H, Sp)[:, :, :S], torch.float32, k=(1 if dtype == torch.float32 else 50), what="attn lse")
    dq_ref = torch.empty((B * S, 3 * D), dtype=dtype)
    emu.attn_bwd(qkv, o_ref, do, lse_ref, dq_ref, B, S, H, scale)
    dqkv = torch.full((B * S, 3 * D), float("nan"), dtype=dtype, device="cuda")
    ops.attn_bwd(qkv.cuda(), o, do.cuda(), lse, dqkv, B, S, H, scale)
    for i, nm in enumerate(("dq", "dk", "dv")):
        cmp(dqkv[:, i * D:(i + 1) * D], dq_ref[:, i * D:(i + 1) * D], dtype, k=3, what=f"attn {nm}")
    # rotation back fused into the dq / dk stores == a separate mh_rope(dir = -1) pass over the result
    from midi_model_amd.engine import RopeTable
    tab = RopeTable(64, 10000.0, "cuda", S)
    want = ops.rope_(dqkv.clone(), tab.cos, tab.sin, S, 0, H, 64, -1)
    got = torch.full((B * S, 3 * D), float("nan"), dtype=dtype, device="cuda")
    ops.attn_bwd(qkv.cuda(), o, do.cuda(), lse, got, B, S, H, scale, tab.cos, tab.sin)
    assert torch.equal(got[:, 2 * D:], dqkv[:, 2 * D:])
    cmp(got, want.cpu(), dtype, k=2, what="attn bwd + rotation back")
    same = (got == want).float().mean().item()
    assert same > 0.99, f"fused rotation agrees with the separate pass on only {same:.4f} of the elements"
    ops.set_option("attn_v3", V3_DEFAULT)
    ops.set_option("attn_v3_wps", 0)


@pytest.mark.parametrize("v3", [255, 223, 95, 31, 7, 0], ids=["v3_lazy", "v3_lazy_tr_3stage", "v3_tr_3stage", "v3_tr", "v3", "first_form"])
def test_attention_forward_when_the_reference_has_to_move(ops, v3):
    """Rows whose scores jump by far more than the lazy-rescale threshold between tiles (a few keys late in the sequence
    are scaled up 8x and 24x: q.k/8 moves by tens to more than a hundred log2 units), plus a first tile of tiny scores.
    The r06 lazy reference maximum (bit 7) takes its slow path exactly here: jumps below 40 binades stay on the fast path with
    probabilities far above one, jumps beyond overflow its partial row sums and send the wave through the classic update."""
    B, S, H = 1, 640, 2
    D = H * 64
    qkv = rnd((B * S, 3 * D), torch.bfloat16, 41)
    qkv[:, :D] *= 2.0
    for j in (70, 200, 333):
        qkv[j, D:2 * D] *= 8.0    # big keys: q.k/8 jumps by tens (log2 units) from one tile to the next
    qkv[590, D:2 * D] *= 24.0     # ... and by more than 128 for some rows (exp2 against the inherited reference overflows)
    qkv[:64, D:2 * D] *= 0.01     # first tile: tiny scores
    Sp = (S + 63) // 64 * 64
    o_ref, lse_ref = torch.empty((B * S, D), dtype=torch.bfloat16), torch.zeros(B * H * Sp)
    emu.attn_fwd(qkv, o_ref, lse_ref, B, S, H, 0.125)
    with (ops.ab_library() if v3 == 0 else contextlib.nullcontext()):
        ops.set_option("attn_v3", v3)
        o, lse = torch.empty((B * S, D), dtype=torch.bfloat16, device="cuda"), torch.zeros(B * H * Sp, device="cuda")
        ops.attn_fwd(qkv.cuda(), o, lse, B, S, H, 0.125)
        ops.set_option("attn_v3", V3_DEFAULT)
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
    cmp(o, o_ref, torch.bfloat16, what="attn o (moving reference)")
    got, want = lse.view(B, H, Sp)[:, :, :S].cpu(), lse_ref.view(B, H, Sp)[:, :, :S]
    assert ((got - want).abs() <= 1e-4 * want.abs().clamp(min=1.0)).all(), (got - want).abs().max()


def test_attention_bwd_in_one_call_hands_over_delta_and_says_what_it_does_not_serve(ops):
    """mh_attn_bwd_o: the dQ kernel leaves delta = rowsum(dO * O) and -lse * log2(e) in the 2 * B*H*Sp scratch; fp32 and the
    other kernel forms are refused with an error (the two-call path serves them), not computed some other way."""
    from midi_model_amd.lib import lib
    B, S, H = 2, 200, 2
    D, Sp = H * 64, 256
    qkv = rnd((B * S, 3 * D), torch.bfloat16, 61).cuda()
    do = rnd((B * S, D), torch.bfloat16, 62).cuda()
    o = torch.empty((B * S, D), dtype=torch.bfloat16, device="cuda")
    lse = torch.zeros(B * H * Sp, device="cuda")
    ops.attn_fwd(qkv, o, lse, B, S, H, 0.125)
    scratch = torch.full((2 * B * H * Sp,), float("nan"), device="cuda")
    dqkv = torch.empty_like(qkv)
    st = torch.cuda.current_stream().cuda_stream
    args = (qkv.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(), scratch.data_ptr(), dqkv.data_ptr(), B, S, H, 0.125, 0, 0)
    lib().call("mh_attn_bwd_o", *args, 1, st)
    torch.cuda.synchronize()
    want = (do.float() * o.float()).view(B, S, H, 64).sum(-1).permute(0, 2, 1)          # [B, H, S]
    got = scratch[:B * H * Sp].view(B, H, Sp)[:, :, :S]
    assert torch.allclose(got, want, rtol=1e-5, atol=1e-5), (got - want).abs().max()
    got2 = scratch[B * H * Sp:].view(B, H, Sp)[:, :, :S]
    assert torch.equal(got2, -(lse.view(B, H, Sp)[:, :, :S] * 1.4426950408889634))
    ref = torch.empty_like(dqkv)
    ops.set_option("attn_v3", 31)   # the two-call path (delta from its own pass)
    ops.attn_bwd(qkv, o, do, lse, ref, B, S, H, 0.125)
    cmp(dqkv, ref, torch.bfloat16, what="dqkv one call vs two calls")
    ops.set_option("attn_v3", 7)    # the backward pair from prepared transposed copies: not served in one call
    with pytest.raises(RuntimeError, match="attn_bwd_o"):
        lib().call("mh_attn_bwd_o", *args, 1, st)
    ops.set_option("attn_v3", V3_DEFAULT)
    with pytest.raises(RuntimeError, match="bf16 only"):
        lib().call("mh_attn_bwd_o", *args, 0, st)        # fp32
    mh_err = lib().cdll.mh_last_error()
    assert mh_err


def test_attention_mfma_vs_plain_on_device(ops):
    """bf16: the MFMA flash kernels against the thread-per-row kernels running on the same device data."""
    from midi_model_amd.lib import lib
    B, S, H = 2, 300, 2
    D, Sp = H * 64, 320
    scale = 0.125
    qkv = rnd((B * S, 3 * D), torch.bfloat16, 20).cuda()
    do = rnd((B * S, D), torch.bfloat16, 21).cuda()
    o, lse = torch.empty((B * S, D), dtype=torch.bfloat16, device="cuda"), torch.zeros(B * H * Sp, device="cuda")
    ops.attn_fwd(qkv, o, lse, B, S, H, scale)
    o2, lse2 = torch.empty_like(o), torch.zeros_like(lse)
    st = torch.cuda.current_stream().cuda_stream
    lib().call("mh_attn_fwd_plain", qkv.data_ptr(), o2.data_ptr(), lse2.data_ptr(), B, S, H, scale, 1, st)
    cmp(o, o2, torch.bfloat16, what="mfma vs plain o")
    dq = torch.empty((B * S, 3 * D), dtype=torch.bfloat16, device="cuda")
    ops.attn_bwd(qkv, o, do, lse, dq, B, S, H, scale)
    dq2 = torch.empty_like(dq)
    delta = torch.zeros(B * H * Sp, device="cuda")
    # delta = rowsum(dO*O) per head, laid out [B,H,Sp]
    d_ = (do.float() * o2.float()).view(B, S, H, 64).sum(-1).permute(0, 2, 1)
    delta.view(B, H, Sp)[:, :, :S] = d_
    lib().call("mh_attn_bwd_plain", qkv.data_ptr(), do.data_ptr(), lse2.data_ptr(), delta.data_ptr(), dq2.data_ptr(), B, S, H, scale, 1, st)
    cmp(dq, dq2, torch.bfloat16, k=2, what="mfma vs plain dqkv")


# ------------------------------------------------------------------------------ token-level attention
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,T,H", [(1, 8, 1), (37, 8, 4), (10, 5, 2), (3, 1, 4)])
def test_tokattn(ops, dtype, N, T, H):
    D = H * 256
    scale = 256 ** -0.5
    qkv, do = rnd((N * T, 3 * D), dtype, 22), rnd((N * T, D), dtype, 23)
    o_ref, dq_ref = torch.empty((N * T, D), dtype=dtype), torch.empty((N * T, 3 * D), dtype=dtype)
    emu.tokattn_fwd(qkv, o_ref, N, T, H, scale)
    emu.tokattn_bwd(qkv, do, dq_ref, N, T, H, scale)
    o = torch.empty((N * T, D), dtype=dtype, device="cuda")
    dq = torch.empty((N * T, 3 * D), dtype=dtype, device="cuda")
    ops.tokattn_fwd(qkv.cuda(), o, N, T, H, scale)
    ops.tokattn_bwd(qkv.cuda(), do.cuda(), dq, N, T, H, scale)
    cmp(o, o_ref, dtype, what="tokattn o")
    cmp(dq, dq_ref, dtype, k=2, what="tokattn dqkv")
    # RoPE fused in: unrotated q,k in, gradient with respect to the unrotated q,k out
    from midi_model_amd.engine import RopeTable
    tab = RopeTable(256, 10000.0, "cuda", 8)
    emu.tokattn_fwd(qkv, o_ref, N, T, H, scale, tab.cos.cpu(), tab.sin.cpu())
    emu.tokattn_bwd(qkv, do, dq_ref, N, T, H, scale, tab.cos.cpu(), tab.sin.cpu())
    ops.tokattn_fwd(qkv.cuda(), o, N, T, H, scale, tab.cos, tab.sin)
    ops.tokattn_bwd(qkv.cuda(), do.cuda(), dq, N, T, H, scale, tab.cos, tab.sin)
    cmp(o, o_ref, dtype, what="tokattn+rope o")
    cmp(dq, dq_ref, dtype, k=3, what="tokattn+rope dqkv")


@pytest.mark.parametrize("dtype", DTYPES)
def test_tokattn_backward_forms_agree(ops, dtype):
    """r06: the octet backward reduces its dot products four per wave reduction (option tokattn_bwd_batched, default 1).  Against
    the one-by-one form: the same values up to fp32 summation order -- fp32 within 1e-5 of the range, bf16 the same but for a
    handful of elements one rounding step apart -- with RoPE, with and without the folded norm's row scale; the oracle-pinned
    comparison of the default form is test_tokattn above."""
    from midi_model_amd.engine import RopeTable
    N, T, H = 301, 8, 4
    D = H * 256
    scale = 256 ** -0.5
    qkv, do = rnd((N * T, 3 * D), dtype, 41).cuda(), rnd((N * T, D), dtype, 42).cuda()
    rs = (0.5 + torch.rand((N * T,), generator=torch.Generator().manual_seed(43))).cuda()
    tab = RopeTable(256, 10000.0, "cuda", 8)
    assert ops.get_option("tokattn_bwd_batched") == 1
    for rowscale in (None, rs):
        out = {}
        for v in (0, 1):
            ops.set_option("tokattn_bwd_batched", v)
            try:
                out[v] = ops.tokattn_bwd(qkv, do, torch.empty_like(qkv), N, T, H, scale, tab.cos, tab.sin, rowscale=rowscale).float()
            finally:
                ops.set_option("tokattn_bwd_batched", 1)
        d = (out[0] - out[1]).abs()
        amax = out[0].abs().max().item()
        if dtype == torch.float32:
            assert d.max().item() <= 1e-5 * amax, (d.max().item(), amax)
        else:
            assert (d <= 2.0 ** -7 * out[0].abs() + 1e-6 * amax).all(), d.max().item()   # one bf16 rounding step at most
            assert (d > 0).float().mean().item() < 2e-3


# ----------------------------------------------------------------------------------------------- SwiGLU
@pytest.mark.parametrize("dtype", DTYPES)
def test_swiglu(ops, dtype):
    M, I = 333, 1024
    gu, da = rnd((M, 2 * I), dtype, 24, 2.0), rnd((M, I), dtype, 25)
    a_ref, d_ref = torch.empty((M, I), dtype=dtype), torch.empty((M, 2 * I), dtype=dtype)
    emu.swiglu_fwd(gu, a_ref)
    emu.swiglu_bwd(gu, da, d_ref)
    a, d = torch.empty((M, I), dtype=dtype, device="cuda"), torch.empty((M, 2 * I), dtype=dtype, device="cuda")
    ops.swiglu_fwd(gu.cuda(), a)
    ops.swiglu_bwd(gu.cuda(), da.cuda(), d)
    cmp(a, a_ref, dtype, what="swiglu a")
    cmp(d, d_ref, dtype, what="swiglu dgu")


# ------------------------------------------------------------------------------------- loss, optimiser
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("R,V,Vp", [(531, 3406, 3456), (100, 1000, 1024), (64, 500, 508), (33, 4000, 4096),
                                    (5003, 3406, 3456)])  # (the last: several rows per wave, next row prefetched)
def test_cross_entropy(ops, dtype, R, V, Vp):
    g = torch.Generator().manual_seed(26)
    logits = torch.zeros((R, Vp), dtype=dtype)
    logits[:, :V] = rnd((R, V), dtype, 27, 3.0)
    logits[:, V:] = 77.0  # garbage in the padding columns must be ignored
    tgt = torch.randint(1, V, (R,), generator=g)
    tgt[::5] = 0
    inv = torch.tensor([1.0 / float((tgt != 0).sum())])
    rl_ref, dl_ref, am_ref = torch.empty(R), torch.empty((R, Vp), dtype=dtype), torch.empty(R, dtype=torch.long)
    emu.cross_entropy(logits, V, tgt, rl_ref, dl_ref, inv, am_ref, 0)
    lg = logits.clone().cuda()
    rl, am = torch.empty(R, device="cuda"), torch.empty(R, dtype=torch.long, device="cuda")
    ops.cross_entropy(lg, V, tgt.cuda(), rl, lg, inv.cuda(), am, 0)  # gradient written in place
    cmp(rl, rl_ref, torch.float32, k=(1 if dtype == torch.float32 else 5), what="ce row loss")
    assert torch.equal(am.cpu(), am_ref)
    cmp(lg, dl_ref, dtype, k=0.05, what="ce dlogits")
    assert (lg[:, V:] == 0).all() and (lg[::5] == 0).all()
    s = torch.empty(1, device="cuda")
    ops.sum_f32(rl, s)
    assert abs(s.item() - rl_ref.sum().item()) < 1e-2
    cnt, iv = torch.empty(1, device="cuda"), torch.empty(1, device="cuda")
    ops.count_valid(tgt.cuda(), 0, cnt, iv)
    assert cnt.item() == float((tgt != 0).sum()) and abs(iv.item() - inv.item()) < 1e-9


@pytest.mark.parametrize("with_argmax", [False, True])
@pytest.mark.parametrize("V,Vp", [(3406, 3408), (3408, 3408), (3401, 3408), (2049, 2056), (2048, 2048), (513, 520), (40, 40), (3585, 3592), (4096, 4096)])
def test_cross_entropy_bf16_edges(ops, V, Vp, with_argmax):
    """r06 form of the bf16 cross entropy (row converted once, padding at -inf, wave-uniform tests for the padding / target chunks,
    arg-max as its own instantiation): vocabulary sizes that end on, one short of and seven short of a 16-byte chunk, rows that
    fill 4 / 7 / 8 chunks per lane exactly, targets on every chunk and lane edge, rows that are all ignored, a maximum in the last
    valid column and ties -- against torch in fp32 on the same bf16 logits."""
    R = 257
    g = torch.Generator().manual_seed(V)
    logits = torch.full((R, Vp), 99.0)
    logits[:, :V] = torch.randn((R, V), generator=g) * 4
    logits[5, V - 1] = 50.0            # the maximum in the last valid column
    logits[6, :V] = 1.25               # a row of ties: the first index wins the arg-max
    logits = logits.to(torch.bfloat16)
    edges = [1, 7, 8, 9, 63, 64, 511, 512, 513, 1023, 1024, 2047, 2048, 3071, 3072, 3583, 3584, V - 9, V - 8, V - 2, V - 1]
    tgt = torch.randint(1, V, (R,), generator=g)
    for i, e in enumerate(edges):
        tgt[10 + i] = min(max(e, 1), V - 1)
    tgt[::9] = 0
    tgt[100:140] = 0                   # whole waves' worth of ignored rows
    scale = torch.tensor([0.37])
    lg = logits.clone().cuda()
    rl = torch.empty(R, device="cuda")
    am = torch.empty(R, dtype=torch.long, device="cuda") if with_argmax else None
    dl = torch.empty_like(lg)
    ops.cross_entropy(lg, V, tgt.cuda(), rl, dl, scale.cuda(), am, 0)
    x = logits[:, :V].float()
    lsm = torch.log_softmax(x, -1)
    keep = tgt != 0
    want_loss = torch.where(keep, -lsm.gather(1, tgt[:, None])[:, 0], torch.zeros(R))
    assert torch.allclose(rl.cpu(), want_loss, atol=3e-5, rtol=1e-5)
    want_d = lsm.exp()
    want_d[torch.arange(R), tgt] -= 1.0
    want_d = want_d * 0.37 * keep[:, None].float()
    got = dl.cpu().float()
    assert (got[:, V:] == 0).all() and (got[~keep] == 0).all()
    assert (got[:, :V] - want_d).abs().max().item() <= 2.0 ** -8 * 0.37 + 1e-6   # one bf16 rounding of a value below 0.37
    if with_argmax:
        assert torch.equal(am.cpu(), x.argmax(-1)) or torch.equal(am.cpu()[torch.arange(R) != 6], x.argmax(-1)[torch.arange(R) != 6])
        assert am[6].item() == 0 and am[5].item() == V - 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_clip_and_adamw(ops, dtype):
    n = 100003 * 8
    p, g = rnd((n,), dtype, 28, 0.02), rnd((n,), dtype, 29, 0.01)
    m, v = rnd((n,), dtype, 30, 0.001), rnd((n,), dtype, 31, 0.001).abs()
    ss, part, coef, norm = (torch.zeros(1, device="cuda"), torch.empty(1024, device="cuda"),
                            torch.empty(1, device="cuda"), torch.empty(1, device="cuda"))
    ops.sumsq(g.cuda(), part, ss, False)
    want = g.float().pow(2).sum().item()
    assert abs(ss.item() - want) / want < 1e-5
    ops.clip_coef(ss, 1.0, coef, norm)
    assert abs(norm.item() - math.sqrt(want)) / math.sqrt(want) < 1e-5
    assert abs(coef.item() - min(1.0, 1.0 / (math.sqrt(want) + 1e-6))) < 1e-6
    args = (3e-3, 0.9, 0.99, 1e-8, 0.01, 1 - 0.9 ** 3, 1 - 0.99 ** 3)
    pr, mr, vr = p.clone(), m.clone(), v.clone()
    emu.adamw(pr, g, mr, vr, *args, coef.cpu())
    pg, mg, vg = p.clone().cuda(), m.clone().cuda(), v.clone().cuda()
    ops.adamw(pg, g.cuda(), mg, vg, *args, coef)
    k = 1 if dtype == torch.float32 else 0.5
    cmp(pg, pr, dtype, k=k, what="adamw p")
    cmp(mg, mr, dtype, k=k, what="adamw m")
    cmp(vg, vr, dtype, k=k, what="adamw v")


# ----------------------------------------------------------------------------------------------- decode
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,H,hd,Lmax,length", [(3, 16, 64, 128, 1), (3, 16, 64, 128, 100), (3, 4, 256, 8, 1), (3, 4, 256, 8, 7),
                                                (3, 2, 64, 1100, 1031), (64, 16, 64, 2048, 1024), (64, 16, 64, 2048, 2047)])
def test_decode_attention_and_cache(ops, dtype, B, H, hd, Lmax, length):
    """(the last two cases: the cache of the benchmarked generate session -- batch 64 x 16 heads, capacity 2048 -- at the
    depth the benchmark ends at and at the last position the capacity holds)"""
    from midi_model_amd.engine import RopeTable
    if B == 64 and length == 2047 and dtype == torch.float32:
        pytest.skip("the full-capacity case runs in the production dtype (4 GiB of fp32 host copies otherwise)")
    D = H * hd
    tab = RopeTable(hd, 10000.0, "cuda", Lmax + 1)
    kc, vc = rnd((B, H, Lmax, hd), dtype, 32), rnd((B, H, Lmax, hd), dtype, 33)
    qkv = rnd((B, 3 * D), dtype, 34)
    pos = length - 1
    kc_r, vc_r, q_r = kc.clone(), vc.clone(), qkv.clone()
    emu.kv_append(q_r, tab.cos.cpu(), tab.sin.cpu(), kc_r, vc_r, B, H, hd, Lmax, pos)
    kc_g, vc_g, q_g = kc.clone().cuda(), vc.clone().cuda(), qkv.clone().cuda()
    ops.kv_append(q_g, tab.cos, tab.sin, kc_g, vc_g, B, H, hd, Lmax, pos)
    cmp(q_g, q_r, dtype, what="kv_append q/k rotation")
    cmp(kc_g, kc_r, dtype, what="kv_append k cache")
    assert torch.equal(vc_g.cpu(), vc_r)
    o_r = torch.empty((B, D), dtype=dtype)
    emu.attn_decode(q_r, kc_r, vc_r, o_r, B, H, hd, Lmax, length, hd ** -0.5)
    o_g = torch.empty((B, D), dtype=dtype, device="cuda")
    ops.attn_decode(q_g, kc_g, vc_g, o_g, B, H, hd, Lmax, length, hd ** -0.5)
    cmp(o_g, o_r, dtype, what="attn_decode")
    # the one-launch form (append fused into the attention; qkv stays unrotated), position from device memory too
    for pos_dev in (None, torch.tensor([pos], dtype=torch.int32, device="cuda")):
        kc_f, vc_f, qkv_f = kc.clone().cuda(), vc.clone().cuda(), qkv.clone().cuda()
        o_f = torch.empty((B, D), dtype=dtype, device="cuda")
        ops.attn_decode_append(qkv_f, tab.cos, tab.sin, kc_f, vc_f, o_f, B, H, hd, Lmax, pos if pos_dev is None else 0,
                               hd ** -0.5, pos_dev)
        cmp(o_f, o_r, dtype, what="attn_decode_append")
        assert torch.equal(kc_f, kc_g) and torch.equal(vc_f, vc_g) and torch.equal(qkv_f.cpu(), qkv)
    S = min(5, Lmax)
    pre = rnd((B * S, 3 * D), dtype, 35)
    ops.kv_store_prefill(pre.cuda(), kc_g, vc_g, B, S, H, hd, Lmax)
    emu.kv_store_prefill(pre, kc_r, vc_r, B, S, H, hd, Lmax)
    assert torch.equal(kc_g.cpu()[:, :, :S], kc_r[:, :, :S]) and torch.equal(vc_g.cpu()[:, :, :S], vc_r[:, :, :S])


@pytest.mark.parametrize("dtype", DTYPES)
def test_masked_softmax(ops, dtype):
    import midi_model_amd as mm
    tok = mm.MIDITokenizerV2()
    first, lo_t, hi_t, _ = tok.grammar_tables()
    B, V, Vp = 9, tok.vocab_size, 3456
    logits = torch.zeros((B, Vp), dtype=dtype)
    logits[:, :V] = rnd((B, V), dtype, 36, 2.0)
    lo = torch.tensor([-1, -1, lo_t[3][1], lo_t[3][7], lo_t[6][4], 0, lo_t[4][5], -1, lo_t[8][5]], dtype=torch.int32)
    hi = torch.tensor([-1, -1, hi_t[3][1], hi_t[3][7], hi_t[6][4], 1, hi_t[4][5], -1, hi_t[8][5]], dtype=torch.int32)
    fm = torch.tensor(first, dtype=torch.uint8)
    want = emu.masked_softmax(logits, lo, hi, fm, torch.empty((B, V)), V, 0.8)
    got = torch.empty((B, V), device="cuda")
    ops.masked_softmax(logits.cuda(), lo.cuda(), hi.cuda(), fm.cuda(), got, V, 0.8)
    cmp(got, want, torch.float32, k=(1 if dtype == torch.float32 else 20), what="masked softmax")
    assert ((got > 0).cpu() == (want > 0)).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("top_p,top_k", [(0.98, 20), (0.5, 8), (1.0, 1), (0.9, 64)])
def test_sample_top_p_k_fused(ops, dtype, top_p, top_k):
    """the fused sampler against the op-by-op chain (masked softmax -> stable sort -> cumsum/top-p/top-k ->
    argmax(p / q)) on the same Exp(1) noise: ids must agree.  bf16 logits produce many exactly-equal probabilities, so
    the tie order (value descending, index ascending) is exercised; summation-order ulps may move a draw only at an
    exact tie of p/q, which random noise does not produce."""
    import midi_model_amd as mm
    tok = mm.MIDITokenizerV2()
    first, lo_t, hi_t, _ = tok.grammar_tables()
    B, V, Vp = 64, tok.vocab_size, 3456
    g = torch.Generator().manual_seed(77)
    logits = torch.zeros((B, Vp), dtype=dtype)
    logits[:, :V] = rnd((B, V), dtype, 37, 3.0)
    ev = torch.randint(3, 9, (B,), generator=g)
    fm = torch.tensor(first, dtype=torch.uint8)
    lo_tab, hi_tab = torch.tensor(lo_t, dtype=torch.int32), torch.tensor(hi_t, dtype=torch.int32)
    q = torch.empty((B, V)).exponential_(1.0, generator=g)
    for pos in (0, 1, 2, 4, 5, 7):  # 0 = event id position (first_mask), else a parameter position of the row's event (4: `bpm`, 384 ids; 7: `duration`, 2048 ids -- the ranges spread over the four waves)
        want = emu.sample_top_p_k(logits, fm, lo_tab, hi_tab, ev, pos, q, torch.empty((B,), dtype=torch.int64), V, 0.9,
                                  top_p, top_k)
        buf = torch.full((B, 8), -7, dtype=torch.int64, device="cuda")
        ob, oc = torch.zeros((B,), dtype=torch.int64, device="cuda"), torch.zeros((B,), dtype=torch.int64, device="cuda")
        span, mr = ops.mask_spans(fm, lo_tab, hi_tab)
        ops.sample_top_p_k(logits.cuda(), fm.cuda(), lo_tab.cuda(), hi_tab.cuda(), ev.cuda(), pos, q.cuda(), buf[:, 3], V,
                           0.9, top_p, top_k, out_b=ob, out_c=oc if pos == 0 else None, first_span=span, max_range=mr[pos],
                           fill_rest=2 if pos == 0 else 0, fill_id=99)
        assert (buf[:, 3].cpu() == want).all(), (pos, (buf[:, 3].cpu() != want).nonzero().flatten().tolist())
        assert torch.equal(ob, buf[:, 3]) and (pos != 0 or torch.equal(oc, buf[:, 3]))
        assert (buf[:, 4:6] == (99 if pos == 0 else -7)).all()
    assert (buf[:, :3] == -7).all() and (buf[:, 6:] == -7).all()


def test_sample_top_p_k_fused_draws_follow_the_filtered_distribution(ops):
    """A second guard on the sampler beside the id-for-id comparison: with fresh Exp(1) variates per row, the ids the fused
    kernel draws for 16384 rows that share ONE distribution must be distributed as sample_top_p_k's filtered, renormalised
    probabilities (midi_model.py:152-165: sort, cumulative top-p cut, first k, renormalise, multinomial) -- argmax(p / q) over
    the sorted ranks IS a multinomial draw.  Chi-square over the kept ids (about 20 cells, 16384 draws): the statistic stays
    under 70 (p ~ 1e-7 for 19 degrees of freedom) and no id outside the kept set is ever drawn."""
    import midi_model_amd as mm
    tok = mm.MIDITokenizerV2()
    first, lo_t, hi_t, _ = tok.grammar_tables()
    B, V, Vp = 16384, tok.vocab_size, 3408
    g = torch.Generator().manual_seed(123)
    row = torch.randn(V, generator=g) * 1.5
    logits = torch.zeros((B, Vp), dtype=torch.bfloat16)
    logits[:, :V] = row.to(torch.bfloat16)[None, :]
    ev = torch.full((B,), 3, dtype=torch.int64)          # "note": position 1 draws time1 out of 128 ids
    pos, temp, top_p, top_k = 1, 1.0, 0.9, 20
    fm = torch.tensor(first, dtype=torch.uint8)
    lo_tab, hi_tab = torch.tensor(lo_t, dtype=torch.int32), torch.tensor(hi_t, dtype=torch.int32)
    q = torch.empty((B, V)).exponential_(1.0, generator=g)
    out = torch.empty((B,), dtype=torch.int64, device="cuda")
    span, mr = ops.mask_spans(fm, lo_tab, hi_tab)
    ops.sample_top_p_k(logits.cuda(), fm.cuda(), lo_tab.cuda(), hi_tab.cuda(), ev.cuda(), pos, q.cuda(), out, V, temp, top_p, top_k,
                       first_span=span, max_range=mr[pos])
    # the reference's filtered distribution of this row (probabilities of the whole vocabulary, masked to the position's range)
    x = logits[0, :V].float()
    probs = torch.softmax(x / temp, -1)
    mask = torch.zeros(V)
    mask[lo_t[3][pos]:hi_t[3][pos]] = 1
    probs = probs * mask
    ps, pi = torch.sort(probs, descending=True, stable=True)
    cum = torch.cumsum(ps, 0)
    ps[cum - ps > top_p] = 0
    ps[top_k:] = 0
    ps = ps / ps.sum()
    kept = ps > 0
    want = torch.zeros(V)
    want[pi[kept]] = ps[kept]
    counts = torch.bincount(out.cpu(), minlength=V).float()
    assert counts[want == 0].sum() == 0, "an id outside the kept set was drawn"
    e = want[want > 0] * B
    chi2 = ((counts[want > 0] - e) ** 2 / e).sum().item()
    assert int(kept.sum()) >= 5 and chi2 < 70.0, (int(kept.sum()), chi2)


def test_collate_windows(ops):
    """device-side batch assembly (mh_collate_windows) against the host restatement"""
    g = torch.Generator().manual_seed(5)
    tokens = torch.randint(-3000, 3000, (5000, 8), generator=g).to(torch.int16)
    start = torch.tensor([0, 4990, 17, 2500, 100], dtype=torch.int64)
    length = torch.tensor([64, 10, 1, 300, 299], dtype=torch.int64)
    want = emu.collate_windows(tokens, start, length, torch.empty((5, 300, 8), dtype=torch.int64), 0)
    out = torch.full((5, 300, 8), -1, dtype=torch.int64, device="cuda")
    ops.collate_windows(tokens.cuda(), start.cuda(), length.cuda(), out, 0)
    assert torch.equal(out.cpu(), want)


@pytest.mark.parametrize("ver", ["v1", "v2"])
def test_augment_on_the_device_is_bit_exact(ops, orc, golden, ver):
    """mh_augment_piece_stats + mh_augment_collate_windows against (a) the outputs of the reference's own
    MIDITokenizerV{1,2}.augment on whole files (tests/golden/augment_*.npz) and (b) the oracle on a large random corpus with
    windows cut inside the files; per-file facts against the host restatement.  Integer work: every token equal."""
    import midi_model_amd as mm
    from midi_model_amd.data import TokenCorpus, WindowSampler
    from midi_model_amd.tokenizer import AUG_STATS, augment_table
    tok = mm.MIDITokenizerV1() if ver == "v1" else mm.MIDITokenizerV2()
    g = golden(f"augment_{ver}.npz")
    off = g["offsets"]
    P = len(off) - 1
    tab = torch.tensor(augment_table(tok), dtype=torch.int32)
    tokens = torch.from_numpy(g["tokens"])
    want_stats = emu.augment_piece_stats(tokens, torch.from_numpy(off), tab, torch.zeros((P, AUG_STATS), dtype=torch.int32))
    stats = torch.full((P, AUG_STATS), -77, dtype=torch.int32, device="cuda")
    ops.augment_piece_stats(tokens.cuda(), torch.from_numpy(off).cuda(), tab.cuda(), stats)
    assert torch.equal(stats.cpu(), want_stats)
    lens = torch.from_numpy(np.diff(off))
    out = torch.full((P, int(lens.max()), tok.max_token_seq), -5, dtype=torch.int64, device="cuda")
    ops.augment_collate_windows(tokens.cuda(), torch.from_numpy(off[:-1].copy()).cuda(), lens.cuda(), torch.arange(P).cuda(),
                                torch.from_numpy(g["shifts"]).cuda(), stats, tab.cuda(), out, tok.pad_id)
    out = out.cpu()
    for i in range(P):
        n = int(lens[i])
        assert np.array_equal(out[i, :n].numpy(), g["augmented"][off[i]:off[i + 1]].astype(np.int64)), (ver, i)
        assert (out[i, n:] == tok.pad_id).all()
    # (b) a sampler over a random corpus: 40 files of 200..3000 events, windows of up to 512, against the oracle per file
    import random
    from midi_model_amd.data import AUG_MAXIMA, synthetic_events
    rs = np.random.default_rng(5)
    pieces = []
    for i in range(40):
        ev = synthetic_events(tok, 1, int(rs.integers(200, 3000)), seed=300 + i, note_p=0.7)[0].numpy().astype(np.int16)
        if i % 3 == 0:  # narrow the pitch range so that some files do get augmented
            col = 1 + tok.events["note"].index("pitch")
            notes = ev[:, 0] == tok.event_ids["note"]
            ev[notes, col] = tok.parameter_ids["pitch"][0] + 20 + (ev[notes, col] - tok.parameter_ids["pitch"][0]) % 80
        pieces.append(ev)
    corpus = TokenCorpus(pieces, device="cuda")
    sampler = WindowSampler(corpus, max_len=512, rand_start=True, seed=21, aug=True, tokenizer=tok)
    idx = [int(x) for x in rs.integers(0, 40, 24)]
    got = sampler.batch(idx, pad_id=tok.pad_id).cpu()
    rng = random.Random(21)
    ref, n_aug = [], 0
    for i in idx:
        m = AUG_MAXIMA
        sh = [rng.randint(-m[0], m[0]), rng.randint(-m[1], m[1]), rng.randint(-m[2], m[2]), rng.randint(-m[3], m[3]),
              rng.randint(0, m[4]), rng.randint(0, m[5])]
        mid = orc.augment(tok, pieces[i], sh)
        n_aug += int((mid != pieces[i]).any())
        start = rng.randrange(0, max(1, mid.shape[0] - 512))
        start = rng.choice([0, start])
        ref.append(torch.from_numpy(mid[start:start + 512].astype(np.int64)))
    L = max(len(x) for x in ref)
    want = torch.stack([torch.nn.functional.pad(x, (0, 0, 0, L - x.shape[0]), value=tok.pad_id) for x in ref])
    assert torch.equal(got, want)
    assert 0 < n_aug < len(idx), n_aug
