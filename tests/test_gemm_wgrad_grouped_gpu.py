"""The grouped weight-gradient launch (mh_gemm_wgrad_grouped, gemm_pp256.hip) on the MI355X: several products over the same
contraction rows in ONE launch, every tile contracting the whole range, with the plain and the fold epilogue.  Operands, poisoned
buffers, fenced outputs and bounds are those of tests/ref_gemm.py; the backend is test_gemm_gpu.Hip.

  * exact operands (integers: every sum is exact in fp32 whatever its order): dW = the fp64 product rounded once, plain and
    with beta = 1 in place; fences intact; every problem bit-identical to mh_gemm(splitk = 1) on it alone;
  * the fold epilogue on exact operands: dW = rd(alpha G w + beta R), the per-tile-row column partials of alpha G W and the
    mh_colsum result are exact -- what check_reduce_fold of test_gemm_gpu.py demands of the split-K form;
  * Gaussian operands on the four layer shapes scaled down by 8: inside gauss_bound with the contraction length as the term
    count, two launches give identical bits.
The tile map of the same groups is checked on the host (tests/test_gemm_wgrad_grouped_host.py)."""
import ctypes

import pytest
import torch

import ref_gemm as G
from ref_gemm import BF16, F32, F64
from test_gemm_gpu import QA, QB, Hip, nan_input, new_out, to_dev

pytestmark = pytest.mark.gpu

# the outputs [N, K_out] of the exact family: one tile, two tile rows, three tile columns, ragged on both sides, below a tile
OUTS = [(256, 256), (512, 256), (256, 768), (300, 264), (40, 24)]
GROUPS = [(0,), (3,), (4,), (1, 4), (3, 2), (0, 1, 2, 3), (4, 3, 0, 1)]   # indices into OUTS: 1, 2 and 4 problems
KCS = [32, 96, 544, 2080]      # 1 and 3 K-steps (the pipeline's depth), 17 steps (not a multiple of 64), 65 steps
LAYER_DIV8 = [(1024, 128), (128, 512), (384, 128), (128, 128)]             # gate|up, down, q|k|v, o at D = 128, I = 512
LAYER_TILES = [(8192, 1024), (1024, 4096), (3072, 1024), (1024, 1024)]     # the benchmarked layer: 128 + 64 + 48 + 16 tiles


class Problem(ctypes.Structure):
    """mh_wgrad_problem of include/midihip.h"""
    _fields_ = [("dz", ctypes.c_void_p), ("lddz", ctypes.c_int64), ("x", ctypes.c_void_p), ("ldx", ctypes.c_int64),
                ("dw", ctypes.c_void_p), ("lddw", ctypes.c_int64), ("R", ctypes.c_void_p), ("ldr", ctypes.c_int64),
                ("N", ctypes.c_int64), ("K_out", ctypes.c_int64), ("alpha", ctypes.c_float), ("beta", ctypes.c_float),
                ("wnorm", ctypes.c_void_p), ("W", ctypes.c_void_p), ("ldw", ctypes.c_int64), ("colpart", ctypes.c_void_p)]


def problem(dz, x, dw, N, K_out, alpha=1.0, beta=0.0, R=None, wnorm=None, W=None, colpart=None):
    q = Problem()
    q.dz, q.lddz, q.x, q.ldx, q.dw, q.lddw = dz.data_ptr(), dz.stride(0), x.data_ptr(), x.stride(0), dw.data_ptr(), dw.stride(0)
    q.R, q.ldr = (R.data_ptr(), R.stride(0)) if R is not None else (None, 0)
    q.N, q.K_out, q.alpha, q.beta = N, K_out, alpha, beta
    if wnorm is not None:
        q.wnorm, q.W, q.ldw, q.colpart = wnorm.data_ptr(), W.data_ptr(), W.stride(0), colpart.data_ptr()
    return q


def launch(be, problems, Kc):
    arr = (Problem * len(problems))(*problems)
    be.call("mh_gemm_wgrad_grouped", arr, len(problems), Kc, 1)


@pytest.fixture(scope="module")
def be():
    return Hip()


_exact = {}


def exact_case(N, K_out, Kc):
    """operands, residual and references of one exact problem, made once: (A, B, dz, x, R, ref_plain, ref_acc)"""
    key = (N, K_out, Kc)
    if key not in _exact:
        seed = 100 + len(_exact)
        A, B = G.exact_operands(N, K_out, Kc, seed)
        P = G.exact_partials(A, B, [(0, Kc)])[0]
        q2 = QA * QB
        R = G.residual(N, K_out, seed + 2, 4 * q2)
        _exact[key] = (A, B, G.operand(A, QA, BF16, True, pad=8), G.operand(B, QB, BF16, True, pad=16), R,
                       G.exact_out(P, q2, BF16), G.exact_out(P, q2, BF16, 1.0, 1.0, R))
    return _exact[key]


@pytest.mark.parametrize("Kc", KCS)
@pytest.mark.parametrize("group", GROUPS)
def test_grouped_plain_bit_exact_and_equal_to_mh_gemm(be, group, Kc):
    """dW = the fp64 product rounded once (plain, and beta = 1 in place), fences intact, and the bits of mh_gemm(splitk = 1) on
    each problem alone"""
    cases = [(OUTS[i], exact_case(*OUTS[i], Kc)) for i in group]
    dev_ops = [(to_dev(dz, be.dev), to_dev(x, be.dev)) for _, (_, _, dz, x, _, _, _) in cases]
    for acc in (False, True):
        outs, probs = [], []
        for ((N, K_out), (A, B, _, _, R, ref0, ref1)), (dz, x) in zip(cases, dev_ops):
            cbuf, c = new_out(N, K_out, BF16, be.dev, init=R if acc else None)
            outs.append((cbuf, c))
            probs.append(problem(dz, x, c, N, K_out, 1.0, 1.0 if acc else 0.0, c if acc else None))
        launch(be, probs, Kc)
        for ((N, K_out), (A, B, _, _, R, ref0, ref1)), (dz, x), (cbuf, c) in zip(cases, dev_ops, outs):
            what = f"group {group} Kc={Kc} accumulate={acc}: problem {N}x{K_out}"
            msg = G.mismatch(c, ref1 if acc else ref0, A, B, QA * QB, add=R if acc else None)
            assert msg is None, f"{what}: {msg}"
            assert G.fence_ok(cbuf, N, K_out), f"{what}: written outside the [N, K_out] view"
            sbuf, s = new_out(N, K_out, BF16, be.dev, init=R if acc else None)
            be.gemm(dz, True, x, True, s, s if acc else None, N, K_out, Kc, 1.0, 1.0 if acc else 0.0, BF16, 1, None)
            assert torch.equal(c.view(torch.int16), s.view(torch.int16)), f"{what}: differs from mh_gemm(splitk=1) alone"


def fold_case(N, K_out, Kc, alpha, seed):
    """integer d z, x, W and w small enough that alpha G w + beta R and every column sum of alpha G W are fp32 values"""
    A, B = G.exact_operands(N, K_out, Kc, seed, cap=max(1, min(3, int((288 // Kc) ** 0.5))))
    Gs = alpha * (A @ B.T)
    g = torch.Generator().manual_seed(seed + 5)
    W = torch.randint(-127, 128, (N, K_out), generator=g).to(F64)
    w = (129 + 2 * torch.randint(0, 64, (K_out,), generator=g)).to(F64) * (1 - 2 * torch.randint(0, 2, (K_out,), generator=g))  # odd, 8 bits
    dw0 = torch.randint(-64, 65, (K_out,), generator=g).to(F64)
    assert float((Gs.abs() * W.abs()).sum(0).max()) + 64 < 2 ** 24 and float(Gs.abs().max()) * 255 + 127 < 2 ** 24
    assert G.wide_share(Gs * w[None, :]) >= 0.5
    return A, B, Gs, W, w, dw0


@pytest.mark.parametrize("N,K_out,Kc,alpha,acc", [(256, 264, 96, 1.0, False), (256, 40, 32, 1.0, True), (300, 264, 96, 0.5, False),
                                                  (300, 512, 544, 1.0, True), (520, 72, 96, 1.0, False), (520, 264, 32, 0.5, True)])
def test_grouped_fold_epilogue_exact(be, N, K_out, Kc, alpha, acc):
    """N on both sides of one and two tile-row blocks; the folded problem rides between two plain ones of another shape"""
    A, B, Gs, W, w, dw0 = fold_case(N, K_out, Kc, alpha, 31 + N + Kc)
    beta = 1.0 if acc else 0.0
    R = G.residual(N, K_out, 7, 1.0) if acc else None
    ref_W = G.exact_out(Gs * w[None, :], 1.0, BF16, 1.0, beta, R)
    dz, x = to_dev(G.operand(A, 1.0, BF16, True, pad=8), be.dev), to_dev(G.operand(B, 1.0, BF16, True, pad=16), be.dev)
    cbuf, c = new_out(N, K_out, BF16, be.dev, init=R)
    nblk = be._lib().cdll.mh_wgrad_grouped_fold_blocks(N)
    assert nblk == -(-N // 256)
    colpart = torch.full((nblk + 1, K_out), G.NAN, dtype=F32, device=be.dev)
    Wd, wd = to_dev(nan_input(W.to(BF16)), be.dev), w.to(BF16).to(be.dev)    # (named: a problem holds addresses, not tensors)
    folded = problem(dz, x, c, N, K_out, alpha, beta, c if acc else None, wd, Wd, colpart)
    (sN, sK), (sA, sB, sdz, sx, _, sref, _) = OUTS[4], exact_case(*OUTS[4], Kc)       # a plain neighbour on either side
    sdz, sx = to_dev(sdz, be.dev), to_dev(sx, be.dev)
    sides = []
    for _ in range(2):
        sbuf, s = new_out(sN, sK, BF16, be.dev)
        sides.append((sbuf, s, problem(sdz, sx, s, sN, sK)))
    launch(be, [sides[0][2], folded, sides[1][2]], Kc)
    what = f"fold {N}x{K_out} Kc={Kc} alpha={alpha} accumulate={acc}"
    msg = G.mismatch(c, ref_W, tile=(256, 256))
    assert msg is None, f"{what}: dW: {msg}"
    assert G.fence_ok(cbuf, N, K_out) and bool(torch.isnan(colpart[nblk]).all()), f"{what}: written outside dW or colpart"
    want_part = torch.zeros((nblk, K_out), dtype=F64).index_add_(0, torch.arange(N) // 256, Gs * W)
    msg = G.mismatch(colpart[:nblk], want_part, tile=(1, 256))
    assert msg is None, f"{what}: column partials: {msg}"
    cs = (Gs * W).sum(0) + (dw0 if acc else 0.0)
    for dt in (BF16, F32):
        out = dw0.to(dt).to(be.dev)
        be.colsum(colpart[:nblk].clone(), nblk, out, K_out, acc)
        msg = G.mismatch(out[None, :], G.rd(cs, dt)[None, :], tile=(1, 256))
        assert msg is None, f"{what}: colsum over {nblk} blocks -> {dt}: {msg}"
    for sbuf, s, _ in sides:
        assert G.mismatch(s, sref, sA, sB, QA * QB) is None and G.fence_ok(sbuf, sN, sK), f"{what}: the plain neighbour"


def test_grouped_gaussian_layer_shapes_bounded_and_repeatable(be):
    """The four layer shapes / 8 at contraction 4096, full-mantissa operands.  Plain problems (down, o): |dW - C64| inside
    gauss_bound with 4096 terms.  Folded problems (gate|up, q|k|v): dW = rd(fp32(G32 w)) with |G32 - C64| <= a terms, so
    |dW - C64 w| <= E |C64 w| + |w| a terms + 2^-23 |C64 w| + TINY (the fp32 multiply's own rounding, then the bf16 one).
    A second launch gives identical bits, column partials included."""
    Kc = 4096
    runs = []
    data = []
    for i, (N, K_out) in enumerate(LAYER_DIV8):
        A, B = G.gauss_operands(N, K_out, Kc, 70 + i)
        g = torch.Generator().manual_seed(80 + i)
        W, w = torch.randn((N, K_out), generator=g).to(BF16), (1.0 + 0.1 * torch.randn((K_out,), generator=g)).to(BF16)
        data.append((A, B, to_dev(G.operand(A, 1.0, BF16, True), be.dev), to_dev(G.operand(B, 1.0, BF16, True, pad=16), be.dev),
                     W.to(be.dev), w.to(be.dev), i in (0, 2)))
    for _ in range(2):
        outs, probs = [], []
        for (N, K_out), (A, B, dz, x, W, w, fold) in zip(LAYER_DIV8, data):
            cbuf, c = new_out(N, K_out, BF16, be.dev)
            colpart = torch.full((-(-N // 256), K_out), G.NAN, dtype=F32, device=be.dev) if fold else None
            outs.append((cbuf, c, colpart))
            probs.append(problem(dz, x, c, N, K_out, wnorm=w if fold else None, W=W if fold else None, colpart=colpart))
        launch(be, probs, Kc)
        torch.cuda.synchronize()
        runs.append(outs)
    for (N, K_out), (A, B, _, _, W, w, fold), (cbuf, c, colpart), (_, c2, colpart2) in zip(LAYER_DIV8, data, runs[0], runs[1]):
        C64, terms = G.gauss_ref(A, B)
        if fold:
            w64 = w.cpu().to(F64)[None, :]
            ref, bnd = C64 * w64, G.E[BF16] * (C64 * w64).abs() + w64.abs() * G.a_gemm() * terms + 2.0 ** -23 * (C64 * w64).abs() + G.TINY
            assert torch.equal(colpart.view(torch.int32), colpart2.view(torch.int32)), f"{N}x{K_out}: column partials differ between two launches"
            cp64, cterms = (C64 * W.cpu().to(F64)), (terms * W.cpu().to(F64).abs())
            blk = torch.arange(N) // 256
            want = torch.zeros((colpart.shape[0], K_out), dtype=F64).index_add_(0, blk, cp64)
            wterms = torch.zeros((colpart.shape[0], K_out), dtype=F64).index_add_(0, blk, cterms)
            # every fp32 addition of a chain of n terms errs by at most 2^-24 of the running sum: n 2^-24 sum |terms| covers product,
            # multiply and the 256-row chain
            msg = G.out_of_bound(colpart, want, (G.a_gemm() + (256 + 2) * 2.0 ** -24) * wterms + G.TINY)
            assert msg is None, f"{N}x{K_out}: column partials: {msg}"
        else:
            ref, bnd = C64, G.gauss_bound(C64, terms, BF16)
        msg = G.out_of_bound(c, ref, bnd)
        assert msg is None, f"{N}x{K_out} fold={fold}: {msg}"
        assert G.fence_ok(cbuf, N, K_out)
        assert torch.equal(c.view(torch.int16), c2.view(torch.int16)), f"{N}x{K_out}: two launches differ"
