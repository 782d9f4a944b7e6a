"""The GEMM family on the MI355X at its tile, K-loop and split-K edges (gemm_pp256.hip, gemm.hip, gemm_skinny.hip), against the exact
operand family of tests/ref_gemm.py: integer operands for which every correct kernel must return the same bits, in poisoned
operand buffers and fenced output views.  Shapes come from the launchers: K by the depth of both main loops (K-step 32: three
steps in flight; K-step 64: the steady part from the third tile), M / N by the wave tile (128 x 64) and the block tile
(256 x 256), tile counts by the XCD remap and the four-row grouping of the tile order, split-K by its slicing.  The epilogue
arithmetic of the fused entry points is held to the float64 bounds of tests/ref_streamers.py applied to the exact product.

Every check is a function of a backend (`Hip` below: the C-ABI on the device).  tests/test_gemm_bounds_host.py runs the same
checks on the CPU against a torch restatement and against named wrong kernels.

Not covered: leading dimensions of 2^22 elements and more (the lean epilogue's fallback to the general form): one such case needs
a 2 GiB buffer.  The ablation builds (option gemm_ablate != 0) are wrong by design."""
import contextlib

import pytest
import torch

import ref_gemm as G
from ref_gemm import BF16, F32, F64
from ref_streamers import RMS_EPS, randu, rstd_ref, swiglu_inputs

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------- the backend
class Hip:
    """the C-ABI of libmidihip.so on the device, every argument spelled out (no defaults of midi_model_amd.ops in between)"""
    dev = "cuda"

    def __init__(self):
        import midi_model_amd.ops as ops
        from midi_model_amd.lib import lib
        self.ops, self._lib = ops, lib

    def call(self, name, *args):
        self._lib().call(name, *args, torch.cuda.current_stream().cuda_stream)

    def set_option(self, name, value):
        self.ops.set_option(name, value)

    def get_option(self, name):
        return self.ops.get_option(name)

    @staticmethod
    def p(t):
        return None if t is None else t.data_ptr()

    @staticmethod
    def ld(t):
        return 0 if t is None else t.stride(0)

    @staticmethod
    def dt(dtype):
        return 1 if dtype == BF16 else 0

    def gemm(self, a, ta, b, tb, c, r, M, N, K, alpha, beta, dtype, splitk, ws):
        p, ld = self.p, self.ld
        self.call("mh_gemm", p(a), ld(a), int(ta), p(b), ld(b), int(tb), p(c), ld(c), p(r), ld(r), M, N, K, alpha, beta, self.dt(dtype), splitk, p(ws))

    def splitk_reduce(self, ws, c, r, M, N, splitk, alpha, beta, dtype):
        self.call("mh_gemm_splitk_reduce", self.p(ws), self.p(c), self.ld(c), self.p(r), self.ld(r), M, N, splitk, alpha, beta, self.dt(dtype))

    def fold_blocks(self, M):
        return self._lib().cdll.mh_splitk_fold_blocks(M)

    def splitk_reduce_fold(self, ws, c, r, M, N, splitk, alpha, beta, wnorm, W, colpart):
        p, ld = self.p, self.ld
        self.call("mh_gemm_splitk_reduce_fold", p(ws), p(c), ld(c), p(r), ld(r), M, N, splitk, alpha, beta, p(wnorm), p(W), ld(W), p(colpart), 1)

    def colsum(self, colpart, nblk, out, D, accumulate):
        self.call("mh_colsum", self.p(colpart), nblk, self.p(out), D, int(accumulate), self.dt(out.dtype))

    def gemm_swiglu(self, a, w, gu, act, M, I, K, rowscale=None):
        p, ld = self.p, self.ld
        if rowscale is None:
            self.call("mh_gemm_swiglu", p(a), ld(a), p(w), ld(w), p(gu), ld(gu), p(act), ld(act), M, I, K, 1)
        else:
            self.call("mh_gemm_swiglu_scaled", p(a), ld(a), p(w), ld(w), p(gu), ld(gu), p(act), ld(act), p(rowscale), M, I, K, 1)

    def gemm_rope(self, a, w, c, table, npos, S, pos0, M, N, K, rowscale=None):
        p, ld = self.p, self.ld
        if rowscale is None:
            self.call("mh_gemm_rope", p(a), ld(a), p(w), ld(w), p(c), ld(c), p(table), npos, S, pos0, 64, M, N, K, 1)
        else:
            self.call("mh_gemm_rope_scaled", p(a), ld(a), p(w), ld(w), p(c), ld(c), p(table), npos, S, pos0, 64, p(rowscale), M, N, K, 1)

    def gemm_dswiglu(self, a, b, gu, dgu, M, I, K, rowscale=None):
        p, ld = self.p, self.ld
        if rowscale is None:
            self.call("mh_gemm_dswiglu", p(a), ld(a), p(b), ld(b), p(gu), ld(gu), p(dgu), ld(dgu), M, I, K, 1)
        else:
            self.call("mh_gemm_dswiglu_scaled", p(a), ld(a), p(b), ld(b), p(gu), ld(gu), p(dgu), ld(dgu), p(rowscale), M, I, K, 1)

    def gemm_rowss(self, a, b, c, r, rowss, M, N, K):
        p, ld = self.p, self.ld
        self.call("mh_gemm_rowss", p(a), ld(a), p(b), ld(b), p(c), ld(c), p(r), ld(r), p(rowss), M, N, K, 1)

    def row_rstd(self, x, parts, nparts, M, D, eps, rstd):
        self.call("mh_row_rstd", self.p(x), self.ld(x), self.p(parts), nparts, M, D, eps, self.p(rstd), 1)

    def gemm_nt_scaled(self, a, b, c, rowscale, M, N, K):
        p, ld = self.p, self.ld
        self.call("mh_gemm_nt_scaled", p(a), ld(a), p(b), ld(b), p(c), ld(c), p(rowscale), M, N, K, 1)

    def gemm_skinny(self, a, w, c, r, mode, eps, row_ids, res_ids, M, N, K):
        p, ld = self.p, self.ld
        self.call("mh_gemm_skinny", p(a), ld(a), p(w), ld(w), p(c), ld(c), p(r), ld(r), mode, eps, p(row_ids), p(res_ids), M, N, K, 1)


@pytest.fixture(scope="module")
def be():
    return Hip()


def to_dev(view, dev):
    """a view of a poisoned buffer -> the same view of the buffer's copy on `dev` (the padding travels with it)"""
    base = view._base if view._base is not None else view
    return base.to(dev)[: view.shape[0], : view.shape[1]] if view.dim() == 2 else base.to(dev)


def new_out(M, N, dtype, dev, ldc=None, init=None):
    buf, _ = G.out_view(M, N, dtype, ldc, init)
    buf = buf.to(dev)
    return buf, buf[:M, :N]


def nan_input(x, pad=8):
    """an input matrix (a residual, gate|up) in a buffer wider than its rows, NaN in the padding"""
    buf = torch.full((x.shape[0] + 1, G.up(x.shape[1], 8) + pad), G.NAN, dtype=x.dtype)
    buf[: x.shape[0], : x.shape[1]] = x
    return buf[: x.shape[0], : x.shape[1]]


@contextlib.contextmanager
def options(be, **kw):
    """set runtime options for the block and put back the values found before it"""
    found = {k: be.get_option(k) for k in kw}
    try:
        for k, v in kw.items():
            be.set_option(k, v)
        yield
    finally:
        for k, v in found.items():
            be.set_option(k, v)


# ------------------------------------------------------------------------------------------------------------------ mh_gemm
def kstep_of(ta, tb, k64, dtype=BF16, variant=1):
    """the K-step of the main loop the launcher picks: slices of a split-K launch are whole steps"""
    if dtype == F32:
        return 32
    if variant == 0:
        return 64
    return 64 if (not ta and ((not tb and k64 != 0) or (tb and k64 == 1))) else 32


QA, QB = 0.25, 0.5     # operand units of the plain products (q^2 = 2^-3)


def check_gemm(be, M, N, K, ta, tb, splitk=1, alpha=1.0, beta=0.0, rmode=None, dtype=BF16, variants=((1, 1),), gemm=1, seed=1, tile=(256, 256)):
    """one product at every (gemm_k64, gemm_lean_epi) of `variants`: bits equal to the exact reference (and so to each other),
    split-K partials equal to the exact slice products, nothing written outside the view"""
    A, B = G.exact_operands(M, N, K, seed)
    q2 = QA * QB
    a, b = to_dev(G.operand(A, QA, dtype, ta, pad=8), be.dev), to_dev(G.operand(B, QB, dtype, tb, pad=16), be.dev)
    R = G.residual(M, N, seed + 2, 4 * q2) if beta != 0.0 else None
    refs = {}
    for k64, lean in variants:
        step = kstep_of(ta, tb, k64, dtype, gemm)
        what = f"{M}x{N}x{K} ta={int(ta)} tb={int(tb)} splitk={splitk} gemm_k64={k64} lean={lean}"
        if step not in refs:
            slices = G.splitk_slices(K, splitk, step)
            parts = G.exact_partials(A, B, slices)
            refs[step] = (slices, parts, G.exact_out(sum(parts), q2, dtype, alpha, beta, R))
        slices, parts, ref = refs[step]
        cbuf, c = new_out(M, N, dtype, be.dev, init=R if rmode == "inplace" else None)
        r = c if rmode == "inplace" else (to_dev(nan_input(R.to(dtype), pad=24), be.dev) if rmode == "separate" else None)
        with options(be, gemm_k64=k64, gemm_lean_epi=lean):
            if splitk == 1:
                be.gemm(a, ta, b, tb, c, r, M, N, K, alpha, beta, dtype, 1, None)
            else:
                ws = torch.full((splitk, M, N), G.NAN, dtype=F32, device=be.dev)
                be.gemm(a, ta, b, tb, c, r, M, N, K, alpha, beta, dtype, splitk, ws)
                for z, (lo, hi) in enumerate(slices):   # (an empty trailing slice stores zeros)
                    msg = G.mismatch(ws[z], q2 * parts[z], A[:, lo:hi], B[:, lo:hi], q2, tile)
                    assert msg is None, f"{what}: partial of slice {z} (k {lo}..{hi}): {msg}"
                be.splitk_reduce(ws, c, r, M, N, splitk, alpha, beta, dtype)
        msg = G.mismatch(c, ref, A, B, q2 * alpha, tile, add=None if R is None else beta * R)
        assert msg is None, f"{what}: {msg}"
        assert G.fence_ok(cbuf, M, N), f"{what}: written outside the [M, N] view"


ALL_VARIANTS = tuple((k64, lean) for k64 in (0, 1, 2) for lean in (0, 1))
NN, NT, TN, TT = (False, False), (False, True), (True, False), (True, True)
LONG_K = 4168    # 65 K-steps of 64 + 8
# (M, N, K, layout): a cross of the M / N edges with the K classes of both loops -- ceil(K / 32) in {1, 2, 3, 4, 5, 7},
# ceil(K / 64) in {1, 2, 3, 4, 6} with tails 8, 24, 32, 40, 56 -- every case at all six option values
GEMM_EDGES = [
    (1, 8, 8, NN), (127, 64, 40, NN), (128, 72, 72, NN), (129, 200, 104, NN), (255, 256, 136, NN), (256, 264, 200, NN),
    (257, 250, 88, NN), (513, 3406, 160, NN), (1, 3406, 232, NN), (513, 8, 376, NN), (257, 264, 64, NN), (129, 250, LONG_K, NN),
    (1, 8, 1, NT), (127, 64, 7, NT), (128, 72, 33, NT), (129, 200, 100, NT), (255, 256, 333, NT), (256, 264, 8, NT),
    (257, 64, 40, NT), (513, 200, 88, NT), (127, 8, 376, NT), (129, 72, 232, NT), (255, 264, 160, NT), (1, 256, LONG_K + 3, NT),
    (128, 250, 33, TN), (256, 3406, 7, TN), (8, 8, 1, TN), (264, 72, 100, TN), (520, 200, 333, TN), (128, 64, LONG_K + 3, TN),
    (128, 64, 1, TT), (256, 264, 100, TT), (8, 200, 333, TT), (520, 8, 7, TT), (264, 256, LONG_K, TT), (128, 72, 33, TT),
]


def case_ids(cases):
    """M x N x K - operand layouts (r: row-major, t: contraction-major) - the rest"""
    def word(v):
        return "".join("rt"[int(t)] for t in v) if isinstance(v, tuple) else str(v)
    return ["-".join(["x".join(str(d) for d in c[:3])] + [word(v) for v in c[3:]]) for c in cases]


@pytest.mark.parametrize("M,N,K,layout", GEMM_EDGES, ids=case_ids(GEMM_EDGES))
def test_gemm_edges_bit_exact_under_every_option(be, M, N, K, layout):
    """option gemm_k64 in {0, 1, 2} x gemm_lean_epi in {0, 1}: identical bits, the exact ones"""
    check_gemm(be, M, N, K, *layout, variants=ALL_VARIANTS)


# (M, N, K, layout, splitk, alpha, beta, R): the M / N edges again, with split-K on both loops: a short last slice, a trailing
# empty slice (K = 100 in three slices of the K-step-64 loop), as many slices as K-steps and more, slices of one and two steps
GEMM_SPLITK = [
    (129, 200, 100, NT, 3, 1.0, 0.0, None), (257, 250, 200, NN, 2, 1.0, 0.0, None), (256, 264, 200, NN, 7, 0.75, 0.5, "inplace"),
    (255, 256, 200, NN, 9, 1.0, 0.0, None), (513, 8, 200, NN, 4, 1.0, 1.0, "inplace"), (1, 3406, 136, NN, 3, 0.5, 0.0, None),
    (127, 64, 8, NN, 2, 1.0, 0.0, None), (128, 72, 104, NN, 2, 2.0, 0.5, "separate"), (513, 3406, 72, NN, 2, 1.0, 0.0, None),
    (1, 8, 376, NT, 5, 1.0, 0.0, None), (127, 64, 333, NT, 3, 1.0, 0.0, None), (128, 72, 232, NT, 2, 0.75, 0.0, None),
    (255, 256, 160, NT, 3, 1.0, 0.5, "separate"), (256, 264, 88, NT, 2, 1.0, 0.0, None), (257, 200, LONG_K, NT, 5, 1.0, 1.0, "inplace"),
    (513, 200, 104, NT, 4, 1.0, 0.0, None),
    (128, 250, 100, TN, 3, 1.0, 0.0, None), (264, 3406, 72, TN, 2, 1.0, 0.5, "inplace"), (520, 200, 333, TN, 11, 1.0, 0.0, None),
    (256, 264, 100, TT, 3, 0.75, 0.0, None), (520, 8, 200, TT, 7, 1.0, 0.0, None), (264, 256, LONG_K, TT, 6, 1.0, 1.0, "separate"),
]


@pytest.mark.parametrize("M,N,K,layout,splitk,alpha,beta,rmode", GEMM_SPLITK, ids=case_ids(GEMM_SPLITK))
def test_gemm_splitk_partials_and_result_bit_exact(be, M, N, K, layout, splitk, alpha, beta, rmode):
    check_gemm(be, M, N, K, *layout, splitk=splitk, alpha=alpha, beta=beta, rmode=rmode, variants=((0, 1), (1, 1), (1, 0)), seed=5)


@pytest.mark.parametrize("alpha,beta,rmode", [(0.75, 0.0, None), (1.0, 1.0, "inplace"), (0.5, 0.5, "separate"), (2.0, 1.0, "separate")])
@pytest.mark.parametrize("M,N,K,layout", [(257, 250, 72, NN), (300, 264, 40, NT), (264, 250, 100, TN)])
def test_gemm_alpha_beta_residual_unsplit(be, M, N, K, layout, alpha, beta, rmode):
    """R = NULL, R = C in place, R separate with ldr != ldc, on the ragged (general) and the interior (lean) epilogue"""
    check_gemm(be, M, N, K, *layout, alpha=alpha, beta=beta, rmode=rmode, variants=((0, 1), (1, 1), (1, 0)), seed=7)


# work items nwg * splitk in {1, 7, 8, 9, 15, 17} and beyond, tiles_m in {1, 3, 4, 5}: the last group of the tile order's
# four-row grouping has 1, 3 and 4 rows; a tile never written is NaN, a tile written to another place breaks bits or fence
TILE_ORDER = [(100, 100, 64, 1), (100, 1600, 64, 1), (1000, 300, 64, 1), (600, 600, 64, 1), (1100, 600, 64, 1), (1100, 600, 64, 3),
              (100, 4200, 64, 1), (100, 100, 544, 17), (1000, 300, 96, 2), (700, 1030, 40, 1), (1281, 257, 64, 1)]


@pytest.mark.parametrize("layout", [NN, NT], ids=["rr", "rt"])
@pytest.mark.parametrize("M,N,K,splitk", TILE_ORDER)
def test_gemm_tile_order(be, M, N, K, splitk, layout):
    if layout == NT:
        N = G.up(N, 8)
    check_gemm(be, M, N, K, *layout, splitk=splitk, variants=((0, 1), (1, 1)), seed=9)


# ---------------------------------------------------------------------------------- the 128x128 kernel of gemm.hip (option gemm = 0)
# fp32: BK = 32 floats, two stages; K in {4, 32, 36, 64, 68, 96, 100, 132, 4100}, M / N around its 128-tile, N % 4 != 0 (scalar stores)
GEMM128_F32 = [(1, 8, 4, 1), (127, 64, 32, 1), (128, 72, 36, 1), (129, 129, 64, 1), (257, 250, 68, 2), (255, 127, 96, 3), (128, 128, 100, 4),
               (385, 264, 132, 2), (130, 200, 4100, 5), (513, 520, 64, 1)]


@pytest.mark.parametrize("M,N,K,splitk", GEMM128_F32)
def test_gemm128_fp32_bit_exact(be, M, N, K, splitk):
    for alpha, beta, rmode in ((1.0, 0.0, None), (0.75, 0.5, "inplace")):
        check_gemm(be, M, N, K, False, False, splitk=splitk, alpha=alpha, beta=beta, rmode=rmode, dtype=F32, tile=(128, 128), seed=11)


@pytest.mark.parametrize("layout", [NN, NT, TN, TT], ids=["rr", "rt", "tr", "tt"])
@pytest.mark.parametrize("M,N,K,splitk", [(128, 128, 64, 1), (136, 264, 72, 1), (264, 136, 200, 3), (520, 72, 333, 2), (8, 8, LONG_K, 4)])
def test_gemm128_bf16_bit_exact(be, M, N, K, splitk, layout):
    """the bf16 instantiations of the 128x128 kernel (BK = 64), which only the A/B library holds"""
    if K % 8 and layout == NN:
        K = G.up(K, 8)
    with be.ops.ab_library(), options(be, gemm=0):
        check_gemm(be, M, N, K, *layout, splitk=splitk, gemm=0, tile=(128, 128), seed=13)


# ------------------------------------------------------------------------------------------------- mh_gemm_splitk_reduce alone
def check_reduce(be, M, N, splitk, alpha, beta, rmode, dtype=BF16, ldc=None, seed=3):
    """a synthetic integer workspace: C = rd(alpha sum_z ws[z] + beta R), every step an fp32 value"""
    g = torch.Generator().manual_seed(seed)
    ws = torch.randint(-2 ** 17, 2 ** 17, (splitk, M, N), generator=g).to(F64)
    q2 = 2.0 ** -6
    R = G.residual(M, N, seed + 1, 4 * q2) if beta != 0.0 else None
    ref = G.exact_out(ws.sum(0), q2, dtype, alpha, beta, R)
    cbuf, c = new_out(M, N, dtype, be.dev, ldc=ldc, init=R if rmode == "inplace" else None)
    r = c if rmode == "inplace" else (to_dev(nan_input(R.to(dtype), pad=24), be.dev) if rmode == "separate" else None)
    be.splitk_reduce((ws * q2).to(F32).to(be.dev), c, r, M, N, splitk, alpha, beta, dtype)
    msg = G.mismatch(c, ref, tile=(1, 1024))
    assert msg is None, f"splitk_reduce {M}x{N} splitk={splitk}: {msg}"
    assert G.fence_ok(cbuf, M, N)


@pytest.mark.parametrize("M,N,splitk,alpha,beta,rmode,ldc", [
    (2047, 8, 2, 1.0, 0.0, None, None), (2048, 12, 3, 0.75, 0.5, "inplace", None), (2049, 8, 9, 1.0, 1.0, "separate", None),   # vector form, its row grid cap
    (5, 1028, 8, 1.0, 0.0, None, None), (3, 2052, 2, 0.5, 0.0, None, None),                                        # a second column block
    (2050, 514, 2, 1.0, 0.5, "inplace", None), (2050, 514, 3, 0.75, 0.0, None, None),                               # scalar form (N % 4 != 0) past 4096 blocks
    (33, 40, 4, 1.0, 1.0, "separate", 42), (1, 1, 1, 2.0, 0.0, None, None)])                                           # scalar form by ldc % 4 != 0
def test_splitk_reduce_alone(be, M, N, splitk, alpha, beta, rmode, ldc):
    check_reduce(be, M, N, splitk, alpha, beta, rmode, ldc=ldc)


def test_splitk_reduce_alone_fp32(be):
    check_reduce(be, 300, 37, 3, 0.75, 0.5, "inplace", dtype=F32)
    check_reduce(be, 4100, 260, 2, 1.0, 0.0, None, dtype=F32)


# ------------------------------------------------------------------------------- mh_gemm_splitk_reduce_fold with mh_colsum
def check_reduce_fold(be, M, N, splitk, alpha, beta, accumulate, seed=17):
    """integer partials, W and w: dW = rd(alpha G w + beta R) and dw = rd(colsum(alpha G W) (+ dw)) are exact"""
    g = torch.Generator().manual_seed(seed)
    ws = torch.randint(-20, 21, (splitk, M, N), generator=g).to(F64)
    W = torch.randint(-127, 128, (M, N), generator=g).to(F64)
    w = (129 + 2 * torch.randint(0, 64, (N,), generator=g)).to(F64) * (1 - 2 * torch.randint(0, 2, (N,), generator=g))   # odd, 8 bits: G w needs more
    R = G.residual(M, N, seed + 1, 1.0) if beta != 0.0 else None
    dw0 = torch.randint(-64, 65, (N,), generator=g).to(F64)
    Gs = alpha * ws.sum(0)
    assert float((Gs.abs() * W.abs()).sum(0).max()) + 64 < 2 ** 24
    ref_W = G.exact_out(Gs * w[None, :], 1.0, BF16, 1.0, beta, R)
    cs = (Gs * W).sum(0) + (dw0 if accumulate else 0.0)
    cbuf, c = new_out(M, N, BF16, be.dev, init=R)
    nblk = be.fold_blocks(M)
    assert nblk == min(M, 1024)
    colpart = torch.full((nblk + 1, N), G.NAN, dtype=F32, device=be.dev)
    be.splitk_reduce_fold(ws.to(F32).to(be.dev), c, c if R is not None else None, M, N, splitk, alpha, beta, w.to(BF16).to(be.dev),
                          to_dev(nan_input(W.to(BF16)), be.dev), colpart)
    msg = G.mismatch(c, ref_W, tile=(1, 1024))
    assert msg is None, f"splitk_reduce_fold {M}x{N}: dW: {msg}"
    assert G.fence_ok(cbuf, M, N) and bool(torch.isnan(colpart[nblk]).all())
    rows = torch.arange(M) % nblk
    want_part = torch.zeros((nblk, N), dtype=F64).index_add_(0, rows, Gs * W)
    msg = G.mismatch(colpart[:nblk], want_part, tile=(1, 1024))
    assert msg is None, f"splitk_reduce_fold {M}x{N}: column partials: {msg}"
    for dt in (BF16, F32):
        out = dw0.to(dt).to(be.dev)
        be.colsum(colpart[:nblk].clone(), nblk, out, N, accumulate)
        msg = G.mismatch(out[None, :], G.rd(cs, dt)[None, :], tile=(1, 1024))
        assert msg is None, f"colsum over {nblk} blocks -> {dt}: {msg}"


@pytest.mark.parametrize("M,N,splitk,alpha,beta,acc", [(1023, 40, 2, 1.0, 0.0, False), (1024, 44, 3, 1.0, 1.0, True), (1025, 40, 2, 0.5, 0.0, False),
                                                       (2500, 1028, 2, 1.0, 1.0, True), (7, 4, 9, 1.0, 0.0, False)])
def test_splitk_reduce_fold_and_colsum(be, M, N, splitk, alpha, beta, acc):
    """M on both sides of mh_splitk_fold_blocks' cap (1024)"""
    check_reduce_fold(be, M, N, splitk, alpha, beta, acc)


# ------------------------------------------------------------------------------------------------------ fused entry points
FUSED_K = [8, 64, 72, 264, LONG_K]


def rowscale_of(M, seed, dev):
    """any fp32 values: the scaled product rd(fp32(rowscale[m] P)) is one correctly rounded multiply of an exact P"""
    rs = randu((M,), seed, 0.5, 1.0).to(F32)
    return rs.to(F64), rs.to(dev)


def scaled_product(P, q2, rs64, dtype=BF16):
    x = q2 * P
    assert G.is_f32(x)
    return G.rd(rs64[:, None] * x, dtype) if rs64 is not None else G.exact_out(P, q2, dtype)


def check_swiglu(be, M, I, K, k64=1, with_gu=True, scaled=False, seed=21):
    A, W = G.exact_operands(M, 2 * I, K, seed)
    P = G.exact_partials(A, W, [(0, K)])[0]
    q2 = G.scale_to(P[:, :I], 8.0)                 # gates in [-8, 8]: not in saturation
    rs64, rs = rowscale_of(M, seed + 2, be.dev) if scaled else (None, None)
    gu_ref = scaled_product(P, q2, rs64)
    assert float(gu_ref[:, :I].abs().max()) <= 8.0 and G.wide_share(q2 * P) >= 0.5
    gu_t = gu_ref.to(BF16)
    act_ref, terms = G.swiglu_fwd_ref(gu_t, BF16)
    a, w = to_dev(G.operand(A, q2, BF16, False), be.dev), to_dev(G.operand(W, 1.0, BF16, False, pad=16), be.dev)
    gbuf, gu = new_out(M, 2 * I, BF16, be.dev)
    abuf, act = new_out(M, I, BF16, be.dev, ldc=I + 24)
    what = f"gemm_swiglu {M}x{I}x{K} k64={k64} gu={with_gu} scaled={scaled}"
    with options(be, gemm_k64=k64):
        be.gemm_swiglu(a, w, gu if with_gu else None, act, M, I, K, rs)
    if with_gu:
        msg = G.mismatch(gu, gu_ref, A, W, q2)
        assert msg is None, f"{what}: gate|up: {msg}"
    else:
        assert bool(torch.isnan(gu).all()), f"{what}: gate|up written in the forward-only form"
    msg = G.out_of_bound(act, act_ref, G.swiglu_fwd_bound(terms, gu_t, BF16))
    assert msg is None, f"{what}: activation: {msg}"
    assert G.fence_ok(gbuf, M, 2 * I) and G.fence_ok(abuf, M, I), f"{what}: written outside the views"


@pytest.mark.parametrize("k64", [0, 1], ids=["k32", "k64"])
@pytest.mark.parametrize("M,I,K,with_gu", [(77, 128, 8, True), (257, 128, 64, True), (257, 256, 72, False), (300, 384, 264, True), (77, 128, LONG_K, True),
                                           (256, 256, 264, False)])
def test_gemm_swiglu(be, k64, M, I, K, with_gu):
    check_swiglu(be, M, I, K, k64, with_gu)


@pytest.mark.parametrize("M,I,K,with_gu", [(260, 128, 8, True), (516, 256, 72, True), (260, 384, 264, False), (516, 128, LONG_K, True)])
def test_gemm_swiglu_scaled(be, M, I, K, with_gu):
    check_swiglu(be, M, I, K, 1, with_gu, scaled=True)


def check_rope(be, M, H, K, S, pos0, k64=1, scaled=False, seed=31):
    N = 3 * H * 64
    A, W = G.exact_operands(M, N, K, seed)
    P = G.exact_partials(A, W, [(0, K)])[0]
    q2 = G.scale_to(P, 4.0)
    rs64, rs = rowscale_of(M, seed + 2, be.dev) if scaled else (None, None)
    c_ref = scaled_product(P, q2, rs64)
    npos = pos0 + min(S, M)                          # the table is exactly as long as the header asks
    cos_t, sin_t = G.rope_tables(64, npos)
    ref, terms = G.rope_ref(c_ref.to(BF16), cos_t, sin_t, S, pos0, H, 64, +1, BF16)
    a, w = to_dev(G.operand(A, q2, BF16, False), be.dev), to_dev(G.operand(W, 1.0, BF16, False, pad=16), be.dev)
    cbuf, c = new_out(M, N, BF16, be.dev)
    what = f"gemm_rope {M}x{N}x{K} S={S} pos0={pos0} k64={k64} scaled={scaled}"
    with options(be, gemm_k64=k64):
        be.gemm_rope(a, w, c, G.rope_fused_table(cos_t, sin_t, npos).to(be.dev), npos, S, pos0, M, N, K, rs)
    msg = G.mismatch(c[:, 2 * H * 64:], c_ref[:, 2 * H * 64:], A, W[2 * H * 64:], q2)
    assert msg is None, f"{what}: v: {msg}"
    msg = G.out_of_bound(c, ref, G.rope_bound(terms, BF16))
    assert msg is None, f"{what}: rotated q|k: {msg}"
    assert G.fence_ok(cbuf, M, N), f"{what}: written outside the view"


# (M, H, K, S, pos0): pos0 > 0, S = 1, S that does not divide 256 (100 with M = 300), S >= M, the smallest width N = 192
ROPE_CASES = [(77, 1, 8, 77, 0), (257, 1, 64, 100, 5), (300, 2, 72, 100, 3), (257, 2, 264, 1, 7), (77, 1, LONG_K, 500, 11), (300, 1, 64, 300, 1), (256, 2, 72, 64, 0)]


@pytest.mark.parametrize("k64", [0, 1], ids=["k32", "k64"])
@pytest.mark.parametrize("M,H,K,S,pos0", ROPE_CASES)
def test_gemm_rope(be, k64, M, H, K, S, pos0):
    check_rope(be, M, H, K, S, pos0, k64)


@pytest.mark.parametrize("M,H,K,S,pos0", [(260, 1, 8, 100, 5), (516, 2, 72, 1, 3), (260, 2, 264, 1000, 9), (516, 1, LONG_K, 129, 0)])
def test_gemm_rope_scaled(be, M, H, K, S, pos0):
    check_rope(be, M, H, K, S, pos0, 1, scaled=True)


def check_dswiglu(be, M, I, K, k64=1, scaled=False, seed=41):
    A, B = G.exact_operands(M, I, K, seed)
    P = G.exact_partials(A, B, [(0, K)])[0]
    q2 = G.scale_to(P, 4.0)
    rs64, rs = rowscale_of(M, seed + 2, be.dev) if scaled else (None, None)
    da = scaled_product(P, q2, rs64).to(BF16)       # d a is exact: the product, rounded once
    gu = swiglu_inputs(M, I, BF16, seed + 3)[0]
    ref, terms = G.swiglu_bwd_ref(gu, da)
    bnd = G.swiglu_bwd_bound(terms, gu, BF16)
    a, b = to_dev(G.operand(A, q2, BF16, False), be.dev), to_dev(G.operand(B, 1.0, BF16, True, pad=16), be.dev)
    gud = to_dev(nan_input(gu), be.dev)
    outs = []
    for lean in (1, 0):
        what = f"gemm_dswiglu {M}x{I}x{K} k64={k64} lean={lean} scaled={scaled}"
        dbuf, dgu = new_out(M, 2 * I, BF16, be.dev, ldc=2 * I + 24)
        with options(be, gemm_k64=k64, gemm_lean_epi=lean):
            be.gemm_dswiglu(a, b, gud, dgu, M, I, K, rs)
        msg = G.out_of_bound(dgu, ref, bnd)
        assert msg is None, f"{what}: {msg}"
        assert G.fence_ok(dbuf, M, 2 * I), f"{what}: written outside the view"
        outs.append(dgu)
    assert torch.equal(outs[0], outs[1]), f"gemm_dswiglu {M}x{I}x{K}: gemm_lean_epi 0 and 1 differ"


# I = 520: the general epilogue's n + 8 <= N edge and the lean form in one launch
@pytest.mark.parametrize("k64", [0, 1], ids=["k32", "k64"])
@pytest.mark.parametrize("M,I,K", [(77, 8, 8), (257, 64, 64), (257, 520, 72), (300, 264, 264), (77, 520, LONG_K), (256, 256, 33)])
def test_gemm_dswiglu(be, k64, M, I, K):
    check_dswiglu(be, M, I, K, k64)


@pytest.mark.parametrize("M,I,K", [(260, 64, 8), (516, 520, 72), (260, 264, 264), (516, 64, LONG_K)])
def test_gemm_dswiglu_scaled(be, M, I, K):
    check_dswiglu(be, M, I, K, 1, scaled=True)


def check_nt_scaled(be, M, N, K, seed=51):
    A, B = G.exact_operands(M, N, K, seed)
    P = G.exact_partials(A, B, [(0, K)])[0]
    rs64, rs = rowscale_of(M, seed + 2, be.dev)
    q2 = QA * QB
    ref = scaled_product(P, q2, rs64)
    a, b = to_dev(G.operand(A, QA, BF16, False), be.dev), to_dev(G.operand(B, QB, BF16, False, pad=16), be.dev)
    for ldc in (None, N + 3):
        cbuf, c = new_out(M, N, BF16, be.dev, ldc=ldc)
        be.gemm_nt_scaled(a, b, c, rs, M, N, K)
        msg = G.mismatch(c, ref, A, B, q2)
        assert msg is None, f"gemm_nt_scaled {M}x{N}x{K} ldc={ldc}: {msg}"
        assert G.fence_ok(cbuf, M, N)


@pytest.mark.parametrize("M,N,K", [(260, 64, 8), (516, 264, 64), (260, 250, 72), (516, 64, 264), (260, 520, LONG_K)])
def test_gemm_nt_scaled(be, M, N, K):
    check_nt_scaled(be, M, N, K)


def check_rowss(be, M, N, K, res, exact_ss, seed=61):
    """exact_ss: operands chosen so that the stored values are integers below 512 (64 c^2 < 2^24): rowss is exact, and
    mh_row_rstd is held to rstd_bound from it.  With a residual the stored values are ODD integers in 256..511 (an odd product
    of magnitude below 128: one odd column, the others even, plus an even R in 384..400), so every one of them needs 9 bits and
    a rowss taken before the rounding shows; without R the products are small and few need more than 8 bits.
    Else the full-width family: C exact, rowss within the bound of a 64-term sum."""
    if exact_ss and res:
        A, B = 2 * G.ints((M, K), 1, seed), G.ints((N, K), 1, seed + 1)
        A[:, 0], B[:, 0] = 1 - 2 * (G.ints((M,), 1, seed + 3) > 0).double(), 1 - 2 * (G.ints((N,), 1, seed + 4) > 0).double()
        R = (384 + 2 * G.ints((M, N), 4, seed + 2).abs()) * (1 - 2 * (G.ints((M, N), 1, seed + 5) > 0).double())
    else:
        A, B = G.exact_operands(M, N, K, seed, cap=max(1, int((500 / K) ** 0.5)) if exact_ss else None)
        R = G.residual(M, N, seed + 2, 4 * QA * QB) if res else None
    wide = res or not exact_ss
    P = G.exact_partials(A, B, [(0, K)], wide=not exact_ss)[0]
    q2 = 1.0 if exact_ss else QA * QB
    ref = G.exact_out(P, q2, BF16, 1.0, 1.0 if res else 0.0, R, wide=wide)
    ss = (ref * ref).view(M, N // 64, 64).sum(-1).T.contiguous()
    a = to_dev(G.operand(A, 1.0 if exact_ss else QA, BF16, False), be.dev)
    b = to_dev(G.operand(B, 1.0 if exact_ss else QB, BF16, False, pad=16), be.dev)
    cbuf, c = new_out(M, N, BF16, be.dev)
    r = to_dev(nan_input(R.to(BF16), pad=24), be.dev) if res else None
    parts = torch.full((N // 64 + 1, M), G.NAN, dtype=F32, device=be.dev)
    what = f"gemm_rowss {M}x{N}x{K} res={res}"
    be.gemm_rowss(a, b, c, r, parts, M, N, K)
    msg = G.mismatch(c, ref, A, B, q2, add=R)
    assert msg is None, f"{what}: C: {msg}"
    assert G.fence_ok(cbuf, M, N) and bool(torch.isnan(parts[N // 64]).all())
    if exact_ss:
        assert float(ref.abs().max()) < 512 and float(64 * ref.abs().max() ** 2) < 2 ** 24
        msg = G.mismatch(parts[: N // 64], ss, tile=(1, 256))
        assert msg is None, f"{what}: rowss (row = 64-column chunk, column = m): {msg}"
        want = rstd_ref(ref, RMS_EPS)
        for src in ("parts", "rows"):
            rstd = torch.full((M,), G.NAN, dtype=F32, device=be.dev)
            if src == "parts":
                be.row_rstd(None, parts, N // 64, M, N, RMS_EPS, rstd)
            else:
                be.row_rstd(c, None, 0, M, N, RMS_EPS, rstd)
            msg = G.out_of_bound(rstd[None, :], want[None, :], G.rstd_bound(want, N, BF16)[None, :])
            assert msg is None, f"{what}: row_rstd from the {src}: {msg}"
    else:
        msg = G.out_of_bound(parts[: N // 64], ss, G.reduction_bound(ss, 64))
        assert msg is None, f"{what}: rowss: {msg}"


@pytest.mark.parametrize("exact_ss", [True, False], ids=["ss_exact", "wide"])
@pytest.mark.parametrize("M,N,K,res", [(77, 64, 8, False), (257, 128, 64, True), (257, 320, 72, True), (300, 64, 264, False)])
def test_gemm_rowss(be, M, N, K, res, exact_ss):
    check_rowss(be, M, N, K, res, exact_ss)


def test_gemm_rowss_long_k(be):
    check_rowss(be, 77, 320, LONG_K, True, False)


# ----------------------------------------------------------------------------------------------------------- mh_gemm_skinny
def check_skinny(be, M, N, K, mode, mb=0, nbt=0, eps=0.0, gather=False, res=False, odd_ldc=False, seed=71):
    """scales are chosen AFTER the normalisation: the activations have unit size (rstd is about 1), the weights carry the power
    of two that puts rstd x product into [-8, 8] (gate|up: not in saturation) or [-4, 4], and the residual has that size too"""
    rows = 2 * N if mode == 1 else N
    T = M + 3 if gather else M                      # rows of the activation table
    A, W = G.exact_operands(T, rows, K, seed)
    P = G.exact_partials(A, W, [(0, K)])[0]
    ids = rids = None
    if gather:   # repeated ids and the last table row
        ids = (torch.arange(M) * 7 + 1) % T
        ids[0] = T - 1
        ids[M // 2] = ids[0]
        rids = (torch.arange(M) * 5 + 2) % T
        rids[M - 1] = T - 1
        A_rows, P = A[ids], P[ids]
    else:
        A_rows = A
    qa = G.scale_to(A, 2.0)
    xa = qa * A_rows
    rstd = torch.rsqrt((xa * xa).sum(-1) / K + eps) if eps > 0.0 else torch.ones(M, dtype=F64)   # (the sum of squares of integers is exact)
    limit = 8.0 if mode == 1 else 4.0
    qw = G.scale_to(rstd[:, None] * qa * P[:, :N], limit)
    q2 = qa * qw
    x = q2 * P
    R = G.residual(T, N, seed + 2, 2.0 ** -5) if res else None     # up to 4, as the product
    Rm = None if R is None else (R[rids] if gather else R)
    a, w = to_dev(G.operand(A, qa, BF16, False), be.dev), to_dev(G.operand(W, qw, BF16, False, pad=16), be.dev)
    r = to_dev(nan_input(R.to(BF16), pad=24), be.dev) if res else None
    cbuf, c = new_out(M, N, BF16, be.dev, ldc=(N + 5) | 1 if odd_ldc else None)
    what = f"gemm_skinny {M}x{N}x{K} mode={mode} mb={mb} nbt={nbt} eps={eps} gather={gather} res={res} odd_ldc={odd_ldc}"
    with options(be, skinny_mb=mb, skinny_nbt=nbt):
        be.gemm_skinny(a, w, c, r, mode, eps, None if ids is None else ids.to(be.dev), None if rids is None or not res else rids.to(be.dev), M, N, K)
    assert G.fence_ok(cbuf, M, N), f"{what}: written outside the view"
    assert limit / 2 < float((rstd[:, None] * x[:, :N]).abs().max()) <= limit
    if res:   # the residual moves more than half of the stored values
        assert float((G.rd(rstd[:, None] * x + Rm, BF16) != G.rd(rstd[:, None] * x, BF16)).double().mean()) > 0.5
    if eps > 0.0:
        # rstd is held to rstd_bound, and the fp32 value rstd x to the interval that leaves: roundings are monotone, so the
        # stored value lies between the rounded ends -- bit-exact wherever rstd's own error moves nothing, one bf16 step where
        # it does
        d = (G.rstd_bound(rstd, K, BF16) / rstd)[:, None]
        e1, e2 = (x * rstd[:, None] * (1 - d)).to(F32).to(F64), (x * rstd[:, None] * (1 + d)).to(F32).to(F64)
        lo, hi = torch.minimum(e1, e2), torch.maximum(e1, e2)
    if mode == 0:
        if eps > 0.0:
            add = 0.0 if Rm is None else Rm
            msg = G.within_rounded_interval(c, lo + add, hi + add, BF16)
            assert float((G.rd(lo + add, BF16) == G.rd(hi + add, BF16)).double().mean()) > 0.9
        else:
            msg = G.mismatch(c, G.exact_out(P, q2, BF16, 1.0, 1.0 if res else 0.0, Rm), A_rows, W, q2, tile=(16, 32), add=Rm)
        assert msg is None, f"{what}: {msg}"
        return
    if eps == 0.0:
        gus = [G.exact_out(P, q2, BF16).to(BF16)]
    else:   # gate and up each at either end of their interval
        g_lo, g_hi = G.rd(lo, BF16).to(BF16), G.rd(hi, BF16).to(BF16)
        assert float((g_lo == g_hi).double().mean()) > 0.9
        gus = [torch.cat([g[:, :N], u[:, N:]], 1) for g in (g_lo, g_hi) for u in (g_lo, g_hi)]
    got = c.detach().cpu().to(F64)
    low, high = None, None
    for gu_t in gus:   # (one candidate: the plain bound; four: their hull, which is the bound itself wherever the ends coincide)
        ref, terms = G.swiglu_fwd_ref(gu_t, BF16)
        bnd = G.swiglu_fwd_bound(terms, gu_t, BF16)
        low = ref - bnd if low is None else torch.minimum(low, ref - bnd)
        high = ref + bnd if high is None else torch.maximum(high, ref + bnd)
    wrong = ~((got >= low) & (got <= high))
    assert not wrong.any(), f"{what}: activation: {int(wrong.sum())}/{wrong.numel()} outside the bound, first {wrong.nonzero()[0].tolist()}"


# every batch class of the launcher: chunks per wave K / (32 waves) with 8 waves (plain, N <= 4096) or 4 (gate|up; two column
# blocks and N > 4096) -> batches of 16 / 8 / 4 chunks, or one chunk per batch with several batches (K = 768, 1536)
SKINNY = [  # (M, N, K, mb, nbt)
    (1, 16, 256, 0, 0), (15, 40, 512, 1, 1), (16, 2047, 768, 2, 1), (17, 2048, 1024, 4, 2), (33, 2056, 1536, 1, 2), (64, 4096, 2048, 2, 2),
    (64, 4104, 4096, 4, 0), (33, 3406, 768, 0, 0), (64, 40, 4096, 1, 1), (17, 4104, 1536, 2, 2), (16, 3406, 256, 4, 1), (1, 2048, 4096, 1, 2),
    (15, 16, 1536, 4, 1), (64, 2047, 1024, 2, 2), (33, 40, 768, 2, 0), (17, 16, 4096, 0, 0),
]


@pytest.mark.parametrize("mode", [0, 1], ids=["plain", "gateup"])
@pytest.mark.parametrize("M,N,K,mb,nbt", SKINNY)
def test_gemm_skinny_bit_exact(be, M, N, K, mb, nbt, mode):
    check_skinny(be, M, N, K, mode, mb, nbt, res=(mode == 0 and (M + N) % 2 == 0))


@pytest.mark.parametrize("mode", [0, 1], ids=["plain", "gateup"])
@pytest.mark.parametrize("M,N,K,mb,nbt", [(17, 40, 768, 1, 1), (64, 2056, 256, 4, 2), (33, 3406, 1536, 2, 0), (1, 16, 4096, 0, 0), (16, 4104, 512, 2, 2)])
def test_gemm_skinny_norm_gather_and_scalar_stores(be, M, N, K, mb, nbt, mode):
    check_skinny(be, M, N, K, mode, mb, nbt, eps=RMS_EPS, res=(mode == 0))
    check_skinny(be, M, N, K, mode, mb, nbt, gather=True, res=(mode == 0), odd_ldc=True)
    check_skinny(be, M, N, K, mode, mb, nbt, eps=RMS_EPS, gather=True, odd_ldc=(mode == 1))


# ----------------------------------------------------------------------------------------------------- full-mantissa family
def check_gauss(be):
    """Gaussian bf16 operands (all eight operand bits in use), one case per entry point"""
    M, N, K = 300, 264, 1096
    A, B = G.gauss_operands(M, N, K, 90)
    C64, terms = G.gauss_ref(A, B)
    a, b, bt = (to_dev(G.operand(X, 1.0, BF16, t, pad=16), be.dev) for X, t in ((A, False), (B, False), (B, True)))
    for name, run in (("mh_gemm rr", lambda c: be.gemm(a, 0, b, 0, c, None, M, N, K, 1.0, 0.0, BF16, 1, None)),
                      ("mh_gemm rt", lambda c: be.gemm(a, 0, bt, 1, c, None, M, N, K, 1.0, 0.0, BF16, 1, None)),
                      ("mh_gemm_nt_scaled", lambda c: be.gemm_nt_scaled(a, b, c, torch.ones(M, device=be.dev), M, N, K))):
        cbuf, c = new_out(M, N, BF16, be.dev)
        run(c)
        msg = G.out_of_bound(c, C64, G.gauss_bound(C64, terms, BF16))
        assert msg is None and G.fence_ok(cbuf, M, N), f"{name}: {msg}"
    # the product part of the fused entry points: gate|up, the v third of q|k|v, the C of mh_gemm_rowss (the epilogues' own
    # arithmetic is held to its bounds on the exact family above; mh_gemm_dswiglu stores no plain product)
    a5 = to_dev(G.operand(A * 2.0 ** -5, 1.0, BF16, False, pad=16), be.dev)      # (gates of unit size)
    cos_t, sin_t = G.rope_tables(64, 100)
    for name, n0, n1, run in (
            ("mh_gemm_swiglu", 0, 256, lambda c: be.gemm_swiglu(a5, b, c, new_out(M, 128, BF16, be.dev)[1], M, 128, K)),
            ("mh_gemm_rope", 128, 192, lambda c: be.gemm_rope(a5, b, c, G.rope_fused_table(cos_t, sin_t, 100).to(be.dev), 100, 100, 0, M, 192, K)),
            ("mh_gemm_rowss", 0, 256, lambda c: be.gemm_rowss(a5, b, c, None, torch.empty((4, M), dtype=F32, device=be.dev), M, 256, K))):
        cbuf, c = new_out(M, n1, BF16, be.dev)
        run(c)
        msg = G.out_of_bound(c[:, n0:], C64[:, n0:n1] / 32, G.gauss_bound(C64[:, n0:n1] / 32, terms[:, n0:n1] / 32, BF16))
        assert msg is None and G.fence_ok(cbuf, M, n1), f"{name}: {msg}"
    ws = torch.full((3, M, N), G.NAN, dtype=F32, device=be.dev)
    cbuf, c = new_out(M, N, BF16, be.dev)
    be.gemm(a, 0, b, 0, c, None, M, N, K, 1.0, 0.0, BF16, 3, ws)
    be.splitk_reduce(ws, c, None, M, N, 3, 1.0, 0.0, BF16)
    msg = G.out_of_bound(c, C64, G.gauss_bound(C64, terms, BF16))
    assert msg is None, f"mh_gemm split-K: {msg}"
    Ms = 33
    cbuf, c = new_out(Ms, N, BF16, be.dev)
    K2 = 1024
    be.gemm_skinny(a[:Ms], b, c, None, 0, 0.0, None, None, Ms, N, K2)
    C2, t2 = G.gauss_ref(A[:Ms, :K2], B[:, :K2])
    msg = G.out_of_bound(c, C2, G.gauss_bound(C2, t2, BF16))
    assert msg is None, f"mh_gemm_skinny: {msg}"
    af, bf = (to_dev(G.operand(X, 1.0, F32, False, pad=4), be.dev) for X in (A, B))
    cbuf, c = new_out(M, N, F32, be.dev)
    be.gemm(af, 0, bf, 0, c, None, M, N, K, 1.0, 0.0, F32, 1, None)
    msg = G.out_of_bound(c, C64, G.gauss_bound(C64, terms, F32))
    assert msg is None, f"mh_gemm fp32: {msg}"


def test_gaussian_operands_within_the_measured_bound(be):
    check_gauss(be)
