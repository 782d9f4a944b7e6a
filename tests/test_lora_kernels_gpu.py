"""The two kernels behind a LoRA adapter per decode row on the MI355X (gemm_skinny.hip: mh_gemm_skinny_ext, mh_lora_shrink_rows),
against the exact operand family, the poisoned operands and the fenced outputs of tests/ref_gemm.py; the checks themselves are in
tests/ref_lora.py, and tests/test_lora_bounds_host.py proves on the CPU that they reject named wrong kernels."""
import pytest
import torch

import ref_gemm as G
import ref_lora as L
import test_gemm_gpu as T
from ref_gemm import BF16
from ref_streamers import RMS_EPS

pytestmark = pytest.mark.gpu


class Hip(T.Hip):
    def gemm_skinny_ext(self, a, w, c, r, t, bst, mode, eps, row_ids, res_ids, M, N, K, K2, parts, dtype=BF16):
        p, ld = self.p, self.ld
        self.call("mh_gemm_skinny_ext", p(a), ld(a), p(w), ld(w), p(c), ld(c), p(r), ld(r), p(t), ld(t), p(bst), ld(bst), mode, eps,
                  p(row_ids), p(res_ids), M, N, K, K2, parts, self.dt(dtype))

    def lora_shrink(self, a, astack, t, row_adapter, slot_scale, row_ids, M, K, Gs, R, parts, dtype=BF16):
        p, ld = self.p, self.ld
        self.call("mh_lora_shrink_rows", p(a), ld(a), p(astack), ld(astack), p(t), ld(t), p(row_adapter), p(slot_scale), p(row_ids),
                  M, K, Gs, R, parts, self.dt(dtype))

    def gemm_skinny_any(self, a, w, c, r, mode, eps, M, N, K):
        p, ld = self.p, self.ld
        self.call("mh_gemm_skinny" if M <= 64 else "mh_gemm_skinny_wide", p(a), ld(a), p(w), ld(w), p(c), ld(c), p(r), ld(r), mode, eps,
                  None, None, M, N, K, 1)

    def last_error(self):
        return self._lib().cdll.mh_last_error().decode()


@pytest.fixture(scope="module")
def be():
    return Hip()


def ext_id(s):
    return "x".join(str(v) for v in s[:5]) + ("-gateup" if s[5] else "-plain")


@pytest.mark.parametrize("M,N,K,K2,parts,mode", L.EXT_SHAPES, ids=[ext_id(s) for s in L.EXT_SHAPES])
def test_ext_bit_exact_against_the_per_part_sums(be, M, N, K, K2, parts, mode):
    L.check_ext_variants(be, M, N, K, K2, parts, mode)


@pytest.mark.parametrize("Gs,R", L.SHRINK_GR)
@pytest.mark.parametrize("M", L.SHRINK_M)
def test_shrink_masks_scales_and_writes_every_element(be, M, Gs, R):
    L.check_shrink_all(be, M, Gs, R)


@pytest.mark.parametrize("M", [17, 64, 129])
def test_no_adapter_returns_the_bits_of_the_plain_projection(be, M):
    """Gaussian bf16 operands, row_adapter all -1: shrink then ext == mh_gemm_skinny / _wide, for the three projection kinds of a
    layer (q|k|v: row scale, 3 parts; o / down: residual, 1 part; gate|up: row scale, SwiGLU, 2 parts).  Values, so -0 == +0."""
    D, I, Gs, R = 256, 512, 4, 64
    g = torch.Generator().manual_seed(5)

    def rn(*shape, s=1.0):
        return (torch.randn(shape, generator=g) * s).to(BF16).to(be.dev)

    none = torch.full((M,), -1, dtype=torch.int32, device=be.dev)
    sc = torch.tensor([0.5, 2.0, 1.0, 0.25], device=be.dev)
    for N, K, parts, mode, eps, res in [(3 * D, D, 3, 0, RMS_EPS, False), (D, D, 1, 0, 0.0, True), (I, D, 2, 1, RMS_EPS, False),
                                        (D, I, 1, 0, 0.0, True)]:
        rows = 2 * N if mode == 1 else N
        a, w, r = rn(M, K), rn(rows, K, s=K ** -0.5), rn(M, N) if res else None
        astack, bst = rn(parts * Gs * R, K, s=K ** -0.5), rn(rows, Gs * R)
        t = torch.full((M, parts * Gs * R), G.NAN, dtype=BF16, device=be.dev)
        be.lora_shrink(a, astack, t, none, sc, None, M, K, Gs, R, parts)
        assert bool((t == 0).all()), "a row without adapter has a non-zero T"
        want, got = torch.full((M, N), G.NAN, dtype=BF16, device=be.dev), torch.full((M, N), G.NAN, dtype=BF16, device=be.dev)
        be.gemm_skinny_any(a, w, want, r, mode, eps, M, N, K)
        be.gemm_skinny_ext(a, w, got, r, t, bst, mode, eps, None, None, M, N, K, Gs * R, parts)
        assert not torch.isnan(want).any() and bool((got == want).all()), f"N={N} K={K} parts={parts} mode={mode}: {int((got != want).sum())} differ"


@pytest.mark.parametrize("what,kw,word", L.REFUSALS, ids=[r[0] for r in L.REFUSALS])
def test_refusals_keep_the_poison_and_leave_a_message(be, what, kw, word):
    msg = L.check_refusal(be, **kw)
    assert word in msg and word in be.last_error()
