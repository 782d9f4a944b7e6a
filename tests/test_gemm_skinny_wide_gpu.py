"""mh_gemm_skinny_wide (decode batches of 65 to 256 rows) on the MI355X, by the checks of tests/test_gemm_gpu.py: `check_skinny` on the
exact operand family (integer operands, every correct kernel returns the same bits whatever order its waves sum in), in the fenced,
poisoned buffers of that file, through a backend whose `gemm_skinny` is the wide entry point.

Shapes: the rows where the handling of row groups can go wrong -- one row past a 64-row group (65, 129), five 16-row blocks (80), the
edges of eight blocks (127, 128), a ragged and a full last group (200, 255, 256) -- crossed with the launcher's column classes
(N < 2048: one 16-column block on 8 waves; 2048 <= N <= 4096: two blocks on 8 waves; N > 4096: two blocks on 4 waves; ragged last
blocks 40, 2047, 2056, 3406, 4104) and its K classes (chunks per wave K / 32 / waves -> batches of 16, 8, 4 or several of 1; (129, 2056, 2048) with the row scale is the class the launcher moves from batches of 8 to 4).
The launcher has no tiling options (64 rows per workgroup always), so nothing is parametrised over them; the narrow entry point's
options are left at their defaults and ignored.

tests/test_gemm_skinny_wide_bounds_host.py runs the same checks on the CPU against a restatement and named wrong kernels."""
import pytest
import torch

import ref_gemm as G
import test_gemm_gpu as T
from ref_gemm import BF16, F32
from ref_streamers import RMS_EPS

pytestmark = pytest.mark.gpu


class HipWide(T.Hip):
    """test_gemm_gpu.Hip with the wide entry point behind `gemm_skinny`"""

    def gemm_skinny(self, a, w, c, r, mode, eps, row_ids, res_ids, M, N, K, dtype=1):
        p, ld = self.p, self.ld
        self.call("mh_gemm_skinny_wide", p(a), ld(a), p(w), ld(w), p(c), ld(c), p(r), ld(r), mode, eps, p(row_ids), p(res_ids), M, N, K, dtype)


@pytest.fixture(scope="module")
def be():
    return HipWide()


WIDE = [  # (M, N, K)
    (65, 40, 512), (80, 2047, 768), (127, 16, 1536), (128, 2056, 1024), (129, 3406, 768), (200, 4104, 256),
    (255, 40, 4096), (256, 2048, 1024), (256, 16, 256), (81, 4104, 1536), (65, 3406, 4096), (200, 2048, 1536),
]


@pytest.mark.parametrize("mode", [0, 1], ids=["plain", "gateup"])
@pytest.mark.parametrize("M,N,K", WIDE)
def test_gemm_skinny_wide_bit_exact(be, M, N, K, mode):
    T.check_skinny(be, M, N, K, mode, res=(mode == 0 and (M + N) % 2 == 0))


WIDE_VARIANTS = [(65, 40, 768), (129, 2056, 256), (200, 3406, 1536), (256, 16, 4096), (80, 4104, 512), (255, 2047, 1024), (129, 2056, 2048)]


@pytest.mark.parametrize("mode", [0, 1], ids=["plain", "gateup"])
@pytest.mark.parametrize("M,N,K", WIDE_VARIANTS)
def test_gemm_skinny_wide_norm_gather_and_scalar_stores(be, M, N, K, mode):
    T.check_skinny(be, M, N, K, mode, eps=RMS_EPS, res=(mode == 0))
    T.check_skinny(be, M, N, K, mode, gather=True, res=(mode == 0), odd_ldc=True)
    T.check_skinny(be, M, N, K, mode, eps=RMS_EPS, gather=True, odd_ldc=(mode == 1))


def check_gauss_wide(be):
    """Gaussian bf16 operands (all eight operand bits in use) under the bound test_gemm_gpu.check_gauss holds the narrow kernel to"""
    M, N, K = 200, 264, 1024
    A, B = G.gauss_operands(M, N, K, 91)
    C64, terms = G.gauss_ref(A, B)
    a, b = (T.to_dev(G.operand(X, 1.0, BF16, False, pad=16), be.dev) for X in (A, B))
    cbuf, c = T.new_out(M, N, BF16, be.dev)
    be.gemm_skinny(a, b, c, None, 0, 0.0, None, None, M, N, K)
    msg = G.out_of_bound(c, C64, G.gauss_bound(C64, terms, BF16))
    assert msg is None and G.fence_ok(cbuf, M, N), f"mh_gemm_skinny_wide: {msg}"


def test_gaussian_operands_within_the_bound(be):
    check_gauss_wide(be)


@pytest.mark.parametrize("M,K,dtype,what", [(64, 256, 1, "64 rows"), (257, 256, 1, "257 rows"), (128, 384, 1, "K = 384"), (128, 256, 0, "fp32")],
                         ids=["M64", "M257", "K384", "fp32"])
def test_gemm_skinny_wide_refusals(be, M, K, dtype, what):
    """what the entry point does not serve is refused with a message, before any launch: the output keeps its poison"""
    N = 16
    a = torch.zeros((M, K), dtype=BF16 if dtype else F32, device=be.dev)
    w = torch.zeros((N, K), dtype=a.dtype, device=be.dev)
    cbuf, c = T.new_out(M, N, a.dtype, be.dev)
    before = cbuf.clone()
    with pytest.raises(RuntimeError, match="mh_gemm_skinny_wide failed"):
        be.gemm_skinny(a, w, c, None, 0, 0.0, None, None, M, N, K, dtype)
    msg = be._lib().cdll.mh_last_error()
    assert msg and b"gemm_skinny_wide" in msg and len(msg) > len(b"gemm_skinny_wide: "), f"{what}: mh_last_error = {msg!r}"
    torch.cuda.synchronize()
    assert torch.equal(before.view(torch.uint8), cbuf.view(torch.uint8)), f"{what}: the refused call wrote"
