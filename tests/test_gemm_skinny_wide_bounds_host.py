"""CPU proof that the comparisons of tests/test_gemm_skinny_wide_gpu.py bite: that file's checks and case lists against a torch
restatement of mh_gemm_skinny_wide (test_gemm_bounds_host.Emu's arithmetic with the entry point's row-count refusals, in torch's fp32
product order and in the 32-deep blocked order), which is accepted, and against named wrong kernels that only a kernel walking
several 64-row groups can be, each of which at least one listed case rejects.  The flaws test_gemm_bounds_host.py names for the
narrow kernel are shown to bite at 129 rows as well."""
import pytest
import torch

import emu_ops as emu
import test_gemm_bounds_host as H
import test_gemm_gpu as T
import test_gemm_skinny_wide_gpu as Wd
from ref_gemm import BF16

WIDE_FLAWS = ("rows >= 64 read activation row m - 64", "rstd of row m taken from row m mod 64",
              "row_ids honoured in the first row group only", "residual of the last row block dropped",
              "gate|up rows >= 128 not rounded before SiLU")


class EmuWide(H.Emu):
    """mh_gemm_skinny_wide restated in torch on the poisoned buffers; `flaw`: one of WIDE_FLAWS or one of the narrow kernel's"""

    def _rows_product(self, rows, w, K):
        x, y = rows.float(), w[:, :K].float()
        if not self.blocked:
            return x @ y.T
        acc = torch.zeros((x.shape[0], y.shape[0]))
        for k0 in range(0, K, 32):
            acc = acc + x[:, k0:k0 + 32] @ y[:, k0:k0 + 32].T
        return acc

    def gemm_skinny(self, a, w, c, r, mode, eps, row_ids, res_ids, M, N, K, dtype=1):
        if dtype != 1 or not 64 < M <= 256 or K % 256:
            raise RuntimeError(f"mh_gemm_skinny_wide failed (1): gemm_skinny_wide: M={M} K={K} dtype={dtype}")
        f = self.flaw
        m = torch.arange(M)
        src = row_ids.clone() if row_ids is not None else m.clone()
        if f == "row_ids honoured in the first row group only" and row_ids is not None:
            src[64:] = m[64:]
        if f == "rows >= 64 read activation row m - 64":
            src[64:] = src[:M - 64].clone()
        rows = a[src][:, :K]
        x = self._rows_product(rows, w, K)
        if eps > 0.0:
            rstd = torch.rsqrt(rows.float().pow(2).sum(-1, keepdim=True) / K + eps)
            if f == "rstd of row m taken from row m mod 64":
                rstd = rstd[m % 64]
            x = x * rstd
        if mode == 1:
            g = x.to(BF16)
            if f == "gate and up halves swapped":
                g = torch.cat([g[:, N:], g[:, :N]], 1)
            if f == "skinny SiLU replaced by max(g, 0)":
                return self._store(c, (g[:, :N].float().clamp_min(0).to(BF16).float() * g[:, N:].float()), 16)
            act = emu.swiglu_fwd(g, torch.empty((M, N), dtype=BF16)).float()
            if f == "gate|up rows >= 128 not rounded before SiLU" and M > 128:
                gf, uf = x[128:, :N], x[128:, N:]
                act[128:] = (gf * torch.sigmoid(gf)).to(BF16).float() * uf
            return self._store(c, act, 16)
        if r is not None and not (eps > 0.0 and f == "skinny residual dropped when norm_eps > 0"):
            add = (r[res_ids] if res_ids is not None and f != "skinny residual row taken from m" else r[:M]).float().clone()
            if f == "residual of the last row block dropped":
                add[(M - 1) // 16 * 16:] = 0.0
            x = x + add
        self._store(c, x, 16)


def variants(be, M, N, K, mode):
    """the four variants every shape runs in"""
    yield lambda: T.check_skinny(be, M, N, K, mode, res=(mode == 0))
    yield lambda: T.check_skinny(be, M, N, K, mode, eps=T.RMS_EPS, res=(mode == 0))
    yield lambda: T.check_skinny(be, M, N, K, mode, gather=True, res=(mode == 0), odd_ldc=True)
    yield lambda: T.check_skinny(be, M, N, K, mode, eps=T.RMS_EPS, gather=True, odd_ldc=(mode == 1))


HOST_SHAPES = [(65, 40, 512), (80, 2047, 768), (127, 16, 1536), (128, 2056, 1024), (129, 3406, 768), (200, 4104, 256), (255, 40, 4096),
               (256, 2048, 1024), (256, 16, 256), (81, 4104, 1536)]


@pytest.mark.parametrize("blocked", [False, True], ids=["torch_fp32", "blocked_fp32"])
@pytest.mark.parametrize("M,N,K", HOST_SHAPES)
def test_the_correct_restatement_is_accepted(M, N, K, blocked):
    be = EmuWide(blocked=blocked)
    for mode in (0, 1):
        for case in variants(be, M, N, K, mode):
            case()


def test_the_gpu_file_lists_are_accepted_and_gaussian_too():
    be = EmuWide()
    for M, N, K in H.small(Wd.WIDE):
        for mode in (0, 1):
            T.check_skinny(be, M, N, K, mode, res=(mode == 0 and (M + N) % 2 == 0))
    for blocked in (False, True):
        Wd.check_gauss_wide(EmuWide(blocked=blocked))


def test_refusals_of_the_restatement():
    be = EmuWide()
    for M, K, dtype in ((64, 256, 1), (257, 256, 1), (128, 384, 1), (128, 256, 0)):
        with pytest.raises(RuntimeError, match="mh_gemm_skinny_wide failed"):
            be.gemm_skinny(None, None, None, None, 0, 0.0, None, None, M, 16, K, dtype)


def wide_cases(be):
    """the GPU file's own lists (its small shapes), as thunks: what the wrong kernels are judged by"""
    for M, N, K in H.small(Wd.WIDE):
        for mode in (0, 1):
            yield lambda M=M, N=N, K=K, mode=mode: T.check_skinny(be, M, N, K, mode, res=(mode == 0 and (M + N) % 2 == 0))
    for M, N, K in H.small(Wd.WIDE_VARIANTS):
        for mode in (0, 1):
            yield from list(variants(be, M, N, K, mode))[1:]


@pytest.mark.parametrize("flaw", WIDE_FLAWS)
def test_every_named_wrong_wide_kernel_is_rejected(flaw):
    rejected = 0
    for case in wide_cases(EmuWide(flaw)):
        try:
            case()
        except AssertionError:
            rejected += 1
            break
    assert rejected, f"no case of the GPU file's lists rejects: {flaw}"


@pytest.mark.parametrize("flaw", ["skinny residual row taken from m", "skinny residual dropped when norm_eps > 0", "skinny SiLU replaced by max(g, 0)"])
def test_the_narrow_kernels_flaws_still_bite_at_129_rows(flaw):
    be = EmuWide(flaw)
    rejected = 0
    for mode in (0, 1):
        for case in variants(be, 129, 40, 768, mode):
            try:
                case()
            except AssertionError:
                rejected += 1
    assert rejected, f"no variant at 129 rows rejects: {flaw}"
