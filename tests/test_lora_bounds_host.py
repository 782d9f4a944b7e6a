"""CPU proof that the checks of tests/test_lora_kernels_gpu.py bite: the same checks (tests/ref_lora.py), on their small shapes,
against the torch restatement of the two entry points -- accepted -- and against named wrong kernels -- each rejected by at least
one case."""
import pytest

import ref_lora as L

SMALL_EXT = [s for s in L.EXT_SHAPES if s[0] * s[1] * (s[2] + s[3]) <= 3e7]


def test_the_correct_restatement_is_accepted():
    be = L.Emu()
    for M, N, K, K2, parts, mode in SMALL_EXT:
        L.check_ext_variants(be, M, N, K, K2, parts, mode)
    for M in (1, 17, 65):
        for Gs, R in L.SHRINK_GR:
            L.check_shrink_all(be, M, Gs, R)


def test_the_shape_lists_reach_every_tiling():
    modes = {(s[5], s[0] > 64) for s in L.EXT_SHAPES}
    assert modes == {(0, False), (1, False), (0, True), (1, True)}
    assert {s[4] for s in L.EXT_SHAPES} == {1, 2, 3} and any(s[1] >= 2048 for s in L.EXT_SHAPES) and any(s[1] % 16 for s in L.EXT_SHAPES)


def ext_cases(be):
    for M, N, K, K2, parts, mode in SMALL_EXT:
        yield lambda M=M, N=N, K=K, K2=K2, parts=parts, mode=mode: L.check_ext_variants(be, M, N, K, K2, parts, mode)


def shrink_cases(be):
    for M in (17, 65):
        for Gs, R in L.SHRINK_GR:
            yield lambda M=M, Gs=Gs, R=R: L.check_shrink_all(be, M, Gs, R)


@pytest.mark.parametrize("flaw", L.Emu.FLAWS_EXT + L.Emu.FLAWS_SHRINK)
def test_every_named_wrong_kernel_is_rejected(flaw):
    be = L.Emu(flaw)
    caught = 0
    for case in (ext_cases if flaw in L.Emu.FLAWS_EXT else shrink_cases)(be):
        try:
            case()
        except AssertionError:
            caught += 1
            break      # (one rejecting case is the proof)
    assert caught > 0, f"no case rejects: {flaw}"


@pytest.mark.parametrize("what,kw,word", L.REFUSALS, ids=[r[0] for r in L.REFUSALS])
def test_refusals_keep_the_poison(what, kw, word):
    assert word in L.check_refusal(L.Emu(), **kw)
