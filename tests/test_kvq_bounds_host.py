"""The 8-bit K/V format on the CPU (tests/ref_kvq.py): the round-trip bound of Q / D, the codes it may produce, and the
decode bound of test_kvq_kernels_gpu.py applied to the torch restatement of the kernel -- it must accept the restatement and reject
every named wrong kernel."""
import pytest
import torch

import kvq_common as kc
import ref_kvq


def _rows():
    g = torch.Generator().manual_seed(0)
    rows = [torch.randn((256, 64), generator=g) * s for s in (1e-3, 1e-2, 1.0, 30.0, 1e4)]
    rows.append(torch.zeros(1, 64))
    one = torch.randn((8, 64), generator=g) * 1e-3
    one[:, 5] = torch.tensor([-7.0, 9.0, 448.0, -448.0, 1e4, -3e-2, 1.0, 2.5])   # one dominant element, either sign
    rows.append(one)
    return torch.cat(rows).bfloat16()


def test_round_trip_bound_and_codes():
    """|D(Q(x)) - x| <= max(2^-4 |x|, 2^-10 s) (1 + 2^-20) elementwise: half a step of a 3-bit mantissa is 2^-4 relative for a
    normal code, half a subnormal step (2^-9) is 2^-10 in units of s, and the two fp32 roundings (x / s, code * s) are the 2^-20
    of room.  The amax element maps to code 126 or 254 (+-448), and the NaN codes 0x7F / 0xFF never appear."""
    x = _rows()
    codes, s = ref_kvq.quantize(x)
    assert codes.dtype == torch.uint8 and codes.shape == x.shape and s.dtype == torch.float32 and s.shape == x.shape[:1]
    assert ((codes & 0x7F) != 0x7F).all()
    d = ref_kvq.dequantize(codes, s)
    xf = x.float()
    lim = torch.maximum(2.0 ** -4 * xf.abs(), 2.0 ** -10 * s[:, None]) * (1 + 2.0 ** -20)
    ratio = ((d - xf).abs().double() / lim.double().clamp_min(1e-300)).max()
    assert ((d - xf).abs() <= lim).all(), float(ratio)
    amax = xf.abs().amax(-1)
    at = xf.abs().argmax(-1)
    top = codes[torch.arange(len(x)), at]
    nz = amax > 0
    assert ((top[nz] == 126) | (top[nz] == 254)).all()
    assert (s[~nz] == 1).all() and (codes[~nz] == 0).all()
    assert torch.equal(ref_kvq.dequantize64(codes, s).float(), d), "D() in fp32 is one exact-product rounding"


def test_ties_and_subnormals():
    """amax = 448 exactly (s = 1): 17 and 19 sit midway between codes (16, 18, 20: ties go to the even mantissa), 2^-10 is half
    the smallest subnormal (-> 0) and 3 * 2^-10 midway between 2^-9 and 2^-8 (-> 2^-8)"""
    x = torch.zeros(64)
    x[:6] = torch.tensor([448.0, 17.0, 19.0, 2.0 ** -10, 3 * 2.0 ** -10, -17.0])
    codes, s = ref_kvq.quantize(x.bfloat16())
    assert float(s) == 1.0
    assert ref_kvq.code_values(codes)[:6].tolist() == [448.0, 16.0, 20.0, 0.0, 2.0 ** -8, -16.0]
    t, _ = ref_kvq.quantize(x.bfloat16(), "truncate")
    assert ref_kvq.code_values(t)[:6].tolist() == [448.0, 16.0, 18.0, 0.0, 2.0 ** -9, -16.0]


LENGTHS = ref_kvq.decode_lengths(520)   # (the GPU test's: every loop edge up to the two-set cycle of 512 keys)


def test_the_restatement_is_inside_the_decode_bound():
    worst = max(kc.check_restatement(n, 520, 100 + n) for n in LENGTHS)
    print(f"restatement: worst |err| / bound = {worst:.3f}")
    assert worst <= 1.0, worst


@pytest.mark.parametrize("wrong", ref_kvq.WRONG)
def test_the_decode_bound_rejects(wrong):
    """every named wrong kernel lands outside the bound.  A flaw of the cached keys is shown at a short row and at a row of more than
    one round; a flaw of the appended row alone (its rounding, its dequantization) moves the output by that row's softmax weight
    times 2^-4 of its value, so it is shown where the row has weight: alone (n = 0) and behind three keys"""
    for n in (0, 3) if wrong in ("truncation", "new row unquantized") else (3, 70):
        r = kc.check_restatement(n, 300, 200 + n, wrong)
        assert r > 1.0, (wrong, n, r)
