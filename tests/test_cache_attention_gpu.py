"""The inference-side attention kernels at their boundaries (attention_small.hip, attention_mfma3.hip):

  1. single-query decode (mh_attn_decode, mh_attn_decode_append, mh_kv_append) at key counts that straddle the key loop's
     rounds, steps and both exits for every (dtype, head_dim) instantiation, with the cache rows it must not read poisoned,
     a one-hot probe that pins every key position, and score shapes that move the online-softmax reference;
  2. the cached-prefix forward mh_attn_fwd_tail against mh_attn_fwd (bit for bit) and a float64 softmax;
  3. the cache row movers mh_kv_store_rows / mh_kv_gather_rows / mh_kv_store_prefill, exactly, past the first grid pass;
  4. the work order of the event attention kernels (option attn_passes): identical bits for every pass count.

Value references are float64 torch on the exact values the kernels read (bf16 inputs converted); data movement is compared
bit for bit.  Every test that sets a kernel option reads it first and restores it."""
import contextlib

import pytest
import torch

import emu_ops as emu

pytestmark = pytest.mark.gpu

BF16_ULP = 2.0 ** -8  # |x - bf16(x)| <= 2^-8 |x|
F64 = torch.float64
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    import midi_model_amd.ops as real
    return real


def rnd(shape, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(shape, generator=g)).to(dtype)


def grnd(shape, dtype, seed, scale=1.0):
    """seeded normal values drawn on the device (the large decode caches and movers' inputs)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (scale * torch.randn(shape, generator=g, device="cuda")).to(dtype)


def bits(t):
    """the raw bits of a tensor: NaN sentinels compare equal, -0 and +0 do not"""
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


@contextlib.contextmanager
def options(ops, **kv):
    """set kernel options for the block, restoring the values read before"""
    old = {k: ops.get_option(k) for k in kv}
    try:
        for k, v in kv.items():
            ops.set_option(k, v)
        yield
    finally:
        for k, v in old.items():
            ops.set_option(k, v)


# ------------------------------------------------------------------------------------------------------------- 1. decode
# (dtype, head_dim) -> KPW, keys per wave per round of attn_decode_kernel: a round is 4 * KPW keys, a step (one register set of
# UNR = 4 rounds) STEP = 16 * KPW; sets A and B alternate, with an exit after each
DECODE_INST = {"bf16_hd64": (torch.bfloat16, 64, 8), "fp32_hd64": (torch.float32, 64, 4),
               "bf16_hd256": (torch.bfloat16, 256, 2), "fp32_hd256": (torch.float32, 256, 1)}
# |o - o64| <= C_REL |o64| + C_ABS max|v| (max over the pair's keys); see test_decode_at_loop_boundaries
DECODE_BOUND = {torch.bfloat16: (BF16_ULP, 2e-6), torch.float32: (3e-6, 2e-6)}
SPIKE = 30.0  # the one-hot probe's score (natural-log units); the other scores are ~N(0, 1)


def decode_lengths(kpw, append):
    rd, st = 4 * kpw, 16 * kpw
    ls = {1, rd - 1, rd, rd + 1, st - 1, st, st + 1, 2 * st - 1, 2 * st, 2 * st + 1, 3 * st + 1, 8 * st + rd + 3}
    if append:  # the cache walk covers len - 1 keys: every boundary shifted by one as well
        ls |= {x + 1 for x in ls}
    return sorted(x for x in ls if x >= 1)


def _decode_case(ops, dtype, hd, length, Lmax, append, seed):
    """One launch over B * H >= length + 6 (batch, head) pairs.  Pair i < length: the one-hot probe with its spike at key i.
    The six pairs behind: score shapes -- random; keys x8 / x24 (the moving-reference case of the event forward); the maximum on
    the first key; the maximum on the last key (APPEND: the new key); all-equal scores; tiny scores.  The rest: random.
    Returns (float64 reference, output, per-pair max|v|, spike v or None per pair, one-hot mask)."""
    from midi_model_amd.engine import RopeTable
    H = 3
    B = (length + 6 + H - 1) // H
    BH, D = B * H, H * hd
    scale = hd ** -0.5
    pos = length - 1
    ilen = length - 1 if append else length   # rows the kernel reads from the cache
    tab = RopeTable(hd, 10000.0, "cuda", Lmax + 1)
    qkv = grnd((B, 3 * D), dtype, seed)
    q_un = qkv[:, :D].reshape(BH, hd).to(F64)
    # the rotated q (APPEND: kv_append's rotation, the one the fused kernel must reproduce)
    if append:
        qa, ka, va = qkv.clone(), torch.empty((B, H, Lmax, hd), dtype=dtype, device="cuda"), None
        va = torch.empty_like(ka)
        ops.kv_append(qa, tab.cos, tab.sin, ka, va, B, H, hd, Lmax, pos)
        q_rot = qa[:, :D].reshape(BH, hd).to(F64)
    else:
        q_rot = q_un
    qn2 = (q_rot * q_rot).sum(-1)                               # |q|^2 per pair
    alpha = SPIKE / (scale * qn2)                               # k = alpha q: score = SPIKE
    kc = torch.full((B, H, Lmax, hd), NAN, dtype=dtype, device="cuda")
    vc = torch.full((B, H, Lmax, hd), NAN, dtype=dtype, device="cuda")
    kf, vf = kc.view(BH, Lmax, hd), vc.view(BH, Lmax, hd)
    if ilen > 0:
        kf[:, :ilen] = grnd((BH, ilen, hd), dtype, seed + 1)
        vf[:, :ilen] = grnd((BH, ilen, hd), dtype, seed + 2)
    # the new position's unrotated k, v (APPEND) live in qkv
    kq, vq = qkv.view(B, 3, H, hd)[:, 1], qkv.view(B, 3, H, hd)[:, 2]   # [B, H, hd]: pair p at (p // H, p % H)
    # the one-hot probe: pair i < length, spike at key i (i == pos in APPEND: the new key, set through its unrotated k)
    idx = torch.arange(length, device="cuda")
    e = torch.arange(hd, device="cuda")
    sign = 1.0 - 2.0 * (idx % 2)
    spike = ((6.0 + (3 * idx[:, None] + e[None, :]) % 7) * sign[:, None]).to(dtype)   # |v| 6..12, one pattern per pair
    ic = idx[:ilen]
    kf[ic, ic] = (alpha[ic, None] * q_rot[ic]).to(dtype)
    vf[ic, ic] = spike[:ilen]
    if append:
        kq[pos // H, pos % H] = (alpha[pos] * q_un[pos]).to(dtype)
        vq[pos // H, pos % H] = spike[pos]
    onehot = torch.zeros(BH, dtype=torch.bool, device="cuda")
    onehot[:length] = True
    spike_v = torch.zeros((BH, hd), dtype=F64, device="cuda")
    spike_v[:length] = spike.to(F64)

    def k_scoring(p, c, q):  # a key whose score against pair p's q is c
        return (alpha[p] * c / SPIKE * q[p]).to(dtype)

    s0 = length  # the score-shape pairs: s0 random, s0 + 1 big keys, + 2 first-key maximum, + 3 last-key maximum,
    if ilen > 0:  # + 4 all-equal scores, + 5 tiny scores
        for j in {ilen // 5, ilen // 2, (3 * ilen) // 4}:
            kf[s0 + 1, j] *= 8.0
        kf[s0 + 1, (9 * ilen) // 10] *= 24.0
        kf[s0 + 2, 0] = k_scoring(s0 + 2, 12.0, q_rot)
        kf[s0 + 4, 1:ilen] = kf[s0 + 4, :1]
        kf[s0 + 5, :ilen] *= 0.01
    if append:
        kq[(s0 + 3) // H, (s0 + 3) % H] = k_scoring(s0 + 3, 12.0, q_un)   # the new key: rotated like q
    elif ilen > 0:
        kf[s0 + 3, ilen - 1] = k_scoring(s0 + 3, 12.0, q_rot)
    kc0, vc0, qkv0 = kc.clone(), vc.clone(), qkv.clone()
    o = torch.full((B, D), NAN, dtype=dtype, device="cuda")
    if append:
        ops.attn_decode_append(qkv, tab.cos, tab.sin, kc, vc, o, B, H, hd, Lmax, pos, scale)
        # after APPEND: row pos of each cache is kv_append's row bit for bit, every other row and qkv unchanged
        qa, ka, va = qkv0.clone(), torch.empty_like(kc), torch.empty_like(vc)
        ops.kv_append(qa, tab.cos, tab.sin, ka, va, B, H, hd, Lmax, pos)
        assert same_bits(kc[:, :, pos], ka[:, :, pos]) and same_bits(vc[:, :, pos], va[:, :, pos]), "appended row"
        kc0[:, :, pos], vc0[:, :, pos] = ka[:, :, pos], va[:, :, pos]
    else:
        ops.attn_decode(qkv, kc, vc, o, B, H, hd, Lmax, length, scale)
    assert same_bits(kc, kc0) and same_bits(vc, vc0) and same_bits(qkv, qkv0), "decode wrote outside its row"
    # the device position (graph replay) through the same entry point: the same bits
    pd = torch.tensor([pos], dtype=torch.int32, device="cuda")
    o2 = torch.full((B, D), NAN, dtype=dtype, device="cuda")
    if append:
        ops.attn_decode_append(qkv, tab.cos, tab.sin, kc, vc, o2, B, H, hd, Lmax, 0, scale, pd)
    else:
        ops.attn_decode(qkv, kc, vc, o2, B, H, hd, Lmax, 1, scale, pd)
    assert same_bits(o2, o), "pos_dev != host position"
    # float64 reference over the exact values the kernel reads (APPEND: the cache as it is after the launch), 256 pairs at a time
    ref = torch.empty((BH, hd), dtype=F64, device="cuda")
    vmax = torch.empty((BH,), dtype=F64, device="cuda")
    for p0 in range(0, BH, 256):
        p1 = min(BH, p0 + 256)
        k64 = kf[p0:p1, :length].to(F64)
        v64 = vf[p0:p1, :length].to(F64)
        sc = torch.einsum("pd,pkd->pk", q_rot[p0:p1], k64) * scale
        if p0 < length and length > 1:  # probe set-up: the spike is the maximum, by >= 20
            n1 = min(p1, length) - p0
            top = sc[:n1].topk(2, -1)
            assert torch.equal(top.indices[:, 0], idx[p0:p0 + n1]), "probe set-up: spike is not the maximum"
            margin = (top.values[:, 0] - top.values[:, 1]).min().item()
            assert margin >= 20, f"probe set-up: spike margin {margin:.1f}"
        ref[p0:p1] = torch.einsum("pk,pkd->pd", torch.softmax(sc, -1), v64)
        vmax[p0:p1] = v64.abs().amax(dim=(1, 2))
    return ref, o.view(BH, hd).to(F64), vmax, spike_v, onehot


@pytest.mark.parametrize("append", [False, True], ids=["plain", "append"])
@pytest.mark.parametrize("inst", list(DECODE_INST))
def test_decode_at_loop_boundaries(ops, inst, append):
    """attn_decode / attn_decode_append at every key count around the loop's round (4 KPW keys), step (STEP = 16 KPW) and the
    exits after register sets A and B (2 STEP +- 1), 3 STEP + 1 and one count above 8 STEP; APPEND (which walks len - 1 cached
    keys and takes the new one from LDS) also at each count + 1.  Capacity Lmax cycles through len, len + 29 and len + 700.
    Every cache row at or past len holds NaN, in APPEND the row at pos too: an extra key read poisons the output.  After the
    launch: APPEND's row pos equals kv_append's bit for bit, every other cache row and qkv are unchanged, and the same launch
    with the position in device memory (pos_dev) gives the same bits.

    One-hot probe: pair i < len has k_i = alpha q (score 30, >= 20 above every other) and a v of magnitude 6..12 no other key
    holds, so its output must be that v: a missing, extra or shifted key, or K/V of a wrong pair, moves it by O(1).  Six pairs
    behind carry score shapes (_decode_case).
    Bound, against float64 softmax(q K^T / sqrt(hd)) V over the exact inputs (APPEND: the rotated q of kv_append, the cache after
    the launch): the kernel accumulates in fp32 -- scores over hd products, __expf, the online rescale, the lane-group / wave
    merges: a few fp32 ulps of max|v| -- and rounds only O.  bf16: 2^-8 |o64| (output rounding) + 2e-6 max|v|; fp32:
    3e-6 |o64| + 2e-6 max|v|.  Measured on the MI355X: the bf16 error never exceeds the rounding term (worst 0.985 of the
    bound); fp32 reaches 0.14 of its bound and exceeds its relative term by at most 2.1e-7 max|v|.  One dropped key of len
    moves an element by ~|v_j - o| / len, 2e-3 at len 1024: far outside."""
    dtype, hd, kpw = DECODE_INST[inst]
    c_rel, c_abs = DECODE_BOUND[dtype]
    worst_abs, worst_ratio = 0.0, 0.0
    for n, length in enumerate(decode_lengths(kpw, append)):
        Lmax = (length, length + 29, length + 700)[n % 3]
        ref, got, vmax, spike_v, onehot = _decode_case(ops, dtype, hd, length, Lmax, append, 1000 * kpw + length)
        bad = ~torch.isfinite(got).all(-1)
        assert not bad.any(), (f"len {length} Lmax {Lmax}: non-finite output (a poisoned row read, or no key) at pairs "
                               f"{bad.nonzero().flatten()[:16].tolist()}")
        # the one-hot probe: the spike's v
        serr = (got[onehot] - spike_v[onehot]).abs()
        sbound = c_rel * spike_v[onehot].abs() + c_abs * vmax[onehot][:, None]
        bad = (serr > sbound).any(-1)
        assert not bad.any(), (f"len {length} Lmax {Lmax}: one-hot probe misses key positions "
                               f"{bad.nonzero().flatten()[:16].tolist()}")
        err = (got - ref).abs()
        bound = c_rel * ref.abs() + c_abs * vmax[:, None]
        ratio = (err / bound).max().item()
        assert ratio <= 1.0, (f"len {length} Lmax {Lmax}: max err/bound {ratio:.3f} at pair "
                              f"{int((err / bound).amax(-1).argmax())}")
        worst_ratio = max(worst_ratio, ratio)
        worst_abs = max(worst_abs, ((err - c_rel * ref.abs()).clamp(min=0) / vmax[:, None]).max().item())
    print(f"decode {inst} {'append' if append else 'plain'}: worst err/bound {worst_ratio:.3f}, "
          f"worst (err - c_rel|o|)/max|v| {worst_abs:.2e} (allowed {c_abs:.0e})")


def test_decode_refuses_what_it_cannot_serve(ops):
    """head dims other than 64 / 256, len > Lmax (or len < 1) without a device position, and kv_append at pos >= Lmax: a
    RuntimeError at the call, nothing launched"""
    from midi_model_amd.engine import RopeTable
    B, H = 2, 2
    for dtype in (torch.bfloat16, torch.float32):
        for hd in (32, 128, 64, 256):
            D, Lmax = H * hd, 16
            tab = RopeTable(hd, 10000.0, "cuda", Lmax + 2)
            qkv = grnd((B, 3 * D), dtype, 5)
            kc, vc = grnd((B, H, Lmax, hd), dtype, 6), grnd((B, H, Lmax, hd), dtype, 7)
            o = torch.empty((B, D), dtype=dtype, device="cuda")
            if hd in (32, 128):
                with pytest.raises(RuntimeError, match="head_dim"):
                    ops.attn_decode(qkv, kc, vc, o, B, H, hd, Lmax, 4, hd ** -0.5)
                with pytest.raises(RuntimeError, match="head_dim"):
                    ops.attn_decode_append(qkv, tab.cos, tab.sin, kc, vc, o, B, H, hd, Lmax, 3, hd ** -0.5)
                continue
            for length in (Lmax + 1, 0):
                with pytest.raises(RuntimeError, match="bad args"):
                    ops.attn_decode(qkv, kc, vc, o, B, H, hd, Lmax, length, hd ** -0.5)
                with pytest.raises(RuntimeError, match="bad args"):
                    ops.attn_decode_append(qkv, tab.cos, tab.sin, kc, vc, o, B, H, hd, Lmax, length - 1, hd ** -0.5)
            kc0, vc0 = kc.clone(), vc.clone()
            for pos in (Lmax, Lmax + 1, -1):
                with pytest.raises(RuntimeError, match="kv_append"):
                    ops.kv_append(qkv, tab.cos, tab.sin, kc, vc, B, H, hd, Lmax, pos)
            torch.cuda.synchronize()
            assert same_bits(kc, kc0) and same_bits(vc, vc0)


# ------------------------------------------------------------------------------------------- 2. cached-prefix forward
# bf16 forms of the forward that serve the tail (attn_v3 bits, attn_v3_wps): 255 / 223 lazy reference maximum + three K/V
# stages (223: the two-call backward, same forward), 127 / 95 three stages, 63 two stages; wps picks the register budget
TAIL_FORMS = [(255, 0), (255, 3), (223, 0), (127, 0), (127, 2), (127, 3), (95, 0), (63, 0), (63, 3)]
TAIL_S = [129, 256, 515, 1100]
TAIL_BH = [(1, 1), (2, 4), (3, 5)]   # 1, 8 and 15 (batch, head) pairs: 15 is a second, ragged group of eight


def q_starts(S):
    return sorted({q for q in (0, 1, 63, 64, 127, 128, 129, S - 129, S - 64, S - 1) if 0 <= q < S})


def attn_ref64(qkv, B, S, H):
    """float64 causal softmax(q k^T / 8) v and log-sum-exp over the exact inputs: ([B*S, D], [B, H, S])"""
    D = H * 64
    q, k, v = (qkv[:, i * D:(i + 1) * D].to(F64).view(B, S, H, 64).transpose(1, 2) for i in range(3))
    s = torch.matmul(q, k.transpose(-1, -2)) * 0.125
    s = s.masked_fill(torch.ones(S, S, dtype=torch.bool, device=s.device).triu(1), float("-inf"))
    lse = torch.logsumexp(s, -1)
    o = torch.matmul(torch.softmax(s, -1), v).transpose(1, 2).reshape(B * S, D)
    rms_v = v.pow(2).mean().sqrt().item()
    return o, lse, rms_v


# |o - o64| <= C_REL |o64| + C_RMS rms(V); |lse - lse64| <= C_LSE max(1, |lse64|)
FWD_BOUND = {torch.bfloat16: (BF16_ULP, 3e-3, 1e-4), torch.float32: (5e-6, 5e-6, 2e-6)}


def check_fwd64(o, lse, ref, B, S, H, dtype, q_start=0, what=""):
    o64, lse64, rms_v = ref
    c_rel, c_rms, c_lse = FWD_BOUND[dtype]
    D, Sp = H * 64, (S + 63) // 64 * 64
    got = o.view(B, S, D)[:, q_start:].to(F64)
    want = o64.view(B, S, D)[:, q_start:]
    err = (got - want).abs()
    ratio = (err / (c_rel * want.abs() + c_rms * rms_v)).max().item()
    assert ratio <= 1.0, (what, "o", err.max().item(), ratio)
    lerr = (lse.view(B, H, Sp)[:, :, q_start:S].to(F64) - lse64[:, :, q_start:]).abs()
    lratio = (lerr / (c_lse * lse64[:, :, q_start:].abs().clamp(min=1.0))).max().item()
    assert lratio <= 1.0, (what, "lse", lerr.max().item(), lratio)
    return ratio, lratio


def _tail_checks(ops, qkv, ref, dtype, B, S, H, what):
    """checks 1-4 of test_attention_tail for the option in force; returns the worst err/bound ratios"""
    D, Sp = H * 64, (S + 63) // 64 * 64
    tile = 128 if dtype == torch.bfloat16 else 64
    o_full = torch.full((B * S, D), NAN, dtype=dtype, device="cuda")
    lse_full = torch.full((B * H * Sp,), NAN, device="cuda")
    ops.attn_fwd(qkv, o_full, lse_full, B, S, H, 0.125)
    worst = [0.0, 0.0]
    for q_start in q_starts(S):
        t0 = q_start // tile * tile
        for poison in (False, True):
            x = qkv
            if poison:  # q columns of the rows below the first computed tile (production: zeroes) must not be read
                x = qkv.clone()
                x.view(B, S, 3 * D)[:, :t0, :D] = NAN
            o = torch.full((B * S, D), NAN, dtype=dtype, device="cuda")
            lse = torch.full((B * H * Sp,), NAN, device="cuda")
            ops.attn_fwd_tail(x, o, lse, B, S, H, 0.125, q_start)
            w = f"{what} q_start={q_start}{' q rows poisoned' if poison else ''}"
            ov, fv = o.view(B, S, D), o_full.view(B, S, D)
            lv, flv = lse.view(B, H, Sp), lse_full.view(B, H, Sp)
            assert same_bits(ov[:, t0:], fv[:, t0:]), f"{w}: o differs from attn_fwd"
            assert same_bits(lv[:, :, t0:S], flv[:, :, t0:S]), f"{w}: lse differs from attn_fwd"
            assert torch.isnan(ov[:, :t0].float()).all(), f"{w}: o rows below the first computed tile were written"
            assert torch.isnan(lv[:, :, :t0]).all(), f"{w}: lse entries below the first computed tile were written"
            if not poison:
                r = check_fwd64(o, lse, ref, B, S, H, dtype, q_start, w)
                worst = [max(a, b) for a, b in zip(worst, r)]
    return worst


@pytest.mark.parametrize("B,H", TAIL_BH, ids=["bh1", "bh8", "bh15"])
@pytest.mark.parametrize("S", TAIL_S)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_attention_tail(ops, dtype, S, B, H):
    """mh_attn_fwd_tail computes the query tiles holding rows >= q_start (bf16: 128-row tiles of the third-form forward, every
    form that serves it; fp32: 64-row tiles of the plain kernel).  (1) From the first computed tile t0 on, o and lse equal
    attn_fwd's over the same qkv and option bit for bit: both launches run the same tile code.  (2) Rows >= q_start against
    a float64 causal softmax: |err| <= 2^-8 |O| + 3e-3 rms(V) for bf16 (test_flash_attention_at_benchmarked_length: output
    rounding, P rounded to bf16 for the PV product), 5e-6 |O| + 5e-6 rms(V) for fp32 (fp32 accumulation and __expf); lse
    within 1e-4 (bf16) / 2e-6 (fp32) of max(1, |lse|).  Measured worst on the MI355X: 0.87 of the bf16 bound (o), 0.2 of the
    fp32 bounds.  (3) o rows and lse entries below t0 keep their NaN sentinel.  (4) With
    NaN in the q columns of the rows below t0, (1)-(3) still hold."""
    qkv = rnd((B * S, 3 * H * 64), dtype, 70 + S).cuda()
    ref = attn_ref64(qkv, B, S, H)
    worst = [0.0, 0.0]
    forms = TAIL_FORMS if dtype == torch.bfloat16 else [(255, 0)]
    for v3, wps in forms:
        with options(ops, attn_v3=v3, attn_v3_wps=wps):
            r = _tail_checks(ops, qkv, ref, dtype, B, S, H, f"attn_v3={v3} wps={wps}")
        worst = [max(a, b) for a, b in zip(worst, r)]
    print(f"attn_fwd_tail {dtype} S={S} B*H={B * H}: worst err/bound o {worst[0]:.3f}, lse {worst[1]:.3f}")


def test_attention_tail_refuses_what_it_cannot_serve(ops):
    """q_start outside [0, S); attn_v3 = 15 / 7 (the forward from a prepared V^T copy, which the tail cannot take); the first
    form in the A/B library: an error at the call, not the rows computed some other way"""
    B, S, H = 1, 200, 2
    D, Sp = H * 64, 256
    for dtype in (torch.bfloat16, torch.float32):
        qkv = rnd((B * S, 3 * D), dtype, 80).cuda()
        o = torch.full((B * S, D), NAN, dtype=dtype, device="cuda")
        lse = torch.full((B * H * Sp,), NAN, device="cuda")
        for q_start in (-1, S, S + 64):
            with pytest.raises(RuntimeError, match="attn_fwd_tail"):
                ops.attn_fwd_tail(qkv, o, lse, B, S, H, 0.125, q_start)
    qkv = rnd((B * S, 3 * D), torch.bfloat16, 81).cuda()
    o = torch.full((B * S, D), NAN, dtype=torch.bfloat16, device="cuda")
    lse = torch.full((B * H * Sp,), NAN, device="cuda")
    for v3 in (15, 7):
        with options(ops, attn_v3=v3):
            for q_start in (0, 64, 150):
                with pytest.raises(RuntimeError):
                    ops.attn_fwd_tail(qkv, o, lse, B, S, H, 0.125, q_start)
    with ops.ab_library():
        with options(ops, attn_v3=0):
            for q_start in (0, 64, 150):
                with pytest.raises(RuntimeError):
                    ops.attn_fwd_tail(qkv, o, lse, B, S, H, 0.125, q_start)
    torch.cuda.synchronize()
    assert torch.isnan(o.float()).all() and torch.isnan(lse).all()


# ---------------------------------------------------------------------------------------------------- 3. row movers
GRID_CAP = 16384 * 256   # threads of the movers' capped grid; one 16-byte pack per thread per pass


@pytest.mark.parametrize("hd", [64, 256])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("B,S,H,Lmax,pos0", [(1, 1, 1, 1, 0), (2, 5, 3, 40, 0), (2, 39, 3, 40, 1), (3, 21, 2, 100, 13),
                                             (2, 130, 4, 300, 170)])
def test_kv_store_and_gather_rows(ops, dtype, hd, B, S, H, Lmax, pos0):
    """kv_store_rows writes rows [pos0, pos0 + S) of each (sequence, head) cache exactly and nothing else (sentinel rows
    around them); kv_gather_rows brings rows [0, n) back into the K / V columns of rows [b Stot, b Stot + n) with their q
    columns zeroed and rows [n, Stot) of each sequence untouched; store then gather returns the K and V columns bit for bit.
    pos0 = 0 runs through kv_store_prefill as well (the same entry point)."""
    _movers(ops, dtype, hd, B, S, H, Lmax, pos0, seed=90 + hd + pos0)


@pytest.mark.parametrize("dtype,B", [(torch.bfloat16, 17), (torch.float32, 9)], ids=["bf16", "fp32"])
def test_kv_movers_past_the_first_grid_pass(ops, dtype, B):
    """(S = 2048, H = 16, hd = 64: B * S * H * hd / (16-byte pack) exceeds the 16384 x 256 threads of the capped grid, so
    every mover's grid-stride loop runs a second pass)"""
    S, H, hd = 2048, 16, 64
    packs = B * S * H * hd * (2 if dtype == torch.bfloat16 else 4) // 16
    assert packs > GRID_CAP
    _movers(ops, dtype, hd, B, S, H, S, 0, seed=95)


def _movers(ops, dtype, hd, B, S, H, Lmax, pos0, seed):
    D = H * hd
    qkv = grnd((B * S, 3 * D), dtype, seed)
    prior = grnd((B, H, Lmax, hd), dtype, seed + 1)   # rows [0, pos0): what the cache held before
    kc = torch.full((B, H, Lmax, hd), NAN, dtype=dtype, device="cuda")
    vc = torch.full((B, H, Lmax, hd), NAN, dtype=dtype, device="cuda")
    kc[:, :, :pos0], vc[:, :, :pos0] = prior[:, :, :pos0], -prior[:, :, :pos0]
    want_k, want_v = kc.clone(), vc.clone()
    emu.kv_store_rows(qkv, want_k, want_v, B, S, H, hd, Lmax, pos0)
    ops.kv_store_rows(qkv, kc, vc, B, S, H, hd, Lmax, pos0)
    assert same_bits(kc, want_k) and same_bits(vc, want_v), "kv_store_rows"
    assert torch.isnan(kc[:, :, pos0 + S:].float()).all() and torch.isnan(vc[:, :, pos0 + S:].float()).all()
    if pos0 == 0:
        k2 = torch.full_like(kc, NAN)
        v2 = torch.full_like(vc, NAN)
        ops.kv_store_prefill(qkv, k2, v2, B, S, H, hd, Lmax)
        assert same_bits(k2, kc) and same_bits(v2, vc), "kv_store_prefill"
    del want_k, want_v
    # gather back: all rows stored so far, into a buffer with room behind them
    n = pos0 + S
    Stot = n + 7
    full = torch.full((B * Stot, 3 * D), NAN, dtype=dtype, device="cuda")
    full.view(B, Stot, 3 * D)[:, n:] = grnd((B, Stot - n, 3 * D), dtype, seed + 2)
    tail = full.view(B, Stot, 3 * D)[:, n:].clone()
    ops.kv_gather_rows(kc, vc, full, B, n, Stot, H, hd, Lmax)
    fv = full.view(B, Stot, 3 * D)
    assert same_bits(fv[:, :n, :D], torch.zeros((B, n, D), dtype=dtype, device="cuda")), "gathered q columns not zero"
    assert same_bits(fv[:, :n, D:2 * D], kc[:, :, :n].transpose(1, 2).reshape(B, n, D)), "gathered K"
    assert same_bits(fv[:, :n, 2 * D:], vc[:, :, :n].transpose(1, 2).reshape(B, n, D)), "gathered V"
    assert same_bits(fv[:, pos0:n, D:], qkv.view(B, S, 3 * D)[:, :, D:]), "store -> gather changed K / V"
    assert same_bits(fv[:, n:], tail), "gather wrote rows [n, Stot)"


def test_kv_movers_refuse_bad_arguments(ops):
    """MH_REQUIRE: pos0 + S > Lmax, n > Stot, n > Lmax and hd % 8 != 0 are errors at the call"""
    B, S, H, hd, Lmax = 2, 8, 2, 64, 16
    D = H * hd
    qkv = torch.zeros((B * S, 3 * D), dtype=torch.bfloat16, device="cuda")
    kc, vc = torch.zeros((B, H, Lmax, hd), dtype=torch.bfloat16, device="cuda"), torch.zeros((B, H, Lmax, hd), dtype=torch.bfloat16, device="cuda")
    ops.kv_store_rows(qkv, kc, vc, B, S, H, hd, Lmax, Lmax - S)     # the limit itself is served
    for pos0 in (Lmax - S + 1, Lmax, -1):
        with pytest.raises(RuntimeError, match="kv_store_rows"):
            ops.kv_store_rows(qkv, kc, vc, B, S, H, hd, Lmax, pos0)
    with pytest.raises(RuntimeError, match="kv_store_rows"):
        ops.kv_store_prefill(qkv, kc, vc, B, Lmax + 1, H, hd, Lmax)
    with pytest.raises(RuntimeError, match="kv_store_rows"):
        ops.kv_store_rows(qkv, kc, vc, B, S, H, 60, Lmax, 0)
    ops.kv_gather_rows(kc, vc, qkv, B, S, S, H, hd, Lmax)
    for n, Stot, Lm in ((S + 1, S, Lmax), (S, S, S - 1), (0, S, Lmax)):
        with pytest.raises(RuntimeError, match="kv_gather_rows"):
            ops.kv_gather_rows(kc, vc, qkv, B, n, Stot, H, hd, Lm)
    with pytest.raises(RuntimeError, match="kv_gather_rows"):
        ops.kv_gather_rows(kc, vc, qkv, B, S, S, H, 60, Lmax)


# ------------------------------------------------------------------------------------------------------ 4. work order
PASSES = [0, 1, 2, 3, 4, 5, 7, 9, 16, 100]


def test_attention_work_order_does_not_change_results(ops):
    """attn_passes P cuts each (batch, head) pair's query-tile ranks into P chunks (attn_work; P = 0 and P > tile count are
    clamped).  B = 3, H = 5 (15 pairs: a ragged second group of eight), S = 1100 (9 query tiles of 128, neither a multiple of
    64 nor of 128).  Forward, the one-call backward (mh_attn_bwd_o) and the tail at q_start = 700 (4 tiles: P clamps
    differently) must be bit-identical to the P = 5 run -- no atomics, every tile writes its own rows.  The P = 5 run holds
    the float64 bounds: forward as test_attention_tail; backward as test_flash_attention_at_benchmarked_length, each element
    within 1.25 x 2^-8 (|g| + sum_k |dS_k| |other_k|) + 1e-3 rms(g) (output rounding + dS / P rounded to bf16 for the MFMA)
    and rms(err) < 3e-3 rms(g)."""
    B, H, S, q_start = 3, 5, 1100, 700
    D, Sp = H * 64, (S + 63) // 64 * 64
    dt = torch.bfloat16
    qkv = rnd((B * S, 3 * D), dt, 100).cuda()
    do = rnd((B * S, D), dt, 101).cuda()
    runs = {}
    for P in PASSES:
        with options(ops, attn_passes=P):
            o = torch.full((B * S, D), NAN, dtype=dt, device="cuda")
            lse = torch.full((B * H * Sp,), NAN, device="cuda")
            ops.attn_fwd(qkv, o, lse, B, S, H, 0.125)
            dqkv = torch.full((B * S, 3 * D), NAN, dtype=dt, device="cuda")
            ops.attn_bwd(qkv, o, do, lse, dqkv, B, S, H, 0.125)
            ot = torch.full((B * S, D), NAN, dtype=dt, device="cuda")
            lt = torch.full((B * H * Sp,), NAN, device="cuda")
            ops.attn_fwd_tail(qkv, ot, lt, B, S, H, 0.125, q_start)
            runs[P] = (o, lse, dqkv, ot, lt)
    base = runs[5]
    for P, r in runs.items():
        for name, a, b in zip(("o", "lse", "dqkv", "tail o", "tail lse"), r, base):
            assert same_bits(a, b), f"attn_passes={P}: {name} differs from attn_passes=5"
    o, lse, dqkv, ot, lt = base
    ref = attn_ref64(qkv, B, S, H)
    fr = check_fwd64(o, lse, ref, B, S, H, dt, 0, "forward")
    check_fwd64(ot, lt, ref, B, S, H, dt, q_start, "tail")
    assert torch.isnan(ot.view(B, S, D)[:, :q_start // 128 * 128].float()).all()
    # backward against float64 closed-form gradients over the same inputs, with delta from the stored O
    q, k, v = (qkv[:, i * D:(i + 1) * D].to(F64).view(B, S, H, 64).transpose(1, 2) for i in range(3))
    dof = do.to(F64).view(B, S, H, 64).transpose(1, 2)
    od = o.to(F64).view(B, S, H, 64).transpose(1, 2)
    s = torch.matmul(q, k.transpose(-1, -2)) * 0.125
    s = s.masked_fill(torch.ones(S, S, dtype=torch.bool, device="cuda").triu(1), float("-inf"))
    p = torch.softmax(s, -1)
    del s
    ds = p * (torch.matmul(dof, v.transpose(-1, -2)) - (dof * od).sum(-1, keepdim=True)) * 0.125
    grads = {"dq": torch.matmul(ds, k), "dk": torch.matmul(ds.transpose(-1, -2), q), "dv": torch.matmul(p.transpose(-1, -2), dof)}
    rbs = {"dq": torch.matmul(ds.abs(), k.abs()), "dk": torch.matmul(ds.abs().transpose(-1, -2), q.abs()),
           "dv": torch.matmul(p.transpose(-1, -2), dof.abs())}
    del ds, p
    worst = 0.0
    for i, nm in enumerate(("dq", "dk", "dv")):
        want = grads[nm].transpose(1, 2).reshape(B * S, D)
        rb = rbs[nm].transpose(1, 2).reshape(B * S, D)
        e = (dqkv[:, i * D:(i + 1) * D].to(F64) - want).abs()
        rms = want.pow(2).mean().sqrt().item()
        bnd = 1.25 * BF16_ULP * (want.abs() + rb) + 1e-3 * rms
        ratio = (e / bnd).max().item()
        assert ratio <= 1.0, (nm, e.max().item(), ratio)
        assert e.pow(2).mean().sqrt().item() < 3e-3 * rms, (nm, e.pow(2).mean().sqrt().item() / rms)
        worst = max(worst, ratio)
    print(f"attn_passes {PASSES}: identical bits; P = 5 worst err/bound: forward o {fr[0]:.3f}, lse {fr[1]:.3f}, "
          f"backward {worst:.3f}")
