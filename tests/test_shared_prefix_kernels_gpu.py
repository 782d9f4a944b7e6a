"""The two kernels of decode attention over a shared prompt (mh_attn_prefix_partial, attention_shared.hip;
mh_attn_decode_append_shared, attention_small.hip) at their boundaries, in the style and with the helpers of
test_cache_attention_gpu.py: prefix lengths around the MFMA tile (16 / 32 / 64-key wave tiles) and the chunk (C = 256), suffix
lengths around the rounds and steps of attn_decode_kernel, batch sizes around the 32-row query tile, every row the kernels must
not read poisoned, a one-hot probe that pins every prefix, suffix and new-key position, score shapes on both sides, device-memory
positions, agreement with the plain kernel and the refusals.

Value references are float64 torch over the exact values read: the prefix rows [0, pre_len), the suffix rows [0, pos - pre_len)
and the new key concatenated per (b, h), and the rotated q of kv_append."""
import pytest
import torch

from test_cache_attention_gpu import (BF16_ULP, DECODE_BOUND, DECODE_INST, F64, FWD_BOUND, NAN, SPIKE, grnd, same_bits)

pytestmark = pytest.mark.gpu

C = 256                       # MH_ATTN_PREFIX_CHUNK
H, HD, SCALE = 3, 64, 0.125
NPROBE_B = 64                 # rows b < 64 of one head carry mutually orthogonal q (a 64 x 64 Hadamard matrix): probe pairs


@pytest.fixture(scope="module")
def sh():
    import midi_model_amd.shared as real
    assert real.lib().cdll.mh_attn_prefix_chunk() == C == real.CHUNK
    return real


@pytest.fixture(scope="module")
def ops():
    import midi_model_amd.ops as real
    return real


def _hadamard64():
    i = torch.arange(64)
    x = i[:, None] & i[None, :]
    pop = sum((x >> b) & 1 for b in range(6))
    return (1.0 - 2.0 * (pop % 2)).float()   # Sylvester: rows mutually orthogonal, entries +-1


def _bound(dtype):
    """bf16: the prefix half rounds P to bf16 for the P V MFMA, as the event forward does -> FWD_BOUND[bf16]
    (2^-8 |o64| + 3e-3 rms(V)); fp32 keeps fp32 probabilities -> DECODE_BOUND (3e-6 |o64| + 2e-6 max|v|)"""
    if dtype == torch.bfloat16:
        return FWD_BOUND[dtype][0], FWD_BOUND[dtype][1], "rms"
    return DECODE_BOUND[dtype][0], DECODE_BOUND[dtype][1], "max"


def _case(ops, sh, dtype, B, pre, suf, Pmax, seed, shift=None, variant=0):
    """One launch pair over B * H (batch, head) pairs; pre prefix rows of Pmax, suffix rows [0, suf) of Lsuf cached, the new key at
    suffix row suf (pos = pre + suf).  ``shift`` is not None: PROBE launch -- pair p = b * H + h (b < 64, p < N) has its spike at
    key shift + p of the N = pre + suf + 1 keys it attends to (prefix keys first, then the suffix, the new key last); the q rows
    of one head are orthogonal, so the spike keys that other rows of the head planted in the shared prefix score ~0 for it.
    ``shift`` is None: SHAPE launch -- random q; per head on the prefix side (variant 0: keys x8 / x24, the maximum on the first
    prefix key, all-equal; variant 1: tiny, the maximum on the last prefix key, random) and per row b % 4 on the suffix side
    (keys x8 / x24, the maximum on the new key, all equal to the first prefix key, tiny).
    Returns (ref64, out64, vmax per pair, rms of the drawn V, probe mask, spike values)."""
    from midi_model_amd.engine import RopeTable
    dev = "cuda"
    BH, D, N = B * H, H * HD, pre + suf + 1
    pos = pre + suf
    Lsuf = suf + 1 + (0, 29, 700)[seed % 3]
    tab = RopeTable(HD, 10000.0, dev, pos + 1)
    qkv = grnd((B, 3 * D), dtype, seed)
    probe = shift is not None
    if probe:
        hq = _hadamard64().to(dev)
        signs = (1.0 - 2.0 * (torch.arange(H * HD, device=dev).view(H, HD) * 7 % 3 % 2)).float()
        nb = min(B, NPROBE_B)
        qkv.view(B, 3, H, HD)[:nb, 0] = (hq[:nb, None, :] * signs[None]).to(dtype)
        if B > nb:
            qkv.view(B, 3, H, HD)[nb:, 0] *= 0.25
    # the rotated q and the new k / v rows as kv_append makes them
    qa = qkv.clone()
    ka = torch.empty((B, H, pos + 1, HD), dtype=dtype, device=dev)
    va = torch.empty_like(ka)
    ops.kv_append(qa, tab.cos, tab.sin, ka, va, B, H, HD, pos + 1, pos)
    q_un = qkv[:, :D].reshape(BH, HD).to(F64)
    q_rot = qa[:, :D].reshape(BH, HD).to(F64)
    alpha = SPIKE / (SCALE * (q_rot * q_rot).sum(-1))
    kpre = torch.full((H, Pmax, HD), NAN, dtype=dtype, device=dev)
    vpre = torch.full((H, Pmax, HD), NAN, dtype=dtype, device=dev)
    kpre[:, :pre] = grnd((H, pre, HD), dtype, seed + 1)
    vpre[:, :pre] = grnd((H, pre, HD), dtype, seed + 2)
    ksuf = torch.full((B, H, Lsuf, HD), NAN, dtype=dtype, device=dev)
    vsuf = torch.full((B, H, Lsuf, HD), NAN, dtype=dtype, device=dev)
    if suf:
        ksuf[:, :, :suf] = grnd((B, H, suf, HD), dtype, seed + 3)
        vsuf[:, :, :suf] = grnd((B, H, suf, HD), dtype, seed + 4)
    drawn = torch.cat([vpre[:, :pre].reshape(-1), vsuf[:, :, :suf].reshape(-1), qkv[:, 2 * D:].reshape(-1)]).to(F64)
    rms_v = drawn.pow(2).mean().sqrt().item()
    kq, vq = qkv.view(B, 3, H, HD)[:, 1], qkv.view(B, 3, H, HD)[:, 2]
    ksf, vsf = ksuf.view(BH, Lsuf, HD), vsuf.view(BH, Lsuf, HD)
    is_probe = torch.zeros(BH, dtype=torch.bool, device=dev)
    spike_v = torch.zeros((BH, HD), dtype=F64, device=dev)
    spike_at = {}

    def k_scoring(p, c, q):  # a key whose score against pair p's q is c
        return (alpha[p] * c / SPIKE * q[p]).to(dtype)

    if probe:
        n_probe = min(min(B, NPROBE_B) * H, N)
        e = torch.arange(HD, device=dev)
        for p in range(n_probe):
            j = (shift + p) % N
            b, h = p // H, p % H
            sv = ((6.0 + (3 * j + e) % 7) * (1.0 - 2.0 * (j % 2))).to(dtype)   # |v| 6..12, one pattern per key index
            if j < pre:
                kpre[h, j], vpre[h, j] = k_scoring(p, SPIKE, q_rot), sv
            elif j < pre + suf:
                ksf[p, j - pre], vsf[p, j - pre] = k_scoring(p, SPIKE, q_rot), sv
            else:
                kq[b, h], vq[b, h] = k_scoring(p, SPIKE, q_un), sv             # the new key: rotated like q
            is_probe[p], spike_v[p], spike_at[p] = True, sv.to(F64), j
    else:
        if variant == 0:
            for j in {pre // 5, pre // 2, (3 * pre) // 4}:
                kpre[0, j] *= 8.0
            kpre[0, (9 * pre) // 10] *= 24.0
            kpre[1, 0] = k_scoring(1, 12.0, q_rot)                # pair (b 0, h 1): the maximum on the first prefix key
            kpre[2, 1:pre] = kpre[2, :1]
        else:
            kpre[0, :pre] *= 0.01
            kpre[1, pre - 1] = k_scoring((B - 1) * H + 1, 12.0, q_rot)   # pair (b B-1, h 1): ... on the last prefix key
        for b in range(B):
            for h in range(H):
                p, kind = b * H + h, (b + h) % 4
                if kind == 0 and suf:
                    for j in {suf // 5, suf // 2, (3 * suf) // 4}:
                        ksf[p, j] *= 8.0
                    ksf[p, (9 * suf) // 10] *= 24.0
                elif kind == 1:
                    kq[b, h] = k_scoring(p, 12.0, q_un)
                elif kind == 2 and suf:
                    ksf[p, :suf] = kpre[h, 0]
                elif kind == 3 and suf:
                    ksf[p, :suf] *= 0.01
    qa = qkv.clone()  # (the new keys changed: rotate again)
    ops.kv_append(qa, tab.cos, tab.sin, ka, va, B, H, HD, pos + 1, pos)
    k_new, v_new = ka[:, :, pos].clone(), va[:, :, pos].clone()
    kpre0, vpre0, ksuf0, vsuf0, qkv0 = kpre.clone(), vpre.clone(), ksuf.clone(), vsuf.clone(), qkv.clone()
    ws = torch.full((sh.workspace_floats(B, H, Pmax),), NAN, device=dev)
    o = torch.full((B, D), NAN, dtype=dtype, device=dev)
    sh.attn_prefix_partial(qkv, tab.cos, tab.sin, kpre, vpre, ws, B, H, HD, Pmax, pre, pos, SCALE)
    sh.attn_decode_append_shared(qkv, tab.cos, tab.sin, ksuf, vsuf, ws, o, B, H, HD, Lsuf, Pmax, pre, pos, SCALE)
    what = f"B {B} pre {pre} suf {suf} Pmax {Pmax} Lsuf {Lsuf}"
    assert same_bits(kpre, kpre0) and same_bits(vpre, vpre0) and same_bits(qkv, qkv0), f"{what}: prefix cache or qkv written"
    assert same_bits(ksuf[:, :, suf], k_new) and same_bits(vsuf[:, :, suf], v_new), f"{what}: appended row != kv_append's"
    ksuf0[:, :, suf], vsuf0[:, :, suf] = k_new, v_new
    assert same_bits(ksuf, ksuf0) and same_bits(vsuf, vsuf0), f"{what}: suffix cache written outside row pos - pre_len"
    # partials of chunks at or past ceil(pre / C) are not written (and never read: o is finite, checked by the caller)
    nch, used = (Pmax + C - 1) // C, (pre + C - 1) // C
    acc = ws[: BH * nch * 64].view(BH, nch, 64)
    ml = ws[BH * nch * 64:].view(BH, nch, 2)
    assert torch.isnan(acc[:, used:]).all() and torch.isnan(ml[:, used:]).all(), f"{what}: a partial past the prompt was written"
    assert torch.isfinite(acc[:, :used]).all() and torch.isfinite(ml[:, :used]).all(), f"{what}: non-finite partial"
    # positions from device memory (graph replay), into poisoned buffers again: the same bits -- and a second run of the same
    pd = torch.tensor([pos], dtype=torch.int32, device=dev)
    pl = torch.tensor([pre], dtype=torch.int32, device=dev)
    ws2 = torch.full_like(ws, NAN)
    o2 = torch.full_like(o, NAN)
    sh.attn_prefix_partial(qkv, tab.cos, tab.sin, kpre, vpre, ws2, B, H, HD, Pmax, 0, 0, SCALE, pl, pd)
    sh.attn_decode_append_shared(qkv, tab.cos, tab.sin, ksuf, vsuf, ws2, o2, B, H, HD, Lsuf, Pmax, 0, 0, SCALE, pl, pd)
    assert same_bits(ws2, ws) and same_bits(o2, o), f"{what}: device positions != host positions (or two runs differ)"
    assert same_bits(ksuf, ksuf0) and same_bits(vsuf, vsuf0)
    # float64 reference over the exact values read
    keys = torch.cat([kpre[None, :, :pre].expand(B, -1, -1, -1), ksuf[:, :, :suf], k_new[:, :, None]], 2).reshape(BH, N, HD).to(F64)
    vals = torch.cat([vpre[None, :, :pre].expand(B, -1, -1, -1), vsuf[:, :, :suf], v_new[:, :, None]], 2).reshape(BH, N, HD).to(F64)
    sc = torch.einsum("pd,pkd->pk", q_rot, keys) * SCALE
    if probe and N > 1:  # probe set-up: the spike is the maximum, by >= 20
        pp = is_probe.nonzero().flatten()
        top = sc[pp].topk(2, -1)
        want = torch.tensor([spike_at[int(p)] for p in pp], device=dev)
        assert torch.equal(top.indices[:, 0], want), f"{what}: probe set-up: spike is not the maximum"
        margin = (top.values[:, 0] - top.values[:, 1]).min().item()
        assert margin >= 20, f"{what}: probe set-up: spike margin {margin:.1f}"
    ref = torch.einsum("pk,pkd->pd", torch.softmax(sc, -1), vals)
    vmax = vals.abs().amax(dim=(1, 2))
    # agreement with the plain kernel on a [B, H, L, 64] cache that holds the prompt B times
    L = pos + 1
    kc = torch.full((B, H, L, HD), NAN, dtype=dtype, device=dev)
    vc = torch.full((B, H, L, HD), NAN, dtype=dtype, device=dev)
    kc[:, :, :pre], vc[:, :, :pre] = kpre[None, :, :pre], vpre[None, :, :pre]
    kc[:, :, pre:pos], vc[:, :, pre:pos] = ksuf[:, :, :suf], vsuf[:, :, :suf]
    o_plain = torch.full_like(o, NAN)
    ops.attn_decode_append(qkv, tab.cos, tab.sin, kc, vc, o_plain, B, H, HD, L, pos, SCALE)
    return (ref, o.view(BH, HD).to(F64), vmax, rms_v, is_probe, spike_v, o_plain.view(BH, HD).to(F64), what, set(spike_at.values()))


def _check(dtype, res, worst):
    ref, got, vmax, rms_v, is_probe, spike_v, plain, what, _ = res
    c_rel, c_abs, kind = _bound(dtype)
    bad = ~torch.isfinite(got).all(-1)
    assert not bad.any(), f"{what}: non-finite output (a poisoned row or partial read) at pairs {bad.nonzero().flatten()[:16].tolist()}"
    absterm = c_abs * (rms_v if kind == "rms" else vmax[:, None])
    if is_probe.any():
        serr = (got[is_probe] - spike_v[is_probe]).abs()
        sb = c_rel * spike_v[is_probe].abs() + (absterm if kind == "rms" else absterm[is_probe])
        bad = (serr > sb).any(-1)
        assert not bad.any(), f"{what}: one-hot probe misses at pairs {is_probe.nonzero().flatten()[bad][:16].tolist()}"
    err = (got - ref).abs()
    bound = c_rel * ref.abs() + absterm
    ratio = (err / bound).max().item()
    print(f"  {what}: err/bound {ratio:.3f}")
    assert ratio <= 1.0, f"{what}: max err/bound {ratio:.3f} at pair {int((err / bound).amax(-1).argmax())}"
    # the plain kernel is held to DECODE_BOUND: the two outputs agree within the sum of the two bounds
    pc_rel, pc_abs = DECODE_BOUND[dtype]
    pb = pc_rel * ref.abs() + pc_abs * vmax[:, None]
    pratio = ((got - plain).abs() / (bound + pb)).max().item()
    assert pratio <= 1.0, f"{what}: differs from attn_decode_append on a replicated cache, {pratio:.3f} of the summed bounds"
    worst[0] = max(worst[0], ratio)
    worst[1] = max(worst[1], pratio)


# (pre_len, suffix length, B): pre_len over {1, 15, 16, 17, 31, 32, 33, C-1, C, C+1, 2C+1, 3C+5}, the suffix over
# {0, 1, 31, 32, 33, 129} (bf16 hd64: KPW 8 -- round 32, step 128; fp32: round 16, step 64; the kernel walks `suffix` cached rows
# and takes the new one from LDS), B over {1, 3, 16, 17, 64, 65} (32-row query tiles: 1, 1, 1, 1, 2, 3 of them).  Long prefixes go
# with large batches: B * 3 pairs (<= 192 probes) pin pre + suffix + 1 keys in ceil(N / probes) launches.
PROBE_CASES = [(1, 0, 1), (15, 1, 3), (16, 31, 16), (17, 32, 17), (31, 33, 64), (32, 129, 65), (33, 0, 16), (1, 33, 17),
               (16, 1, 1), (31, 31, 3), (C - 1, 1, 64), (C, 31, 65), (C + 1, 32, 64), (2 * C + 1, 33, 65), (3 * C + 5, 129, 64)]
SHAPE_CASES = [(33, 129, 3, 0), (17, 1, 1, 1), (C - 1, 33, 17, 0), (C + 1, 0, 16, 1), (2 * C + 1, 32, 65, 0), (3 * C + 5, 31, 64, 1),
               (32, 32, 64, 1), (C, 129, 3, 0)]
assert {c[0] for c in PROBE_CASES} == {1, 15, 16, 17, 31, 32, 33, C - 1, C, C + 1, 2 * C + 1, 3 * C + 5}
assert {c[1] for c in PROBE_CASES} == {0, 1, 31, 32, 33, 129} and {c[2] for c in PROBE_CASES} == {1, 3, 16, 17, 64, 65}


@pytest.mark.parametrize("inst", ["bf16_hd64", "fp32_hd64"])
def test_shared_prefix_at_boundaries(ops, sh, inst):
    """attn_prefix_partial + attn_decode_append_shared at the prefix, suffix and batch sizes listed above (44 probe + 8 shape
    launch pairs per dtype), Pmax cycling through pre_len, + 29, + 700 and the suffix capacity likewise.
    Poison: prefix rows >= pre_len, suffix rows >= pos - pre_len (the appended row included), the whole workspace and o hold
    NaN before the launch; the outputs and the partials of the chunks in use must be finite and the partials past them still
    NaN; the prefix cache and qkv are bit-unchanged, the suffix cache is unchanged except row pos - pre_len, which equals
    kv_append's row bit for bit.  The same launches with pos / pre_len in device memory give the same bits (o and workspace).
    One-hot probe: every one of the pre_len + suffix + 1 key positions of every case is pinned by a pair whose score there is 30
    (>= 20 above every other, asserted on the reference) and whose v (|v| 6..12) no other key index holds.  Score shapes on
    both sides in the shape launches (_case).
    Bounds against float64 over the exact inputs: bf16 -- P is rounded to bf16 for the P V MFMA -- FWD_BOUND[bf16] =
    2^-8 |o64| + 3e-3 rms(V) with rms(V) that of the drawn N(0, 1) values (the spikes excluded); fp32 DECODE_BOUND =
    3e-6 |o64| + 2e-6 max|v|.  And within the sum of that bound and DECODE_BOUND of attn_decode_append on a cache that holds
    the prompt B times.
    Measured on the MI355X: not yet -- this test has not run on the device at this commit (the test prints each err/bound)."""
    dtype = DECODE_INST[inst][0]
    worst = [0.0, 0.0]
    n_launch = 0
    for n, (pre, suf, B) in enumerate(PROBE_CASES):
        Pmax = (pre, pre + 29, pre + 700)[n % 3]
        N = pre + suf + 1
        n_probe = min(min(B, NPROBE_B) * H, N)
        pinned = set()
        for shift in range(0, N, n_probe):
            res = _case(ops, sh, dtype, B, pre, suf, Pmax, 7000 + 13 * n + shift, shift=shift)
            _check(dtype, res, worst)
            pinned |= res[-1]
            n_launch += 1
        assert pinned == set(range(N)), f"pre {pre} suf {suf}: key positions never probed: {sorted(set(range(N)) - pinned)[:16]}"
    for n, (pre, suf, B, variant) in enumerate(SHAPE_CASES):
        Pmax = (pre + 29, pre + 700, pre)[n % 3]
        _check(dtype, _case(ops, sh, dtype, B, pre, suf, Pmax, 9000 + 17 * n, variant=variant), worst)
        n_launch += 1
    print(f"shared prefix {inst}: {n_launch} launch pairs, worst err/bound {worst[0]:.3f}, worst |shared - plain| / summed bounds "
          f"{worst[1]:.3f}")


def test_shared_prefix_refusals(ops, sh):
    """hd 32 / 128 / 256, pre_len 0, pre_len > Pmax, pos < pre_len and a full suffix: RuntimeError at the call, buffers
    bit-unchanged"""
    from midi_model_amd.engine import RopeTable
    B, Pmax, Lsuf = 2, 40, 4
    for dtype in (torch.bfloat16, torch.float32):
        for hd in (32, 128, 256, 64):
            D = H * hd
            tab = RopeTable(hd, 10000.0, "cuda", 64)
            qkv = grnd((B, 3 * D), dtype, 5)
            kp, vp = grnd((H, Pmax, hd), dtype, 6), grnd((H, Pmax, hd), dtype, 7)
            ks, vs = grnd((B, H, Lsuf, hd), dtype, 8), grnd((B, H, Lsuf, hd), dtype, 9)
            ws = torch.full((sh.workspace_floats(B, H, Pmax),), NAN, device="cuda")
            o = torch.full((B, D), NAN, dtype=dtype, device="cuda")
            keep = [t.clone() for t in (qkv, kp, vp, ks, vs, ws, o)]
            part = lambda pre, pos: sh.attn_prefix_partial(qkv, tab.cos, tab.sin, kp, vp, ws, B, H, hd, Pmax, pre, pos, hd ** -0.5)
            dec = lambda pre, pos: sh.attn_decode_append_shared(qkv, tab.cos, tab.sin, ks, vs, ws, o, B, H, hd, Lsuf, Pmax, pre,
                                                                pos, hd ** -0.5)
            if hd != 64:
                for fn in (part, dec):
                    with pytest.raises(RuntimeError, match="head_dim"):
                        fn(8, 9)
            else:
                for pre, pos in ((0, 3), (Pmax + 1, Pmax + 2), (8, 7)):
                    for fn in (part, dec):
                        with pytest.raises(RuntimeError, match="bad args"):
                            fn(pre, pos)
                with pytest.raises(RuntimeError, match="bad args"):
                    dec(8, 8 + Lsuf)   # a full suffix: row pos - pre_len == Lsuf
                with pytest.raises(RuntimeError, match="workspace"):
                    sh.attn_prefix_partial(qkv, tab.cos, tab.sin, kp, vp, ws[:-1], B, H, hd, Pmax, 8, 9, hd ** -0.5)
            torch.cuda.synchronize()
            for t, t0 in zip((qkv, kp, vp, ks, vs, ws, o), keep):
                assert same_bits(t, t0)
