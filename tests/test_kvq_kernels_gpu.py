"""The three kernels of the 8-bit K/V cache on the MI355X (attention_kvq.hip), held to tests/ref_kvq.py:

  store   mh_kv_store_seqs_rows_fp8: codes and scale bits equal ref_kvq.quantize of the same bf16 rows, every other byte keeps its
          sentinel (0xA5 codes, NaN scales); ties, subnormals, an all-zero row, a negative amax, one large among 63 tiny elements;
          dropped sequences write nothing;
  decode  mh_attn_decode_append_rows_fp8 at the edges of its key loop: (a) the appended row equals quantize() of the row
          ops.kv_append_rows writes into a bf16 cache, and nothing else changes; (b) the output within the decode bound of
          kvq_common.py of float64 attention over the exactly dequantized cache; (c) a one-hot probe for every key; (d) a row's bits
          do not depend on the other rows;
  fork    mh_kv_fork_rows_fp8: codes and scales copied bit for bit, sentinels kept, a fan-out, dropped pairs.
"""
import pytest
import torch

import kvq_common as kc
import ref_kvq

pytestmark = pytest.mark.gpu

NAN = float("nan")
H, HD = 3, 64
D = H * HD


@pytest.fixture(scope="module")
def ops():
    import midi_model_amd.ops as real
    return real


def sentinel_cache(*lead):
    k8 = torch.full(lead + (HD,), 0xA5, dtype=torch.uint8, device="cuda")
    return k8, k8.clone(), torch.full(lead + (2,), NAN, dtype=torch.float32, device="cuda")


def same_f32_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ store
def _store_inputs(M):
    g = torch.Generator().manual_seed(11)
    qkv = torch.randn((M, 3 * D), generator=g) * torch.exp2(torch.randint(-8, 9, (M, 1), generator=g).float())
    k = qkv[:, D:2 * D].view(M, H, HD)
    v = qkv[:, 2 * D:].view(M, H, HD)
    k[0, 0] = 0.0                                            # an all-zero row
    v[0, 1] = 0.0
    k[1, 0] = torch.randn(HD, generator=g)
    k[1, 0, 9] = -7.5                                        # amax negative
    for t in (k[2, 1], v[3, 2]):                             # amax = 448 exactly: s = 1, ties and subnormals
        t[:] = 0.0
        t[:8] = torch.tensor([448.0, 17.0, 19.0, 2.0 ** -10, 3 * 2.0 ** -10, -17.0, -19.0, -3 * 2.0 ** -10])
    k[4, 2] = torch.randn(HD, generator=g) * 1e-4            # one large among 63 tiny
    k[4, 2, 63] = 300.0
    v[5, 0] = torch.randn(HD, generator=g) * 1e-6
    v[5, 0, 0] = -1e4
    return qkv.bfloat16()


def _expect_store(qkv, lengths, rows, B, Lmax):
    ek, ev, es = [t.cpu() for t in sentinel_cache(B, H, Lmax)]
    a = 0
    for r, L in zip(rows, lengths):
        if 0 <= r < B:
            ek[r, :, :L], es[r, :, :L, 0] = ref_kvq.quantize(qkv[a:a + L, D:2 * D].view(L, H, HD).transpose(0, 1))
            ev[r, :, :L], es[r, :, :L, 1] = ref_kvq.quantize(qkv[a:a + L, 2 * D:].view(L, H, HD).transpose(0, 1))
        a += L
    return ek, ev, es


def test_store_writes_quantize_and_nothing_else(ops):
    """four packed sequences (a length of 1, a length of Lmax; 3 x 218 = 654 (event, head) rows: 20.4 workgroups of 32 rows) into
    rows of a cache of 7: codes and scale bits equal quantize(), every other byte keeps its sentinel"""
    lengths, Lmax, B, rows = (10, 1, 200, 7), 200, 7, (5, 0, 3, 6)
    M = sum(lengths)
    qkv = _store_inputs(M)
    plan = ops.attn_seq_plan(lengths, H).upload("cuda")
    k8, v8, sc = sentinel_cache(B, H, Lmax)
    ops.kv_store_seqs_rows_fp8(qkv.cuda(), plan, rows, k8, v8, sc, H, HD, Lmax)
    torch.cuda.synchronize()
    ek, ev, es = _expect_store(qkv, lengths, rows, B, Lmax)
    assert torch.equal(k8.cpu(), ek), (k8.cpu() != ek).nonzero()[:4]
    assert torch.equal(v8.cpu(), ev), (v8.cpu() != ev).nonzero()[:4]
    assert same_f32_bits(sc.cpu(), es)
    # (said twice) the named inputs did what they are there for
    assert (ek[5, 0, 0] == 0).all() and float(es[5, 0, 0, 0]) == 1.0
    assert ref_kvq.code_values(ek[5, 1, 2, :8]).tolist() == [448.0, 16.0, 20.0, 0.0, 2.0 ** -8, -16.0, -20.0, -2.0 ** -8]
    assert int(ek[5, 0, 1, 9]) == 254 and ((ek[0] & 0x7F) != 0x7F).all()


def test_store_drops_sequences_outside_the_cache(ops):
    """row ids -1 and B, through the entry point (the wrapper refuses them): nothing of those sequences is written"""
    from midi_model_amd.lib import lib
    from midi_model_amd.ops import _p, _stream, dt
    lengths, Lmax, B = (6, 9, 4), 12, 3
    M = sum(lengths)
    qkv = _store_inputs(M).cuda()
    plan = ops.attn_seq_plan(lengths, H).upload("cuda")
    rows = torch.tensor([-1, 1, B], dtype=torch.int32, device="cuda")
    k8, v8, sc = sentinel_cache(B, H, Lmax)
    lib().call("mh_kv_store_seqs_rows_fp8", _p(qkv), _p(plan.seq_start), _p(rows), _p(k8), _p(v8), _p(sc), 3, B, M, H, HD, Lmax,
               dt(qkv), _stream())
    torch.cuda.synchronize()
    ek, ev, es = _expect_store(qkv.cpu(), lengths, (-1, 1, B), B, Lmax)
    assert torch.equal(k8.cpu(), ek) and torch.equal(v8.cpu(), ev) and same_f32_bits(sc.cpu(), es)
    assert (k8[0] == 0xA5).all() and (k8[2] == 0xA5).all() and torch.isnan(sc[0]).all()
    for kw, match in ((dict(hd=128), "head_dim"), (dict(dtype=0), "bf16"), (dict(n=4), "4 sequences for a cache of 3")):
        a = dict(n=3, hd=HD, dtype=dt(qkv))
        a.update(kw)
        with pytest.raises(RuntimeError, match=match):
            lib().call("mh_kv_store_seqs_rows_fp8", _p(qkv), _p(plan.seq_start), _p(rows), _p(k8), _p(v8), _p(sc), a["n"], B, M, H,
                       a["hd"], Lmax, a["dtype"], _stream())
    with pytest.raises(ValueError, match="outside"):
        ops.kv_store_seqs_rows_fp8(qkv, plan, [-1, 1, 2], k8, v8, sc, H, HD, Lmax)


# ----------------------------------------------------------------------------------------------------------------- decode
LMAX = 520
POSITIONS = ref_kvq.decode_lengths(LMAX)   # cached rows per sequence = its position: every loop edge +-1, 0 and LMAX - 1


def _rope(n):
    from midi_model_amd.engine import RopeTable
    return RopeTable(HD, 10000.0, torch.device("cuda"), n)


@pytest.fixture(scope="module")
def decode_run(ops):
    """one launch over len(POSITIONS) rows x 3 heads, shared by (a), (b) and (d): the inputs, the caches before and after, and
    the rotated rows ops.kv_append_rows leaves in a bf16 cache from the same qkv"""
    B = len(POSITIONS)
    g = torch.Generator().manual_seed(5)
    k8, v8, sc = [torch.empty((B, H, LMAX, n), dtype=t) for n, t in ((HD, torch.uint8), (HD, torch.uint8), (2, torch.float32))]
    for b, n in enumerate(POSITIONS):
        for h in range(H):
            _, k8[b, h], v8[b, h], sc[b, h], _, _ = kc.random_case(n, LMAX, 1000 * b + h)
    qkv = torch.randn((B, 3 * D), generator=g)
    qkv[:, D:] *= 3
    qkv = qkv.bfloat16()
    pos = torch.tensor(POSITIONS, dtype=torch.int32, device="cuda")
    rope = _rope(LMAX)

    def rotate(x):
        kb = torch.zeros((B, H, LMAX, HD), dtype=torch.bfloat16, device="cuda")
        vb = torch.zeros_like(kb)
        xr = x.cuda().clone()
        ops.kv_append_rows(xr, rope.cos, rope.sin, kb, vb, B, H, HD, LMAX, pos)
        torch.cuda.synchronize()
        at = torch.tensor(POSITIONS)
        ar = torch.arange(B)
        return xr.cpu()[:, :D].view(B, H, HD), kb.cpu()[ar, :, at], vb.cpu()[ar, :, at]

    # a power of two per (row, head) on q keeps every |score| <= 8 (exact in bf16, and the rotation is linear)
    qr, kn, vn = rotate(qkv)
    for b, n in enumerate(POSITIONS):
        for h in range(H):
            c, s = ref_kvq.quantize(kn[b, h])
            keys = torch.cat([ref_kvq.dequantize64(k8[b, h, :n], sc[b, h, :n, 0]), ref_kvq.dequantize64(c, s)[None]])
            top = float((keys @ qr[b, h].double()).abs().max()) * kc.SCALE
            e = max(0, int(torch.ceil(torch.log2(torch.tensor(top / 8.0)))))
            qkv[b, h * HD:(h + 1) * HD] *= 2.0 ** -e
    qr, kn, vn = rotate(qkv)
    dev = [t.cuda() for t in (k8, v8, sc)]
    o = torch.full((B, D), NAN, dtype=torch.bfloat16, device="cuda")
    q_dev = qkv.cuda()
    ops.attn_decode_append_rows_fp8(q_dev, rope.cos, rope.sin, *dev, o, B, H, HD, LMAX, kc.SCALE, pos)
    torch.cuda.synchronize()
    assert torch.equal(q_dev.cpu(), qkv), "qkv is left untouched"
    return dict(B=B, qkv=qkv, pos=pos, rope=rope, before=(k8, v8, sc), after=[t.cpu() for t in dev], o=o.cpu(), qr=qr, kn=kn, vn=vn)


def test_decode_appends_quantize_of_the_bf16_row(decode_run):
    """(a) codes and scale bits of the appended row equal quantize() of the row ops.kv_append_rows writes; no other byte changes"""
    r = decode_run
    ek, ev, es = [t.clone() for t in r["before"]]
    for b, n in enumerate(POSITIONS):
        ek[b, :, n], es[b, :, n, 0] = ref_kvq.quantize(r["kn"][b])
        ev[b, :, n], es[b, :, n, 1] = ref_kvq.quantize(r["vn"][b])
    k8, v8, sc = r["after"]
    assert torch.equal(k8, ek), (k8 != ek).nonzero()[:4]
    assert torch.equal(v8, ev), (v8 != ev).nonzero()[:4]
    assert same_f32_bits(sc, es)


def test_decode_output_is_inside_the_bound(decode_run):
    """(b) |o - o64| <= C_REL |o64| + C_ABS max|v^| (kvq_common.py derives the constants) against float64 attention over the exactly
    dequantized cache as read back, the new row included; rows at or past each position hold NaN codes and NaN scales, and the
    output is finite.  Measured on the MI355X: worst 0.930 of the bound (the bf16 rounding of the output; printed)."""
    r = decode_run
    k8, v8, sc = r["after"]
    assert torch.isfinite(r["o"].float()).all()
    worst = 0.0
    for b, n in enumerate(POSITIONS):
        for h in range(H):
            o64 = ref_kvq.attend64(r["qr"][b, h].double() * kc.SCALE, k8[b, h], v8[b, h], sc[b, h], n + 1)
            vmax = float(ref_kvq.dequantize64(v8[b, h, :n + 1], sc[b, h, :n + 1, 1]).abs().max())
            ratio = kc.bound_ratio(r["o"][b, h * HD:(h + 1) * HD], o64, vmax)
            worst = max(worst, ratio)
            assert ratio <= 1.0, (n, h, ratio)
    print(f"fp8 decode: worst |err| / bound = {worst:.3f}")


def test_decode_rows_are_independent(ops, decode_run):
    """(d) the even rows' output bits do not change when the odd rows stand at position 0 over other caches, and the reverse"""
    r = decode_run
    B = r["B"]
    g = torch.Generator().manual_seed(6)
    for keep in (0, 1):
        other = torch.arange(B) % 2 != keep
        k8, v8, sc = [t.clone() for t in r["before"]]
        k8[other] = torch.randint(0, 127, k8[other].shape, generator=g, dtype=torch.int32).to(torch.uint8)
        v8[other] = torch.randint(0, 127, v8[other].shape, generator=g, dtype=torch.int32).to(torch.uint8)
        sc[other] = 0.5
        pos = r["pos"].clone()
        pos[other.cuda()] = 0
        qkv = r["qkv"].clone()
        qkv[other] = torch.randn((int(other.sum()), 3 * D), generator=g).bfloat16()
        o = torch.full((B, D), NAN, dtype=torch.bfloat16, device="cuda")
        ops.attn_decode_append_rows_fp8(qkv.cuda(), r["rope"].cos, r["rope"].sin, k8.cuda(), v8.cuda(), sc.cuda(), o, B, H, HD, LMAX,
                                        kc.SCALE, pos)
        torch.cuda.synchronize()
        assert torch.equal(o.cpu()[~other].view(torch.int16), r["o"][~other].view(torch.int16)), keep


def test_decode_one_hot_probe(ops):
    """(c) 516 keys (the 515 cached ones and the appended one), one (row, head) pair per key i: key i has score 30 -- its codes are
    sign(q) 3.75 / ks_i, so the score is 30 only under ITS K scale -- every other key scores within +-8, and the v of key i
    dequantizes to magnitudes 6 to 12 under ITS V scale, the others' to at most 1.  The output must be that v (to the bf16
    rounding and the e^-22 of weight the others hold): a missing, shifted or doubled key, or a neighbour's scale, moves it by O(1).
    Identity RoPE tables, so that q is the bf16 row as given."""
    n = 516
    pos_v, B = n - 1, n // H
    g = torch.Generator().manual_seed(8)
    j = torch.arange(LMAX)
    ks = torch.exp2(((j * 7) % 6 - 3).float())          # 2^-3 .. 2^2, neighbours differ
    vs = torch.exp2(((j * 5) % 7 - 3).float())          # 2^-3 .. 2^3
    sgn = (torch.randint(0, 2, (B, H, HD), generator=g) * 2 - 1).float()
    u = torch.tensor([0.25, 0.5, 0.75, 1.0])
    pick = lambda shape: u[torch.randint(0, 4, shape, generator=g)] * (torch.randint(0, 2, shape, generator=g) * 2 - 1)
    kval = pick((B, H, LMAX, HD)) / ks[:, None]
    vval = pick((B, H, LMAX, HD)) / vs[:, None]
    w = torch.tensor([6.0, 7.0, 8.0, 10.0, 12.0])[torch.randint(0, 5, (B, H, HD), generator=g)] * \
        (torch.randint(0, 2, (B, H, HD), generator=g) * 2 - 1)
    qkv = torch.zeros((B, 3, H, HD))
    qkv[:, 0] = sgn
    qkv[:, 1] = pick((B, H, HD))
    qkv[:, 2] = pick((B, H, HD))
    for b in range(B):
        for h in range(H):
            i = b * H + h
            if i < pos_v:
                kval[b, h, i] = sgn[b, h] * 3.75 / ks[i]
                vval[b, h, i] = w[b, h] / vs[i]
            else:
                qkv[b, 1, h] = sgn[b, h] * 3.75
                qkv[b, 2, h] = w[b, h]
    k8 = kval.to(ref_kvq.F8)
    v8 = vval.to(ref_kvq.F8)
    assert torch.equal(k8.float(), kval) and torch.equal(v8.float(), vval), "every probe value is a code"
    k8, v8 = k8.view(torch.uint8), v8.view(torch.uint8)
    k8[:, :, pos_v:], v8[:, :, pos_v:] = 0x7F, 0x7F
    sc = torch.stack([ks, vs], -1)[None, None].repeat(B, H, 1, 1).contiguous()
    sc[:, :, pos_v:] = NAN
    dev = [t.contiguous().cuda() for t in (k8, v8, sc)]
    cos = torch.ones((LMAX, HD // 2), device="cuda")
    sin = torch.zeros((LMAX, HD // 2), device="cuda")
    o = torch.full((B, D), NAN, dtype=torch.bfloat16, device="cuda")
    pos = torch.full((B,), pos_v, dtype=torch.int32, device="cuda")
    ops.attn_decode_append_rows_fp8(qkv.view(B, 3 * D).bfloat16().cuda(), cos, sin, *dev, o, B, H, HD, LMAX, kc.SCALE, pos)
    torch.cuda.synchronize()
    k8, v8, sc = [t.cpu() for t in dev]
    o = o.cpu().float().view(B, H, HD)
    for b in range(B):
        for h in range(H):
            i = b * H + h
            want = ref_kvq.dequantize(v8[b, h, i], sc[b, h, i, 1])
            assert (want.abs() >= 5.5).all() and (want.abs() <= 12.5).all()
            assert ((o[b, h] - want).abs() <= 2.0 ** -8 * want.abs() + 1e-4).all(), (i, o[b, h][:4], want[:4])


def test_decode_refusals(ops):
    from midi_model_amd.lib import lib
    from midi_model_amd.ops import _p, _stream
    k8, v8, sc = sentinel_cache(2, H, 8)
    qkv = torch.zeros((2, 3 * D), dtype=torch.bfloat16, device="cuda")
    o = torch.zeros((2, D), dtype=torch.bfloat16, device="cuda")
    pos = torch.zeros(2, dtype=torch.int32, device="cuda")
    rope = _rope(8)
    args = [_p(qkv), _p(rope.cos), _p(rope.sin), _p(k8), _p(v8), _p(sc), _p(o), 2, H, HD, 8, 0.125, _p(pos), 1, _stream()]
    for at, val, match in ((9, 128, "head_dim"), (13, 0, "bf16"), (12, 0, "row_pos is NULL"), (5, 0, "null buffer"), (7, 0, "bad args")):
        a = list(args)
        a[at] = val
        with pytest.raises(RuntimeError, match=match):
            lib().call("mh_attn_decode_append_rows_fp8", *a)
    torch.cuda.synchronize()
    assert (k8 == 0xA5).all() and torch.isnan(sc).all()


# ------------------------------------------------------------------------------------------------------------------- fork
LAYERS, FB, FL = 3, 6, 130


def _fork_caches(dst_rows):
    shape = (LAYERS, FB, H, FL)
    n = LAYERS * FB * H * FL
    k8 = (torch.arange(n * HD, dtype=torch.int64, device="cuda") % 251).to(torch.uint8).view(shape + (HD,))
    v8 = ((torch.arange(n * HD, dtype=torch.int64, device="cuda") * 7 + 3) % 253).to(torch.uint8).view(shape + (HD,))
    sc = torch.arange(n * 2, dtype=torch.int32, device="cuda").view(torch.float32).view(shape + (2,)).clone()
    k8[:, list(dst_rows)], v8[:, list(dst_rows)], sc[:, list(dst_rows)] = 0xA5, 0xA5, NAN
    return k8, v8, sc


def _expect_fork(t, pairs):
    e = t.clone()
    for s, d, n in pairs:
        e[:, d, :, :n] = t[:, s, :, :n]
    return e


@pytest.mark.parametrize("lengths", [(1, 63, 64, 65), (FL, 17, 128, 129)], ids=["1_63_64_65", "Lmax_17_128_129"])
def test_fork_copies_codes_and_scales_and_nothing_else(ops, lengths):
    """pairs (0 -> 1, 0 -> 2, 0 -> 4) and (3 -> 5) in one launch, lengths on both sides of a workgroup's 64 positions: bit-equal
    copies of codes and scale pairs, the sentinels at or past each length and the sources untouched"""
    pairs = [(0, 1, lengths[0]), (0, 2, lengths[1]), (0, 4, lengths[2]), (3, 5, lengths[3])]
    k8, v8, sc = _fork_caches((1, 2, 4, 5))
    ek, ev, es = (_expect_fork(t, pairs) for t in (k8, v8, sc))
    assert not torch.equal(k8, ek)
    ops.kv_fork_rows_fp8(k8, v8, sc, [p[0] for p in pairs], [p[1] for p in pairs], [p[2] for p in pairs])
    torch.cuda.synchronize()
    assert torch.equal(k8, ek) and torch.equal(v8, ev) and same_f32_bits(sc, es)
    for s, d, n in pairs:
        assert (k8[:, d, :, n:] == 0xA5).all() and (v8[:, d, :, n:] == 0xA5).all() and torch.isnan(sc[:, d, :, n:]).all(), d


def test_fork_dropped_pairs_and_refusals(ops):
    from midi_model_amd.lib import lib
    from midi_model_amd.ops import _p, _stream
    k8, v8, sc = _fork_caches((1, 5))
    k0, v0, s0 = k8.clone(), v8.clone(), sc.clone()
    tab = torch.tensor([[-1, 0, 2, FB, 3], [1, -1, 2, 1, FB], [7, 7, 7, 7, 7]], dtype=torch.int32, device="cuda")

    def call(kp, vp, cp, sp, dp, lp, n=5, max_len=7, layers=LAYERS, B_=FB, H_=H, hd=HD, Lmax=FL):
        lib().call("mh_kv_fork_rows_fp8", kp, vp, cp, sp, dp, lp, n, max_len, layers, B_, H_, hd, Lmax, _stream())

    args = (_p(k8), _p(v8), _p(sc), _p(tab[0]), _p(tab[1]), _p(tab[2]))
    call(*args)
    torch.cuda.synchronize()
    assert torch.equal(k8, k0) and torch.equal(v8, v0) and same_f32_bits(sc, s0), "a dropped pair wrote something"
    big = torch.tensor([[3], [5], [1 << 20]], dtype=torch.int32, device="cuda")   # a length past Lmax is cut at Lmax
    call(_p(k8), _p(v8), _p(sc), _p(big[0]), _p(big[1]), _p(big[2]), n=1, max_len=FL)
    torch.cuda.synchronize()
    ek, ev, es = (_expect_fork(t, [(3, 5, FL)]) for t in (k0, v0, s0))
    assert torch.equal(k8, ek) and torch.equal(v8, ev) and same_f32_bits(sc, es)
    for i, name in enumerate(("k8", "v8", "sc", "src", "dst", "len")):
        with pytest.raises(RuntimeError, match=f"{name} is NULL"):
            call(*[0 if jj == i else a for jj, a in enumerate(args)])
    for kw, match in ((dict(hd=8), "head_dim"), (dict(n=0), "0 pairs"), (dict(n=FB + 1), f"{FB + 1} pairs for a cache of {FB}"),
                      (dict(max_len=0), "max_len 0"), (dict(max_len=FL + 1), f"max_len {FL + 1}"), (dict(layers=65536, H_=1), "grid"),
                      (dict(layers=0), "bad args")):
        with pytest.raises(RuntimeError, match=match):
            call(*args, **kw)
    for src, dst, lens, match in (([0], [FB], [3], "outside"), ([0, 3], [1, 1], [3, 3], "twice"), ([0, 1], [1, 2], [3, 3], "at once"),
                                  ([0], [1], [FL + 1], "length"), ([0], [1], [0], "length")):
        with pytest.raises(ValueError, match=match):
            ops.kv_fork_rows_fp8(k8, v8, sc, src, dst, lens)
    torch.cuda.synchronize()
    assert torch.equal(k8, ek) and torch.equal(v8, ev) and same_f32_bits(sc, es)
