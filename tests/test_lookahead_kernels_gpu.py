"""The attention pair of a lookahead session (mh_kv_append_rows_via, mh_attn_decode_rows_via; attention_small.hip): the per-row K/V
append and decode attention THROUGH A ROW MAP -- row b at position row_pos[b] of cache sequence row_cache[b], the rows of a group on
one sequence, -1 (or any value outside the cache) for a row that sits the step out.  The yardstick is the pair they generalise:
mh_kv_append_rows + mh_attn_decode_rows.  Whole buffers are compared through integer views, poisoned with NaN first, so what must not
be read or written is checked with what must.

Shapes: H = 3, B = 9 rows, caches of 4 sequences, capacity 600; bf16 and fp32, head_dim 64.  Key counts: every count of
test_cache_attention_gpu.decode_lengths for attn_decode_kernel<64> (the loop's round, its step, the exits behind either register set,
+-1) that fits the capacity -- bf16's count above 8 steps, 1059 keys, does not and stays with that file -- which includes position 0."""
import pytest
import torch

from test_cache_attention_gpu import DECODE_BOUND, DECODE_INST, F64, NAN, bits, decode_lengths, grnd, same_bits

pytestmark = pytest.mark.gpu

H, B, NC, LMAX, HD, SCALE = 3, 9, 4, 600, 64, 0.125
D = H * HD
# the one-hot probe's score.  Twice test_cache_attention_gpu.SPIKE: the spike keys of the OTHER rows of a group are long keys too (|k| =
# SPIKE / (scale |q|)), and against a foreign q they score SPIKE N(0, 1) / 8 -- at 60 the margin of 20 holds to five sigma
LSPIKE = 60.0
INSTS = ["bf16_hd64", "fp32_hd64"]
# the test map: a group of 4 rows on cache sequence 0, a group of 2 on sequence 1, a single row on sequence 2, two inactive rows (-1,
# and the first value past the cache); sequence 3 belongs to no row.  Rows and sequences are deliberately not in step.
ROW_CACHE = [1, 1, 0, 0, 0, 0, -1, 2, NC]
GROUP4, GROUP2, SINGLE, INACTIVE = (2, 3, 4, 5), (0, 1), (7,), (6, 8)


@pytest.fixture(scope="module")
def ops():
    import midi_model_amd.ops as real
    return real


@pytest.fixture(scope="module")
def tab():
    from midi_model_amd.engine import RopeTable
    return RopeTable(HD, 10000.0, "cuda", LMAX + 1)


def _i32(x):
    return torch.tensor(list(x), dtype=torch.int32, device="cuda")


def _positions(length):
    """row positions for one key count: the group of 4 at consecutive positions from length - 1, the group of 2 likewise, the single
    row at length - 1; the inactive rows anywhere"""
    p = length - 1
    pos = [0] * B
    for j, b in enumerate(GROUP4):
        pos[b] = p + j
    for j, b in enumerate(GROUP2):
        pos[b] = p + j
    pos[SINGLE[0]] = p
    pos[INACTIVE[0]], pos[INACTIVE[1]] = 5, 7
    return pos


def _caches(dtype, n, filled, seed):
    """K and V caches of n sequences: rows [0, filled[c]) random, everything else NaN"""
    kc = torch.full((n, H, LMAX, HD), NAN, dtype=dtype, device="cuda")
    vc = torch.full_like(kc, NAN)
    for c, f in enumerate(filled):
        if f:
            kc[c, :, :f] = grnd((H, f, HD), dtype, seed + c)
            vc[c, :, :f] = grnd((H, f, HD), dtype, seed + 50 + c)
    return kc, vc


def _pair_via(ops, tab, qkv, kc, vc, pos, cache):
    """the pair on clones -> (qkv after, kc after, vc after, o)"""
    q, k, v = qkv.clone(), kc.clone(), vc.clone()
    o = torch.full((qkv.shape[0], D), NAN, dtype=qkv.dtype, device="cuda")
    n = qkv.shape[0]
    ops.kv_append_rows_via(q, tab.cos, tab.sin, k, v, n, H, HD, LMAX, pos, cache)
    ops.attn_decode_rows_via(q, k, v, o, n, H, HD, LMAX, SCALE, pos, cache)
    return q, k, v, o


@pytest.mark.parametrize("inst", INSTS)
def test_the_identity_map_is_the_existing_pair(ops, tab, inst):
    """row_cache = 0..B-1 on caches of B sequences: qkv, both caches and o bit-equal to mh_kv_append_rows + mh_attn_decode_rows on the
    whole batch, at positions on the loop's edges"""
    dtype, _, kpw = DECODE_INST[inst]
    lens = [x for x in decode_lengths(kpw, False) if x <= LMAX]
    for n, l0 in enumerate(range(0, len(lens), 3)):
        pos_h = [lens[(l0 + b) % len(lens)] - 1 for b in range(B)]
        qkv = grnd((B, 3 * D), dtype, 10 + n)
        kc, vc = _caches(dtype, B, pos_h, 100 * n)
        pos, ident = _i32(pos_h), _i32(range(B))
        q1, k1, v1, o1 = _pair_via(ops, tab, qkv, kc, vc, pos, ident)
        q2, k2, v2 = qkv.clone(), kc.clone(), vc.clone()
        o2 = torch.full((B, D), NAN, dtype=dtype, device="cuda")
        ops.kv_append_rows(q2, tab.cos, tab.sin, k2, v2, B, H, HD, LMAX, pos)
        ops.attn_decode_rows(q2, k2, v2, o2, B, H, HD, LMAX, SCALE, pos)
        for name, a, b in (("qkv", q1, q2), ("k cache", k1, k2), ("v cache", v1, v2), ("o", o1, o2)):
            assert same_bits(a, b), f"positions {pos_h}: {name} differs at {(bits(a) != bits(b)).nonzero()[:4].tolist()}"
        assert torch.isfinite(o1.float()).all()


@pytest.mark.parametrize("inst", INSTS)
def test_groups_share_a_cache_sequence(ops, tab, inst):
    """the test map at every key count: for every active row, the cache row it wrote, the rotated q and k it left in qkv and its o are
    bit-equal to the existing pair run at B = 1 on a copy of its cache sequence after the group's appends (its own row poisoned
    first: the existing append must write it back); the inactive rows' o is zero and their qkv untouched; no other byte of any cache
    changes -- sequence 3, which no row names, included"""
    dtype, _, kpw = DECODE_INST[inst]
    cache = _i32(ROW_CACHE)
    for length in [x for x in decode_lengths(kpw, False) if x + 3 <= LMAX]:
        pos_h = _positions(length)
        pos = _i32(pos_h)
        qkv = grnd((B, 3 * D), dtype, 1000 + length)
        kc, vc = _caches(dtype, NC, [length - 1, length - 1, length - 1, 0], 2000 + length)
        q, k, v, o = _pair_via(ops, tab, qkv, kc, vc, pos, cache)
        want_k, want_v = kc.clone(), vc.clone()
        for b in range(B):
            c, p = ROW_CACHE[b], pos_h[b]
            if b in INACTIVE:
                assert same_bits(o[b], torch.zeros_like(o[b])), f"len {length}: inactive row {b}: o is not zero"
                assert same_bits(q[b], qkv[b]), f"len {length}: inactive row {b}: qkv was written"
                continue
            q1 = qkv[b:b + 1].clone()
            k1, v1 = k[c:c + 1].clone(), v[c:c + 1].clone()
            k1[:, :, p], v1[:, :, p] = NAN, NAN
            o1 = torch.full((1, D), NAN, dtype=dtype, device="cuda")
            ops.kv_append_rows(q1, tab.cos, tab.sin, k1, v1, 1, H, HD, LMAX, pos[b:b + 1].contiguous())
            ops.attn_decode_rows(q1, k1, v1, o1, 1, H, HD, LMAX, SCALE, pos[b:b + 1].contiguous())
            assert same_bits(k1[0, :, p], k[c, :, p]) and same_bits(v1[0, :, p], v[c, :, p]), f"len {length}: row {b}: the cache row it wrote"
            assert same_bits(k1, k[c:c + 1]) and same_bits(v1, v[c:c + 1])
            assert same_bits(q1[0], q[b]), f"len {length}: row {b}: the rotated q and k left in qkv"
            assert same_bits(o1[0], o[b]), f"len {length}: row {b} at {p} of sequence {c}: o differs"
            assert torch.isfinite(o[b].float()).all(), f"len {length}: row {b}: a poisoned key was read"
            want_k[c, :, p], want_v[c, :, p] = k[c, :, p], v[c, :, p]
        assert same_bits(k, want_k) and same_bits(v, want_v), f"len {length}: a cache byte outside the rows' own positions changed"


def _rot(x, tab, p, dtype, inverse=False):
    """the kernels' rotation at position p in float64 on the table values as they read them (rounded to dtype)"""
    c, s = tab.cos[p].to(dtype).to(F64), tab.sin[p].to(dtype).to(F64)
    if inverse:
        s = -s
    x1, x2 = x[..., :HD // 2], x[..., HD // 2:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)


@pytest.mark.parametrize("inst", INSTS)
@pytest.mark.parametrize("d", [1, 2, 3])
def test_one_hot_probe_across_the_rows_of_a_group(ops, tab, inst, d):
    """the group of 4 at positions p .. p + 3 of one sequence, p at a step edge.  Head 0 of row j >= d: the key that row j - d of the
    group appends IN THIS LAUNCH PAIR scores 60 against row j's q (>= 20 above every other) and carries a v of magnitude 6..12 that
    no other key holds, so row j's output must be that v: a row that misses the keys its group stored below it is off by O(1).
    Head 1 of every row: the spike is the row's own key.  Head 2 of row j < 3: the spike is the key row j + 1 appends, one ABOVE row
    j's position, with a v of 50: it must not be reached, so o stays on the float64 reference over keys [0, p + j] (the decode bound of
    test_cache_attention_gpu.py); reaching it moves o by O(50)."""
    dtype, _, kpw = DECODE_INST[inst]
    c_rel, c_abs = DECODE_BOUND[dtype]
    for p in (0, 16 * kpw - 2, 2 * 16 * kpw):
        pos_h = _positions(p + 1)
        pos, cache = _i32(pos_h), _i32(ROW_CACHE)
        qkv = grnd((B, 3 * D), dtype, 300 + p + d)
        kc, vc = _caches(dtype, NC, [p, p, p, 0], 400 + p)
        view = qkv.view(B, 3, H, HD)   # [row, q|k|v, head, hd]
        probes, hidden = [], []

        def spike_key(j_q, h, j_k):
            """the unrotated k of (row j_k, head h) := the key that scores SPIKE against the rotated q of (row j_q, head h)"""
            bq, bk = GROUP4[j_q], GROUP4[j_k]
            q_rot = _rot(view[bq, 0, h].to(F64), tab, pos_h[bq], dtype).to(dtype).to(F64)   # (the kernel rounds the rotated q)
            alpha = LSPIKE / (SCALE * (q_rot * q_rot).sum())
            view[bk, 1, h] = _rot(alpha * q_rot, tab, pos_h[bk], dtype, inverse=True).to(dtype)

        for j in range(4):
            e = torch.arange(HD, device="cuda")
            sv = ((6.0 + (3 * j + e) % 7) * (1.0 - 2.0 * (j % 2))).to(dtype)
            if j >= d:                      # head 0: the key of row j - d, stored in this pair
                spike_key(j, 0, j - d)
                view[GROUP4[j - d], 2, 0] = sv
                probes.append((j, 0, sv))
        for j in range(4):                  # head 1: the row's own key
            e = torch.arange(HD, device="cuda")
            sv = ((6.0 + (5 * j + e) % 7) * (2.0 * (j % 2) - 1.0)).to(dtype)
            spike_key(j, 1, j)
            view[GROUP4[j], 2, 1] = sv
            probes.append((j, 1, sv))
        for j in range(3):                  # head 2: the key ABOVE row j, which row j + 1 stores
            spike_key(j, 2, j + 1)
            view[GROUP4[j + 1], 2, 2] = 50.0
            hidden.append(j)
        q, k, v, o = _pair_via(ops, tab, qkv, kc, vc, pos, cache)
        assert torch.isfinite(o[list(GROUP4)].float()).all()
        seq = ROW_CACHE[GROUP4[0]]
        for j, h, sv in probes:
            b = GROUP4[j]
            got, want = o[b].view(H, HD)[h].to(F64), sv.to(F64)
            # the set-up holds: the spike is the maximum of row j's scores over the keys it may read, by >= 20
            sc = (k[seq, h, :pos_h[b] + 1].to(F64) @ q[b].view(3, H, HD)[0, h].to(F64)) * SCALE
            top = sc.topk(min(2, len(sc)))
            want_key = pos_h[b] - (d if h == 0 else 0)
            assert int(top.indices[0]) == want_key and (len(sc) == 1 or float(top.values[0] - top.values[1]) >= 20), \
                f"probe set-up: row {j} head {h}: maximum at key {int(top.indices[0])}, wanted {want_key}"
            vmax = v[seq, h, :pos_h[b] + 1].to(F64).abs().max()
            bound = c_rel * want.abs() + c_abs * vmax
            assert ((got - want).abs() <= bound).all(), \
                f"p {p}: row {j} head {h} misses the key its group stored at position {want_key}: err {(got - want).abs().max():.3g}"
        for j in hidden:
            b = GROUP4[j]
            n = pos_h[b] + 1   # the keys row j may read; the spike sits at key n
            q2 = q[b].view(3, H, HD)[0, 2].to(F64)
            assert float((k[seq, 2, n].to(F64) @ q2) * SCALE) >= 50 and float(v[seq, 2, n].to(F64).abs().min()) == 50.0, "probe set-up"
            k64, v64 = k[seq, 2, :n].to(F64), v[seq, 2, :n].to(F64)
            ref = torch.softmax((k64 @ q2) * SCALE, -1) @ v64
            got = o[b].view(H, HD)[2].to(F64)
            bound = c_rel * ref.abs() + c_abs * v64.abs().max()
            assert ((got - ref).abs() <= bound).all(), \
                f"p {p}: row {j} reached the key above its position: off the reference over keys [0, {n - 1}] by {(got - ref).abs().max():.3g}"


def test_refusals(ops, tab):
    """the entry points' own refusals (MH_ERR_ARG -> RuntimeError) and the wrappers' (ValueError), nothing launched, nothing written"""
    from midi_model_amd.lib import lib
    from midi_model_amd.ops import _p, _stream, dt
    qkv = grnd((B, 3 * D), torch.bfloat16, 1)
    kc, vc = _caches(torch.bfloat16, NC, [4, 4, 4, 4], 2)
    o = torch.full((B, D), NAN, dtype=torch.bfloat16, device="cuda")
    pos, cache = _i32([3] * B), _i32(ROW_CACHE)
    keep = [t.clone() for t in (qkv, kc, vc, o)]

    def append(B_=B, H_=H, hd=HD, Lmax=LMAX, pos_=pos, cache_=cache, n=NC, q=qkv, dtype=None):
        lib().call("mh_kv_append_rows_via", _p(q), _p(tab.cos), _p(tab.sin), _p(kc), _p(vc), B_, H_, hd, Lmax, _p(pos_), _p(cache_), n,
                   dt(qkv) if dtype is None else dtype, _stream())

    def attend(B_=B, H_=H, hd=HD, Lmax=LMAX, pos_=pos, cache_=cache, n=NC, q=qkv, dtype=None):
        lib().call("mh_attn_decode_rows_via", _p(q), _p(kc), _p(vc), _p(o), B_, H_, hd, Lmax, SCALE, _p(pos_), _p(cache_), n,
                   dt(qkv) if dtype is None else dtype, _stream())

    for call in (append, attend):
        for kw, match in ((dict(hd=128), "head_dim"), (dict(hd=256), "head_dim"), (dict(dtype=7), "dtype"), (dict(pos_=None), "row_pos"),
                          (dict(cache_=None), "row_cache"), (dict(n=0), "n_cache"), (dict(n=65536), "n_cache"), (dict(B_=0), "bad args"),
                          (dict(B_=65536), "bad args"), (dict(Lmax=0), "bad args"), (dict(Lmax=1 << 24), "bad args"), (dict(H_=0), "bad args"),
                          (dict(q=None), "null buffer")):
            with pytest.raises(RuntimeError, match=match):
                call(**kw)
    for args, match in (((qkv, tab.cos, tab.sin, kc, vc, B, H, HD, LMAX, pos, None), "row_cache"),
                        ((qkv, tab.cos, tab.sin, kc, vc, B, H, HD, LMAX, pos, cache.long()), "row_cache"),
                        ((qkv, tab.cos, tab.sin, kc, vc, B, H, HD, LMAX, pos[:4], cache), "row_pos"),
                        ((qkv, tab.cos, tab.sin, kc, vc, B, H, HD, LMAX, pos.cpu(), cache), "row_pos"),
                        ((qkv, tab.cos, tab.sin, kc, vc.float(), B, H, HD, LMAX, pos, cache), "whole sequences"),
                        ((qkv, tab.cos, tab.sin, kc, vc, B, H, HD, LMAX - 1, pos, cache), "whole sequences"),
                        ((qkv[:, :-HD], tab.cos, tab.sin, kc, vc, B, H, HD, LMAX, pos, cache), "qkv")):
        with pytest.raises(ValueError, match=match):
            ops.kv_append_rows_via(*args)
    with pytest.raises(ValueError, match="o \\["):
        ops.attn_decode_rows_via(qkv, kc, vc, o.float(), B, H, HD, LMAX, SCALE, pos, cache)
    torch.cuda.synchronize()
    for t, t0 in zip((qkv, kc, vc, o), keep):
        assert same_bits(t, t0), "a refused call wrote"
