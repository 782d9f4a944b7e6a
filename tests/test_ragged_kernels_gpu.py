"""The four entry points of generate_ragged on the MI355X (attention_small.hip):

  1. the per-row decode forms (mh_kv_append_rows, mh_attn_decode_rows, mh_attn_decode_append_rows) against the uniform entry points,
     bit for bit: one launch whose rows stand at every position that straddles the key loop's rounds, steps and exits;
  2. the packed K/V store mh_kv_store_seqs, exactly;
  3. what the entry points refuse, with values the host can check.

Data movement and bit equality: no tolerance anywhere."""
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")
H, HD, LMAX = 3, 64, 1152
# (dtype) -> KPW, keys per wave per round of attn_decode_kernel at head_dim 64 (test_cache_attention_gpu.py, DECODE_INST)
INST = {"bf16": (torch.bfloat16, 8), "fp32": (torch.float32, 4)}


@pytest.fixture(scope="module")
def ops():
    import midi_model_amd.ops as real
    return real


def decode_lengths(kpw, append):
    """test_cache_attention_gpu.py's list, restated: key counts around the loop's round (4 KPW), step (16 KPW), the exits after
    register sets A and B, 3 steps + 1 and one count above 8 steps; APPEND walks len - 1 cached keys: every boundary + 1 as well"""
    rd, st = 4 * kpw, 16 * kpw
    ls = {1, rd - 1, rd, rd + 1, st - 1, st, st + 1, 2 * st - 1, 2 * st, 2 * st + 1, 3 * st + 1, 8 * st + rd + 3}
    if append:
        ls |= {x + 1 for x in ls}
    return sorted(x for x in ls if x >= 1)


def grnd(shape, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(shape, generator=g, device="cuda").to(dtype)


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


@pytest.mark.parametrize("order", ["ascending", "shuffled"])
@pytest.mark.parametrize("append", [False, True], ids=["append_then_decode", "fused_append"])
@pytest.mark.parametrize("inst", list(INST))
def test_rows_forms_equal_the_uniform_entry_points_bit_for_bit(ops, inst, append, order):
    """ONE launch of the per-row form with row b at position len_b - 1, len over decode_lengths (1, 2, a round +- 1, a step +- 1,
    two steps +- 1, ..., 1059 in bf16), ascending and in a fixed shuffled order; per b, the uniform entry point at pos = row_pos[b]
    on copies of the same inputs.  Row b of ``o``, the rotated q and k left in qkv (kv_append_rows), and the one cache row written
    have identical bits; every other cache row keeps its bits (rows at or past row_pos[b] hold NaN before the launch, so a key
    read too many poisons the output, which must be finite)."""
    from midi_model_amd.engine import RopeTable
    dtype, kpw = INST[inst]
    lens = decode_lengths(kpw, append)
    assert 1 in lens and (2 in lens or not append) and 8 * 16 * kpw + 4 * kpw + 3 in lens and max(lens) <= LMAX
    if order == "shuffled":
        perm = torch.randperm(len(lens), generator=torch.Generator().manual_seed(7)).tolist()
        lens = [lens[i] for i in perm]
    B, D, scale = len(lens), H * HD, HD ** -0.5
    pos_host = [n - 1 for n in lens]
    row_pos = torch.tensor(pos_host, dtype=torch.int32, device="cuda")
    tab = RopeTable(HD, 10000.0, "cuda", LMAX + 1)
    qkv0 = grnd((B, 3 * D), dtype, 1)
    kc0 = torch.full((B, H, LMAX, HD), NAN, dtype=dtype, device="cuda")
    vc0 = torch.full((B, H, LMAX, HD), NAN, dtype=dtype, device="cuda")
    kr, vr = grnd((B, H, LMAX, HD), dtype, 2), grnd((B, H, LMAX, HD), dtype, 3)
    for b, p in enumerate(pos_host):  # rows [0, pos) are cached; row pos is the one this step writes
        kc0[b, :, :p], vc0[b, :, :p] = kr[b, :, :p], vr[b, :, :p]
    del kr, vr
    qkv, kc, vc = qkv0.clone(), kc0.clone(), vc0.clone()
    o = torch.full((B, D), NAN, dtype=dtype, device="cuda")
    if append:
        ops.attn_decode_append_rows(qkv, tab.cos, tab.sin, kc, vc, o, B, H, HD, LMAX, scale, row_pos)
        assert same_bits(qkv, qkv0), "the fused form leaves qkv untouched"
    else:
        ops.kv_append_rows(qkv, tab.cos, tab.sin, kc, vc, B, H, HD, LMAX, row_pos)
        ops.attn_decode_rows(qkv, kc, vc, o, B, H, HD, LMAX, scale, row_pos)
        assert same_bits(qkv[:, 2 * D:], qkv0[:, 2 * D:]), "v is not rotated"
    torch.cuda.synchronize()
    assert torch.isfinite(o.float()).all(), "a row read a key at or past its position"
    expect_k, expect_v = kc0.clone(), vc0.clone()
    for b, p in enumerate(pos_host):
        qu, ku, vu = qkv0.clone(), kc0.clone(), vc0.clone()
        ou = torch.full((B, D), NAN, dtype=dtype, device="cuda")
        if append:
            ops.attn_decode_append(qu, tab.cos, tab.sin, ku, vu, ou, B, H, HD, LMAX, p, scale)
        else:
            ops.kv_append(qu, tab.cos, tab.sin, ku, vu, B, H, HD, LMAX, p)
            ops.attn_decode(qu, ku, vu, ou, B, H, HD, LMAX, p + 1, scale)
            assert same_bits(qkv[b, :2 * D], qu[b, :2 * D]), (b, p, "rotated q / k left in qkv")
        assert same_bits(o[b], ou[b]), (b, p, "attention output")
        assert same_bits(kc[b, :, p], ku[b, :, p]) and same_bits(vc[b, :, p], vu[b, :, p]), (b, p, "the cache row written")
        expect_k[b, :, p], expect_v[b, :, p] = ku[b, :, p], vu[b, :, p]
    assert same_bits(kc, expect_k) and same_bits(vc, expect_v), "a cache row other than row_pos[b] changed"


@pytest.mark.parametrize("inst", list(INST))
def test_kv_store_seqs_moves_every_row_and_nothing_else(ops, inst):
    """sequences of (1, 5, 64, 127, 128, 130) rows laid end to end: packed row m of sequence s lands in cache row m - start_s of
    (s, h), exactly, and every other cache row keeps its sentinel bits.  (The kernel's grid is not capped: one lane per 16
    bytes, no grid-stride loop to pass.)"""
    dtype, _ = INST[inst]
    lengths = (1, 5, 64, 127, 128, 130)
    n, M, D, Lmax = len(lengths), sum(lengths), H * HD, 131
    plan = ops.attn_seq_plan(lengths, H).upload("cuda")
    qkv = grnd((M, 3 * D), dtype, 4)
    kc = torch.full((n, H, Lmax, HD), NAN, dtype=dtype, device="cuda")
    vc = torch.full((n, H, Lmax, HD), NAN, dtype=dtype, device="cuda")
    ek, ev = kc.clone(), vc.clone()
    ops.kv_store_seqs(qkv, plan, kc, vc, H, HD, Lmax)
    a = 0
    for s, L in enumerate(lengths):
        ek[s, :, :L] = qkv[a:a + L, D:2 * D].view(L, H, HD).transpose(0, 1)
        ev[s, :, :L] = qkv[a:a + L, 2 * D:].view(L, H, HD).transpose(0, 1)
        a += L
    assert same_bits(kc, ek) and same_bits(vc, ev)


def test_refusals(ops):
    """hd 256, a null row_pos and a length above Lmax come back as errors with a message, and nothing is launched (the buffers
    keep their sentinels).  Only values the host can check are passed: no out-of-range device position."""
    from midi_model_amd.lib import lib
    from midi_model_amd.ops import _p, _stream, dt
    from midi_model_amd.engine import RopeTable
    B, Lmax = 2, 8
    tab = RopeTable(HD, 10000.0, "cuda", Lmax)
    row_pos = torch.zeros(B, dtype=torch.int32, device="cuda")

    def buffers(hd):
        return (torch.full((B, 3 * H * hd), 1.0, device="cuda"), torch.full((B, H, Lmax, hd), 2.0, device="cuda"),
                torch.full((B, H, Lmax, hd), 3.0, device="cuda"), torch.full((B, H * hd), 4.0, device="cuda"))

    def untouched(t):
        torch.cuda.synchronize()
        q, k, v, o = t
        return bool((q == 1).all() and (k == 2).all() and (v == 3).all() and (o == 4).all())

    t = q, k, v, o = buffers(256)
    tab256 = RopeTable(256, 10000.0, "cuda", Lmax)
    with pytest.raises(RuntimeError, match="head_dim 256 unsupported"):
        ops.kv_append_rows(q, tab256.cos, tab256.sin, k, v, B, H, 256, Lmax, row_pos)
    with pytest.raises(RuntimeError, match="head_dim 256 unsupported"):
        ops.attn_decode_rows(q, k, v, o, B, H, 256, Lmax, 0.0625, row_pos)
    with pytest.raises(RuntimeError, match="head_dim 256 unsupported"):
        ops.attn_decode_append_rows(q, tab256.cos, tab256.sin, k, v, o, B, H, 256, Lmax, 0.0625, row_pos)
    assert untouched(t)
    t = q, k, v, o = buffers(HD)
    with pytest.raises(RuntimeError, match="row_pos is NULL"):
        lib().call("mh_kv_append_rows", _p(q), _p(tab.cos), _p(tab.sin), _p(k), _p(v), B, H, HD, Lmax, 0, dt(q), _stream())
    with pytest.raises(RuntimeError, match="row_pos is NULL"):
        lib().call("mh_attn_decode_rows", _p(q), _p(k), _p(v), _p(o), B, H, HD, Lmax, 0.125, 0, dt(q), _stream())
    with pytest.raises(RuntimeError, match="row_pos is NULL"):
        lib().call("mh_attn_decode_append_rows", _p(q), _p(tab.cos), _p(tab.sin), _p(k), _p(v), _p(o), B, H, HD, Lmax, 0.125, 0,
                   dt(q), _stream())
    assert untouched(t)
    # one sequence of Lmax + 1 rows: the wrapper refuses it from the plan's lengths, the entry point from M > n * Lmax
    plan = ops.attn_seq_plan([Lmax + 1], H).upload("cuda")
    rows = torch.full((Lmax + 1, 3 * H * HD), 1.0, device="cuda")
    with pytest.raises(ValueError, match="rows in a cache"):
        ops.kv_store_seqs(rows, plan, k[:1], v[:1], H, HD, Lmax)
    with pytest.raises(RuntimeError, match="exceeds Lmax"):
        lib().call("mh_kv_store_seqs", _p(rows), _p(plan.seq_start), _p(k), _p(v), 1, Lmax + 1, H, HD, Lmax, dt(rows), _stream())
    assert untouched(t)
