"""mh_kv_store_seqs_rows on the MI355X (attention_small.hip): the packed K/V store into CHOSEN sequences of a cache in use --
what DecodeSession.admit lands a prefill with.

  1. scatter, exactly: every moved row bit-equal to its source, every other cache element -- the unnamed sequences, rows at or past
     a named sequence's length -- keeping its sentinel bits; once with lengths around the 64 / 128 marks, once with a launch whose
     last workgroup is partial and a sequence as long as the cache;
  2. rows = arange(n), B = n: both caches bit-equal to mh_kv_store_seqs on the same inputs;
  3. what the entry point and the wrapper refuse, before any launch.

Data movement and bit equality: no tolerance anywhere."""
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")
H, HD = 16, 64
INST = {"bf16": torch.bfloat16, "fp32": torch.float32}


@pytest.fixture(scope="module")
def ops():
    import midi_model_amd.ops as real
    return real


def grnd(shape, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(shape, generator=g, device="cuda").to(dtype)


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def sentinel_caches(B, Lmax, dtype):
    return (torch.full((B, H, Lmax, HD), NAN, dtype=dtype, device="cuda"), torch.full((B, H, Lmax, HD), NAN, dtype=dtype, device="cuda"))


@pytest.mark.parametrize("lengths, Lmax, B, rows", [
    ((1, 5, 64, 127, 128, 130), 131, 9, (7, 0, 4, 2, 8, 5)),
    ((1, 5, 3), 5, 4, (3, 0, 2)),   # a length equal to Lmax, a length of 1; bf16: 9 x 16 x 8 = 1152 lanes = 4.5 workgroups
], ids=["six_into_nine", "partial_last_workgroup"])
@pytest.mark.parametrize("inst", list(INST))
def test_scatter_moves_every_row_and_nothing_else(ops, inst, lengths, Lmax, B, rows):
    """packed row m of sequence s lands in cache row m - start_s of (rows[s], h), exactly; every other element of both caches --
    the B - n unnamed sequences whole, rows >= L_s of the named ones -- keeps its NaN sentinel bits"""
    dtype = INST[inst]
    M, D = sum(lengths), H * HD
    plan = ops.attn_seq_plan(lengths, H).upload("cuda")
    qkv = grnd((M, 3 * D), dtype, 4)
    kc, vc = sentinel_caches(B, Lmax, dtype)
    ek, ev = kc.clone(), vc.clone()
    ops.kv_store_seqs_rows(qkv, plan, rows, kc, vc, H, HD, Lmax)
    torch.cuda.synchronize()
    a = 0
    for r, L in zip(rows, lengths):
        ek[r, :, :L] = qkv[a:a + L, D:2 * D].view(L, H, HD).transpose(0, 1)
        ev[r, :, :L] = qkv[a:a + L, 2 * D:].view(L, H, HD).transpose(0, 1)
        a += L
    assert same_bits(kc, ek) and same_bits(vc, ev)
    for r in set(range(B)) - set(rows):   # (said twice: the unnamed sequences are all sentinel)
        assert torch.isnan(kc[r].float()).all() and torch.isnan(vc[r].float()).all(), r


@pytest.mark.parametrize("inst", list(INST))
def test_identity_rows_equal_kv_store_seqs(ops, inst):
    dtype = INST[inst]
    lengths, Lmax = (1, 5, 64, 127, 128, 130), 131
    n, M, D = len(lengths), sum(lengths), H * HD
    plan = ops.attn_seq_plan(lengths, H).upload("cuda")
    qkv = grnd((M, 3 * D), dtype, 5)
    kc, vc = sentinel_caches(n, Lmax, dtype)
    k0, v0 = sentinel_caches(n, Lmax, dtype)
    ops.kv_store_seqs(qkv, plan, k0, v0, H, HD, Lmax)
    ops.kv_store_seqs_rows(qkv, plan, list(range(n)), kc, vc, H, HD, Lmax)
    torch.cuda.synchronize()
    assert same_bits(kc, k0) and same_bits(vc, v0)


def test_refusals(ops):
    """a null rows, n > B, M > n * Lmax and a bad dtype at the entry point; a row id outside [0, B), a repeated row id and a length
    above Lmax at the wrapper: all come back as errors with a message, and nothing is launched (the caches keep their values)"""
    from midi_model_amd.lib import lib
    from midi_model_amd.ops import _p, _stream, dt
    B, Lmax, D = 3, 8, H * HD
    lengths = (2, 8)
    plan = ops.attn_seq_plan(lengths, H).upload("cuda")
    qkv = torch.full((10, 3 * D), 1.0, device="cuda")
    k, v = torch.full((B, H, Lmax, HD), 2.0, device="cuda"), torch.full((B, H, Lmax, HD), 3.0, device="cuda")
    rows = torch.tensor([2, 0], dtype=torch.int32, device="cuda")

    def call(rows_p, n, B_, M, Lmax_, dtype):
        lib().call("mh_kv_store_seqs_rows", _p(qkv), _p(plan.seq_start), rows_p, _p(k), _p(v), n, B_, M, H, HD, Lmax_, dtype, _stream())

    with pytest.raises(RuntimeError, match="rows is NULL"):
        call(0, 2, B, 10, Lmax, dt(qkv))
    with pytest.raises(RuntimeError, match="2 sequences for a cache of 1"):
        call(_p(rows), 2, 1, 10, Lmax, dt(qkv))
    with pytest.raises(RuntimeError, match="exceeds Lmax"):
        call(_p(rows), 2, B, 10, 4, dt(qkv))
    with pytest.raises(RuntimeError, match="bad dtype"):
        call(_p(rows), 2, B, 10, Lmax, 7)
    for bad, match in (((2, 3), "outside"), ((-1, 0), "outside"), ((1, 1), "twice"), ((1,), "cache rows for")):
        with pytest.raises(ValueError, match=match):
            ops.kv_store_seqs_rows(qkv, plan, bad, k, v, H, HD, Lmax)
    long = ops.attn_seq_plan((2, Lmax + 1), H).upload("cuda")
    with pytest.raises(ValueError, match="rows in a cache"):
        ops.kv_store_seqs_rows(torch.full((Lmax + 3, 3 * D), 1.0, device="cuda"), long, (2, 0), k, v, H, HD, Lmax)
    torch.cuda.synchronize()
    assert bool((k == 2).all() and (v == 3).all())
