"""mh_kv_fork_rows on the MI355X (attention_small.hip): cache sequences copied inside a whole K/V cache [layers, B, H, Lmax, hd] -- what
DecodeSession.fork duplicates a row with.

  1. the copy, exactly: positions [0, len) of every (layer, head) of src bit-equal in dst, every other element of both caches -- the
     sources, the unnamed sequences, positions at or past len of a destination -- keeping its bits; lengths on both sides of what one
     workgroup covers of a run (256 lanes x 16 bytes: 32 positions of 64 bf16, 16 of 64 fp32), 1 and Lmax among them; a fan-out;
  2. hd = 8, and a max_len above every length;
  3. what the kernel drops (an id of -1 or B, src == dst: nothing written, MH_OK) and what the entry point and the wrapper refuse
     before any launch.

Data movement and bit equality: no tolerance anywhere."""
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")
LAYERS, B, H, LMAX, HD = 3, 6, 2, 40, 64
INST = {"bf16": torch.bfloat16, "fp32": torch.float32}


@pytest.fixture(scope="module")
def ops():
    import midi_model_amd.ops as real
    return real


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def caches(shape, dtype, dst_rows):
    """K and V with a bit pattern of its own at every element (bf16: the element index mod 2^16, which differs between the same
    place of any two sequences or layers of these shapes; fp32: the index itself), V's shifted against K's; NaN in ``dst_rows``"""
    n = 1
    for s in shape:
        n *= s
    idx = torch.arange(n, dtype=torch.int32, device="cuda")
    out = []
    for shift in (0, 12345):
        if dtype == torch.bfloat16:
            t = ((idx + shift) % 65536 - 32768).to(torch.int16).view(torch.bfloat16)
        else:
            t = (idx + shift).view(torch.float32)
        t = t.view(shape).clone()
        t[:, list(dst_rows)] = NAN
        out.append(t)
    return out


def expect(k, v, pairs):
    ek, ev = k.clone(), v.clone()
    for s, d, n in pairs:
        ek[:, d, :, :n] = k[:, s, :, :n]
        ev[:, d, :, :n] = v[:, s, :, :n]
    return ek, ev


@pytest.mark.parametrize("lengths", [(1, 33, 40, 17), (32, 16, 31, 15)], ids=["1_33_Lmax_17", "32_16_31_15"])
@pytest.mark.parametrize("inst", list(INST))
def test_fork_copies_every_position_and_nothing_else(ops, inst, lengths):
    """pairs (0 -> 1, 0 -> 2, 0 -> 4) and (3 -> 5) in one launch: bit-equal copies, everything else untouched -- the NaN sentinels at
    or past each length in rows 1, 2, 4, 5, and rows 0 and 3 whole"""
    dtype = INST[inst]
    pairs = [(0, 1, lengths[0]), (0, 2, lengths[1]), (0, 4, lengths[2]), (3, 5, lengths[3])]
    k, v = caches((LAYERS, B, H, LMAX, HD), dtype, (1, 2, 4, 5))
    ek, ev = expect(k, v, pairs)
    assert not same_bits(k, ek) and not same_bits(k, v)
    ops.kv_fork_rows(k, v, [p[0] for p in pairs], [p[1] for p in pairs], [p[2] for p in pairs])
    torch.cuda.synchronize()
    assert same_bits(k, ek) and same_bits(v, ev)
    for s, d, n in pairs:   # (said twice: past its length a destination is all sentinel, when its length leaves anything)
        assert torch.isnan(k[:, d, :, n:].float()).all() and torch.isnan(v[:, d, :, n:].float()).all(), d
        assert not torch.isnan(k[:, d, :, :n].float()).all()


@pytest.mark.parametrize("inst", list(INST))
def test_head_dim_8_device_table_and_a_loose_max_len(ops, inst):
    """hd = 8 (a run of len x 8 elements: a hard-coded 64 would copy the wrong places), the caller's own device table, and, through
    the entry point, a max_len = Lmax above every length: the grid's surplus lanes write nothing"""
    from midi_model_amd.lib import lib
    from midi_model_amd.ops import _p, _stream, dt
    dtype = INST[inst]
    shape = (2, 4, 3, 70, 8)
    pairs = [(2, 0, 70), (2, 3, 5)]
    k, v = caches(shape, dtype, (0, 3))
    ek, ev = expect(k, v, pairs)
    dev = torch.tensor([[2, 2], [0, 3], [70, 5]], dtype=torch.int32, device="cuda")
    ops.kv_fork_rows(k, v, [2, 2], [0, 3], [70, 5], dev=dev)
    torch.cuda.synchronize()
    assert same_bits(k, ek) and same_bits(v, ev)
    k, v = caches(shape, dtype, (0, 3))
    ek, ev = expect(k, v, [(2, 0, 1), (2, 3, 5)])
    dev = torch.tensor([[2, 2], [0, 3], [1, 5]], dtype=torch.int32, device="cuda")
    lib().call("mh_kv_fork_rows", _p(k), _p(v), _p(dev[0]), _p(dev[1]), _p(dev[2]), 2, 70, 2, 4, 3, 8, 70, dt(k), _stream())
    torch.cuda.synchronize()
    assert same_bits(k, ek) and same_bits(v, ev)


def test_dropped_pairs_and_refusals(ops):
    """straight through the entry point: ids -1 and B and src == dst are dropped whole, a length past Lmax is cut at Lmax, MH_OK
    and nothing else written; a null buffer by name, a bad dtype, hd % 8 != 0, n < 1, n > B, max_len outside [1, Lmax] and a grid
    past the launch limits are refused; so is what the wrapper checks on the host.  The caches keep their bits throughout."""
    from midi_model_amd.lib import lib
    from midi_model_amd.ops import _p, _stream, dt
    shape = (LAYERS, B, H, LMAX, HD)
    k, v = caches(shape, torch.bfloat16, (1, 5))
    k0, v0 = k.clone(), v.clone()
    tab = torch.tensor([[-1, 0, 2, B, 3], [1, -1, 2, 1, B], [7, 7, 7, 7, 7]], dtype=torch.int32, device="cuda")

    def call(kp, vp, sp, dp, lp, n=5, max_len=7, layers=LAYERS, B_=B, H_=H, hd=HD, Lmax=LMAX, dtype=dt(k)):
        lib().call("mh_kv_fork_rows", kp, vp, sp, dp, lp, n, max_len, layers, B_, H_, hd, Lmax, dtype, _stream())

    args = (_p(k), _p(v), _p(tab[0]), _p(tab[1]), _p(tab[2]))
    call(*args)
    torch.cuda.synchronize()
    assert same_bits(k, k0) and same_bits(v, v0), "a dropped pair wrote something"
    # a length past Lmax (and past max_len) beside the dropped pairs: row 5 takes row 3's Lmax positions, no more
    big = torch.tensor([[3], [5], [1 << 20]], dtype=torch.int32, device="cuda")
    call(_p(k), _p(v), _p(big[0]), _p(big[1]), _p(big[2]), n=1, max_len=LMAX)
    torch.cuda.synchronize()
    ek, ev = expect(k0, v0, [(3, 5, LMAX)])
    assert same_bits(k, ek) and same_bits(v, ev)
    for i, name in enumerate(("kcache", "vcache", "src", "dst", "len")):
        with pytest.raises(RuntimeError, match=f"{name} is NULL"):
            call(*[0 if j == i else a for j, a in enumerate(args)])
    for kw, match in ((dict(dtype=7), "bad dtype"), (dict(hd=12), "multiple of 8"), (dict(hd=0), "multiple of 8"),
                      (dict(n=0), "0 pairs"), (dict(n=B + 1), f"{B + 1} pairs for a cache of {B}"), (dict(max_len=0), "max_len 0"),
                      (dict(max_len=LMAX + 1), f"max_len {LMAX + 1}"), (dict(layers=65536, H_=1), "grid"),
                      (dict(layers=0), "bad args")):
        with pytest.raises(RuntimeError, match=match):
            call(*args, **kw)
    for src, dst, lens, match in (([0], [B], [3], "outside"), ([-1], [1], [3], "outside"), ([0, 3], [1, 1], [3, 3], "twice"),
                                  ([0, 1], [1, 2], [3, 3], "at once"), ([2], [2], [3], "at once"), ([0], [1], [LMAX + 1], "length"),
                                  ([0], [1], [0], "length"), ([0], [1, 2], [3], "destinations")):
        with pytest.raises(ValueError, match=match):
            ops.kv_fork_rows(k, v, src, dst, lens)
    torch.cuda.synchronize()
    assert same_bits(k, ek) and same_bits(v, ev)
