"""The two kernels of decode attention over prefix SLOTS (mh_attn_prefix_partial_slots, attention_shared.hip;
mh_attn_decode_append_rows_shared, attention_small.hip): G prompts, every row of the batch at a position of its own and in at most one
slot.  The yardstick is the pair of kernels they generalise: per row, the partials, the output and the cache row written must be BIT
equal to mh_attn_prefix_partial + mh_attn_decode_append_shared called for that row alone (B = 1, its slot's K/V, its position, its own
cache), and to mh_attn_decode_append_rows for a row without a slot.  Whole buffers are compared through integer views, poisoned first,
so what must not be written is checked with what must.  Values: float64 over the concatenated prefix and suffix, under the bounds of
test_shared_prefix_kernels_gpu.py."""
import pytest
import torch

from test_cache_attention_gpu import DECODE_INST, F64, NAN, bits, grnd, same_bits
from test_shared_prefix_kernels_gpu import _bound

import emu_poolshare

pytestmark = pytest.mark.gpu

C = 256
HD, SCALE = 64, 0.125
INSTS = ["bf16_hd64", "fp32_hd64"]


@pytest.fixture(scope="module")
def ops():
    import midi_model_amd.ops as real
    return real


@pytest.fixture(scope="module")
def sh():
    import midi_model_amd.shared as real
    return real


def _i32(x):
    return torch.tensor(list(x), dtype=torch.int32, device="cuda")


class Case:
    """B rows, H heads, G slots of Pmax rows, caches of Lsuf rows; slot g holds slot_len[g] rows, row b names row_slot[b] and stands
    ``suf[b]`` rows behind its prompt.  Everything the kernels must not read or write holds NaN."""

    def __init__(self, dtype, B, H, G, Pmax, Lsuf, slot_len, row_slot, suf, seed):
        from midi_model_amd.engine import RopeTable
        self.dtype, self.B, self.H, self.G, self.Pmax, self.Lsuf = dtype, B, H, G, Pmax, Lsuf
        self.slot_len, self.row_slot, self.suf = list(slot_len), list(row_slot), list(suf)
        self.pre = [min(self.slot_len[g], Pmax) if 0 <= g < G else 0 for g in self.row_slot]
        self.pos = [p + s for p, s in zip(self.pre, self.suf)]
        assert len(self.row_slot) == B == len(self.suf) and max(self.suf) < Lsuf
        D = H * HD
        self.tab = RopeTable(HD, 10000.0, "cuda", max(self.pos) + 1)
        self.qkv = grnd((B, 3 * D), dtype, seed)
        self.kpre = torch.full((G, H, Pmax, HD), NAN, dtype=dtype, device="cuda")
        self.vpre = torch.full_like(self.kpre, NAN)
        for g, n in enumerate(self.slot_len):
            n = min(n, Pmax)
            if n:
                self.kpre[g, :, :n] = grnd((H, n, HD), dtype, seed + 10 + g)
                self.vpre[g, :, :n] = grnd((H, n, HD), dtype, seed + 20 + g)
        self.ksuf = torch.full((B, H, Lsuf, HD), NAN, dtype=dtype, device="cuda")
        self.vsuf = torch.full_like(self.ksuf, NAN)
        for b, n in enumerate(self.suf):
            if n:
                self.ksuf[b, :, :n] = grnd((H, n, HD), dtype, seed + 100 + b)
                self.vsuf[b, :, :n] = grnd((H, n, HD), dtype, seed + 300 + b)
        self.len_dev, self.slot_dev, self.pos_dev = _i32(self.slot_len), _i32(self.row_slot), _i32(self.pos)
        self.nch = (Pmax + C - 1) // C

    def fresh(self, B=None):
        """a poisoned (workspace, o) pair for B rows"""
        B = self.B if B is None else B
        return (torch.full((66 * B * self.H * self.nch,), NAN, device="cuda"),
                torch.full((B, self.H * HD), NAN, dtype=self.dtype, device="cuda"))

    def run(self, ops, slot_dev=None, len_dev=None):
        """the two slot kernels on clones of the caches -> (ws, o, ksuf, vsuf); the inputs must come back bit-unchanged"""
        ws, o = self.fresh()
        ks, vs = self.ksuf.clone(), self.vsuf.clone()
        slot_dev = self.slot_dev if slot_dev is None else slot_dev
        len_dev = self.len_dev if len_dev is None else len_dev
        keep = [t.clone() for t in (self.qkv, self.kpre, self.vpre)]
        ops.attn_prefix_partial_slots(self.qkv, self.tab.cos, self.tab.sin, self.kpre, self.vpre, len_dev, slot_dev, self.pos_dev, ws,
                                      self.B, self.H, HD, self.G, self.Pmax, SCALE)
        ops.attn_decode_append_rows_shared(self.qkv, self.tab.cos, self.tab.sin, ks, vs, ws, o, self.B, self.H, HD, self.Lsuf, self.G,
                                           self.Pmax, SCALE, len_dev, slot_dev, self.pos_dev)
        for t, t0 in zip((self.qkv, self.kpre, self.vpre), keep):
            assert same_bits(t, t0), "qkv or a slot cache was written"
        return ws, o, ks, vs

    def expected(self, ops, sh):
        """the same four buffers assembled row by row from the EXISTING kernels: a sharing row from the uniform pair at B = 1 on its
        slot's K/V, its position and its own cache; a row without a slot from mh_attn_decode_append_rows at B = 1, its partials
        left poisoned"""
        ws, o = self.fresh()
        ks, vs = self.ksuf.clone(), self.vsuf.clone()
        n_acc = self.B * self.H * self.nch * 64
        acc, ml = ws[:n_acc].view(self.B, -1), ws[n_acc:].view(self.B, -1)
        for b in range(self.B):
            q1 = self.qkv[b:b + 1].contiguous()
            k1, v1 = ks[b:b + 1].clone(), vs[b:b + 1].clone()
            ws1, o1 = self.fresh(1)
            if self.pre[b]:
                g = self.row_slot[b]
                sh.attn_prefix_partial(q1, self.tab.cos, self.tab.sin, self.kpre[g], self.vpre[g], ws1, 1, self.H, HD, self.Pmax,
                                       self.pre[b], self.pos[b], SCALE)
                sh.attn_decode_append_shared(q1, self.tab.cos, self.tab.sin, k1, v1, ws1, o1, 1, self.H, HD, self.Lsuf, self.Pmax,
                                             self.pre[b], self.pos[b], SCALE)
                acc[b], ml[b] = ws1[: self.H * self.nch * 64], ws1[self.H * self.nch * 64:]
            else:
                ops.attn_decode_append_rows(q1, self.tab.cos, self.tab.sin, k1, v1, o1, 1, self.H, HD, self.Lsuf, SCALE,
                                            self.pos_dev[b:b + 1].contiguous())
            o[b], ks[b], vs[b] = o1[0], k1[0], v1[0]
        return ws, o, ks, vs


def _assert_same(got, want, what):
    for name, a, b in zip(("workspace", "o", "k cache", "v cache"), got, want):
        if not same_bits(a, b):
            at = (bits(a) != bits(b)).nonzero()
            raise AssertionError(f"{what}: {name} differs in {len(at)} elements, first at {at[0].tolist()}")


@pytest.mark.parametrize("inst", INSTS)
def test_one_slot_at_a_uniform_position_is_the_uniform_pair(ops, sh, inst):
    """G = 1, every row a member, all row_pos equal (37 rows: two query tiles, the second padded; a prompt of 300 of 600: the second
    chunk ragged, the third unused): the whole workspace, o and both caches are bit-equal to mh_attn_prefix_partial +
    mh_attn_decode_append_shared at that (pre_len, pos)"""
    dtype = DECODE_INST[inst][0]
    B, H, pre, suf = 37, 2, 300, 7
    c = Case(dtype, B, H, 1, 600, 40, [pre], [0] * B, [suf] * B, 100)
    got = c.run(ops)
    ws, o = c.fresh()
    ks, vs = c.ksuf.clone(), c.vsuf.clone()
    sh.attn_prefix_partial(c.qkv, c.tab.cos, c.tab.sin, c.kpre[0], c.vpre[0], ws, B, H, HD, 600, pre, pre + suf, SCALE)
    sh.attn_decode_append_shared(c.qkv, c.tab.cos, c.tab.sin, ks, vs, ws, o, B, H, HD, 40, 600, pre, pre + suf, SCALE)
    _assert_same(got, (ws, o, ks, vs), f"{inst} one slot, uniform")
    assert torch.isfinite(o).all()


SLOT_LENS = ([257, 600, 0], [1, 256, 512])   # lengths on both sides of a chunk edge (256) and of a wave's 64 keys


@pytest.mark.parametrize("slot_len", SLOT_LENS, ids=["257_600_0", "1_256_512"])
@pytest.mark.parametrize("inst", INSTS)
def test_several_slots_per_row_positions(ops, sh, inst, slot_len):
    """B = 6, H = 2, G = 3, Pmax = 600 (three chunks), Lsuf = 40, row_slot = [1, -1, 0, 1, -1, 0], six distinct positions: every
    sharing row's partials, output and cache are bit-equal to the uniform pair called for that row alone, every row without a slot to
    mh_attn_decode_append_rows; the partials of chunks at or past ceil(slot_len / 256) and of rows without a slot keep their poison;
    the caches are compared whole"""
    dtype = DECODE_INST[inst][0]
    c = Case(dtype, 6, 2, 3, 600, 40, slot_len, [1, -1, 0, 1, -1, 0], [3, 17, 0, 39, 5, 22], 200)
    assert len(set(c.pos)) == 6
    got, want = c.run(ops), c.expected(ops, sh)
    _assert_same(got, want, f"{inst} slots {slot_len}")
    ws, o = got[0], got[1]
    assert torch.isfinite(o).all()
    acc = ws[: 6 * 2 * c.nch * 64].view(6, 2, c.nch, 64)
    ml = ws[6 * 2 * c.nch * 64:].view(6, 2, c.nch, 2)
    for b in range(6):
        used = (c.pre[b] + C - 1) // C
        assert torch.isfinite(acc[b, :, :used]).all() and torch.isfinite(ml[b, :, :used]).all()
        assert torch.isnan(acc[b, :, used:]).all() and torch.isnan(ml[b, :, used:]).all(), f"row {b}: a partial past its prompt"


@pytest.mark.parametrize("inst", INSTS)
def test_more_members_than_one_query_tile(ops, sh, inst):
    """B = 40, slot 1 of 2 with 35 members at scattered rows (two 32-row query tiles, the second padded), 5 rows without a slot:
    per row the same reference"""
    dtype = DECODE_INST[inst][0]
    B = 40
    out = {3, 11, 12, 30, 39}
    c = Case(dtype, B, 2, 2, 300, 24, [0, 290], [-1 if b in out else 1 for b in range(B)], [(7 * b) % 23 for b in range(B)], 300)
    _assert_same(c.run(ops), c.expected(ops, sh), f"{inst} 35 members")


@pytest.mark.parametrize("slot_len", SLOT_LENS, ids=["257_600_0", "1_256_512"])
@pytest.mark.parametrize("inst", INSTS)
def test_against_float64(ops, inst, slot_len):
    """a straight softmax attention in float64 over the concatenated prefix, suffix and new key (emu_poolshare.reference), under the
    bounds of test_shared_prefix_kernels_gpu.py: bf16 2^-8 |o64| + 3e-3 rms(V), fp32 3e-6 |o64| + 2e-6 max|v|"""
    dtype = DECODE_INST[inst][0]
    c = Case(dtype, 6, 2, 3, 600, 40, slot_len, [1, -1, 0, 1, -1, 0], [3, 17, 0, 39, 5, 22], 400)
    _, o, _, _ = c.run(ops)
    cpu = lambda t: t.cpu()
    ref = emu_poolshare.reference(cpu(c.qkv), cpu(c.tab.cos), cpu(c.tab.sin), cpu(c.kpre), cpu(c.vpre), cpu(c.ksuf), cpu(c.vsuf), c.H,
                                  c.slot_len, c.row_slot, c.pos, SCALE).view(6, c.H, HD)
    got = o.cpu().to(F64).view(6, c.H, HD)
    c_rel, c_abs, kind = _bound(dtype)
    D = c.H * HD
    for b in range(6):
        g = c.row_slot[b]
        vals = [c.vsuf[b, :, :c.suf[b]], c.qkv[b, 2 * D:].view(c.H, 1, HD)] + ([c.vpre[g, :, :c.pre[b]]] if c.pre[b] else [])
        v = torch.cat([x.reshape(c.H, -1) for x in vals], 1).cpu().to(F64)
        scale_v = v.pow(2).mean().sqrt().item() if kind == "rms" else v.abs().amax(1)[:, None]
        bound = c_rel * ref[b].abs() + c_abs * scale_v
        ratio = ((got[b] - ref[b]).abs() / bound).max().item()
        print(f"  {inst} slots {slot_len} row {b} (pre {c.pre[b]}, pos {c.pos[b]}): err/bound {ratio:.3f}")
        assert ratio <= 1.0, (b, ratio)


def test_refusals_and_what_the_kernels_drop(ops):
    """every host refusal is MH_ERR_ARG with the buffers untouched -- a NULL array by name, a dtype, hd != 64, G < 1, a short
    workspace, the grid limits; in the kernels a row_slot entry outside [0, G) is -1 and slot_len is clamped to Pmax"""
    from midi_model_amd.lib import MH_BF16, MH_F32, lib
    MH_ERR_ARG = -1
    cdll = lib().cdll
    st = torch.cuda.current_stream().cuda_stream
    for dtype, code in ((torch.bfloat16, MH_BF16), (torch.float32, MH_F32)):
        c = Case(dtype, 6, 2, 3, 600, 40, [257, 600, 0], [1, -1, 0, 1, -1, 0], [3, 17, 0, 39, 5, 22], 500)
        ws, o = c.fresh()
        ks, vs = c.ksuf.clone(), c.vsuf.clone()
        p = lambda t: t.data_ptr()
        part = [p(c.qkv), p(c.tab.cos), p(c.tab.sin), p(c.kpre), p(c.vpre), p(c.len_dev), p(c.slot_dev), p(c.pos_dev), p(ws),
                ws.numel(), 6, 2, 64, 3, 600, SCALE, code, st]
        dec = [p(c.qkv), p(c.tab.cos), p(c.tab.sin), p(ks), p(vs), p(ws), ws.numel(), p(o), 6, 2, 64, 40, 3, 600, SCALE,
               p(c.len_dev), p(c.slot_dev), p(c.pos_dev), code, st]
        keep = [t.clone() for t in (c.qkv, c.kpre, c.vpre, ks, vs, ws, o)]

        def refused(name, args, at, value, word):
            bad = list(args)
            bad[at] = value
            assert getattr(cdll, name)(*bad) == MH_ERR_ARG, (name, at, value)
            msg = cdll.mh_last_error().decode()
            assert word in msg, (name, at, value, msg)

        for at, word in ((0, "qkv"), (1, "rope"), (2, "rope"), (3, "kpre"), (4, "vpre"), (5, "slot_len"), (6, "row_slot"),
                         (7, "row_pos"), (8, "ws")):
            refused("mh_attn_prefix_partial_slots", part, at, 0, word)
        for at, value, word in ((16, 7, "dtype"), (12, 32, "head_dim"), (12, 128, "head_dim"), (13, 0, "slots"), (13, -1, "slots"),
                                (13, 65536, "slots"), (9, ws.numel() - 1, "workspace"), (10, 0, "bad args"), (10, 4097, "bad args"),
                                (11, 0, "bad args"), (14, 0, "bad args"), (14, 1 << 24, "bad args")):
            refused("mh_attn_prefix_partial_slots", part, at, value, word)
        for at, word in ((0, "qkv"), (1, "rope"), (2, "rope"), (3, "ksuf"), (4, "vsuf"), (5, "ws"), (7, "o is NULL"), (15, "slot_len"),
                         (16, "row_slot"), (17, "row_pos")):
            refused("mh_attn_decode_append_rows_shared", dec, at, 0, word)
        for at, value, word in ((18, 7, "dtype"), (10, 32, "head_dim"), (10, 256, "head_dim"), (12, 0, "slots"), (12, 65536, "slots"),
                                (6, ws.numel() - 1, "workspace"), (8, 0, "bad args"), (8, 65536, "bad args"), (9, 0, "bad args"),
                                (11, 0, "bad args"), (11, 1 << 24, "bad args"), (13, 0, "bad args")):
            refused("mh_attn_decode_append_rows_shared", dec, at, value, word)
        torch.cuda.synchronize()
        for t, t0 in zip((c.qkv, c.kpre, c.vpre, ks, vs, ws, o), keep):
            assert same_bits(t, t0), "a refused call wrote a buffer"
        # ---- an out-of-range row_slot entry behaves as -1 (rows 1 and 4 name slots 3 and -7; the others are as they were)
        want = c.run(ops)
        got = c.run(ops, slot_dev=_i32([1, 3, 0, 1, -7, 0]))
        _assert_same(got, want, f"{dtype} out-of-range row_slot")
        # ---- slot_len past Pmax is Pmax (slot 1 is full: 600 of 600)
        got = c.run(ops, len_dev=_i32([257, 650, 0]))
        _assert_same(got, want, f"{dtype} slot_len past Pmax")
