"""The table form of the event-level attention (mh_attn_fwd_seqs / mh_attn_bwd_seqs) and mh_rope_pos on the MI355X.

Criterion: BIT equality with the existing uniform entry points run on every sequence alone (B = 1, S = its length, same default
kernel forms).  The table form only changes the kernels' preambles -- where a sequence's rows and statistics lie -- and a sequence's
tiles are counted from its own first row, so every (sequence, head, tile) performs the arithmetic of the uniform launch in the same
order; the work list only decides WHEN a tile runs.  One ragged table is also checked against the float64 stand-ins of
emu_packed.py with the `cmp` bounds of test_kernels_gpu.py: that anchor does not rest on the uniform kernels.

Every operand and result is a view between NaN-filled guard rows of one allocation: a read past a sequence's end that leaks into a
result shows as a NaN or as a mismatch, a write past the buffer shows in the guards -- without provoking a fault."""
import pytest
import torch

import emu_packed
from test_kernels_gpu import cmp

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
GUARD = 8  # rows
SCALE = 64 ** -0.5

# (lengths, H): single rows, tile edges (64 / 65 / 128 / 129), starts that are no multiple of 64 or 8, more 128-row tiles than one,
# more (sequence, head) pairs than XCDs, and one table whose head count is no power of two
TABLES = [([1], 2), ([64], 2), ([65], 2), ([1, 1, 1], 2), ([63, 1, 64], 2), ([33, 200, 7, 128, 129], 2), ([515, 40], 2),
          ([128, 128, 128], 2), ([200, 200], 2), ([70, 3, 129], 3)]


@pytest.fixture(scope="module")
def ops():
    import midi_model_amd.ops as real
    return real


@pytest.fixture(scope="module")
def rope_tab():
    from midi_model_amd.engine import RopeTable
    return RopeTable(64, 10000.0, "cuda", 1024)


def guarded(rows, cols, dtype):
    """-> (whole allocation, the [rows, cols] view between its guard rows), everything NaN"""
    whole = torch.full((rows + 2 * GUARD, cols), float("nan"), dtype=dtype, device="cuda")
    return whole, whole[GUARD:GUARD + rows]


def guards_intact(whole, what):
    assert torch.isnan(whole[:GUARD]).all() and torch.isnan(whole[-GUARD:]).all(), f"{what}: a guard row was written"
    assert not torch.isnan(whole[GUARD:-GUARD]).any(), f"{what}: NaN in the result (unwritten row, or a read past a sequence)"


def rnd(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(dtype)


class Case:
    """inputs of one (table, H, dtype) on the device, in guarded buffers, and the packed results"""

    def __init__(self, ops, lengths, H, dtype, rope_tab):
        self.lengths, self.H, self.dtype, self.D = lengths, H, dtype, H * 64
        self.plan = ops.attn_seq_plan(lengths, H).upload("cuda")
        M = self.M = self.plan.M
        self.bounds = list(zip(self.plan.host_views()[0].tolist()[:-1], self.plan.host_views()[0].tolist()[1:]))
        self.qkv_w, self.qkv = guarded(M, 3 * self.D, dtype)
        self.do_w, self.do = guarded(M, self.D, dtype)
        self.qkv.copy_(rnd((M, 3 * self.D), dtype, 18))
        self.do.copy_(rnd((M, self.D), dtype, 19))
        self.rs = (0.5 + torch.rand(M, generator=torch.Generator().manual_seed(20))).cuda()
        self.o_w, self.o = guarded(M, self.D, dtype)
        self.lse_w, lse = guarded(H, M, torch.float32)
        self.lse = lse
        ops.attn_fwd_seqs(self.qkv, self.o, self.lse, self.plan, H, SCALE)
        self.variants = {"plain": {}, "rotated back": dict(cos_t=rope_tab.cos, sin_t=rope_tab.sin)}
        if dtype == torch.bfloat16:  # (rowscale: the bf16 kernels only, as in the uniform entry points)
            self.variants["rowscale"] = dict(rowscale=self.rs)
            self.variants["rowscale, rotated back"] = dict(rowscale=self.rs, cos_t=rope_tab.cos, sin_t=rope_tab.sin)
        self.dqkv = {}
        for name, kw in self.variants.items():
            w, v = guarded(M, 3 * self.D, dtype)
            ops.attn_bwd_seqs(self.qkv, self.o, self.do, self.lse, v, self.plan, H, SCALE, **kw)
            self.dqkv[name] = (w, v)
        torch.cuda.synchronize()

    def check_guards(self):
        for w, what in ((self.qkv_w, "qkv"), (self.do_w, "dout"), (self.o_w, "o"), (self.lse_w, "lse")):
            guards_intact(w, what)
        for name, (w, _) in self.dqkv.items():
            guards_intact(w, f"dqkv ({name})")

    def uniform(self, ops, B, S, a, b):
        """the uniform entry points on rows [a, b) = B sequences of S rows -> (o, lse [B*H, S], {variant: dqkv})"""
        H, D = self.H, self.D
        qkv, do = self.qkv[a:b].clone(), self.do[a:b].clone()
        Sp = (S + 63) // 64 * 64
        o = torch.full((B * S, D), float("nan"), dtype=self.dtype, device="cuda")
        lse = torch.full((B * H * Sp,), float("nan"), device="cuda")
        ops.attn_fwd(qkv, o, lse, B, S, H, SCALE)
        out = {}
        for name, kw in self.variants.items():
            kw = dict(kw)
            if "rowscale" in kw:
                kw["rowscale"] = self.rs[a:b].clone()
            out[name] = ops.attn_bwd(qkv, o, do, lse, torch.full((B * S, 3 * D), float("nan"), dtype=self.dtype, device="cuda"), B, S, H,
                                     SCALE, **kw)
        return o, lse.view(B * H, Sp)[:, :S], out


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("lengths,H", TABLES, ids=[f"{'_'.join(map(str, t))}-H{h}" for t, h in TABLES])
def test_table_form_equals_the_uniform_kernels_per_sequence(ops, rope_tab, lengths, H, dtype):
    """bf16: the table-form MFMA kernels against the uniform launches.  fp32 has NO table-form kernels (ops.attn_*_seqs run the
    uniform plain kernels sequence by sequence), so its cases compare those kernels with themselves: what they check is the
    wrapper -- the [H, M] <-> [H, Sp] lse re-layout, the row slices, the rotation back per sequence, untouched guard rows."""
    c = Case(ops, lengths, H, dtype, rope_tab)
    c.check_guards()
    for i, (a, b) in enumerate(c.bounds):
        o, lse, dq = c.uniform(ops, 1, b - a, a, b)
        assert torch.equal(c.o[a:b], o), f"o of sequence {i} (rows {a}..{b})"
        assert torch.equal(c.lse[:, a:b], lse), f"lse of sequence {i}"
        for name in c.variants:
            got, want = c.dqkv[name][1][a:b], dq[name]
            assert torch.equal(got, want), (f"dqkv ({name}) of sequence {i} (rows {a}..{b}): "
                                            f"{int((got != want).sum())} elements differ, first at {(got != want).nonzero()[0].tolist()}")
    if len(set(lengths)) == 1 and len(lengths) > 1:  # equal lengths: the whole batch against ONE uniform launch
        n, S = len(lengths), lengths[0]
        o, lse, dq = c.uniform(ops, n, S, 0, c.M)
        assert torch.equal(c.o, o)
        assert torch.equal(c.lse, lse.view(n, H, S).transpose(0, 1).reshape(H, n * S))
        for name in c.variants:
            assert torch.equal(c.dqkv[name][1], dq[name]), name


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_table_form_against_the_float64_stand_in(ops, rope_tab, dtype):
    """independent of the uniform kernels: the ragged table against emu_packed, bounds = test_kernels_gpu.cmp with the factors
    test_attention_fwd_bwd uses (o 1, lse 1 / 50, gradients 3)"""
    lengths, H = [33, 200, 7, 128, 129], 2
    c = Case(ops, lengths, H, dtype, rope_tab)
    plan = ops.attn_seq_plan(lengths, H)
    qkv, do = c.qkv.cpu(), c.do.cpu()
    o_ref, lse_ref = torch.empty_like(c.o, device="cpu"), torch.empty((H, c.M))
    emu_packed.attn_fwd_seqs(qkv, o_ref, lse_ref, plan, H, SCALE)
    cmp(c.o, o_ref, dtype, what="o")
    cmp(c.lse, lse_ref, torch.float32, k=(1 if dtype == torch.float32 else 50), what="lse")
    for name, kw in c.variants.items():
        kw = {k: v.cpu() for k, v in kw.items()}
        want = emu_packed.attn_bwd_seqs(qkv, o_ref, do, lse_ref, torch.empty_like(qkv), plan, H, SCALE, **kw)
        cmp(c.dqkv[name][1], want, dtype, k=3 * (1.5 if "rowscale" in kw else 1.0), what=f"dqkv ({name})")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("H,hd", [(2, 64), (1, 256)])
def test_rope_pos_equals_rope_per_sequence(ops, dtype, H, hd):
    from midi_model_amd.engine import RopeTable
    tab = RopeTable(hd, 10000.0, "cuda", 256)
    lengths = [33, 200, 7, 1, 129]
    plan = ops.attn_seq_plan(lengths, H).upload("cuda")
    src = rnd((plan.M, 3 * H * hd), dtype, 21).cuda()
    bounds = plan.host_views()[0].tolist()
    for direction in (1, -1):
        whole, x = guarded(plan.M, 3 * H * hd, dtype)
        x.copy_(src)
        ops.rope_pos_(x, tab.cos, tab.sin, plan.pos, H, hd, direction)
        guards_intact(whole, "rope_pos")
        for a, b in zip(bounds[:-1], bounds[1:]):
            want = ops.rope_(src[a:b].clone(), tab.cos, tab.sin, b - a, 0, H, hd, direction)
            assert torch.equal(x[a:b], want), (direction, a, b)
        assert torch.equal(x[:, 2 * H * hd:], src[:, 2 * H * hd:])  # v untouched


def test_other_attention_forms_are_an_error(ops, rope_tab):
    """a non-default "attn_v3" is refused by the bf16 table form -- no other computation, nothing written"""
    H, lengths = 2, [40, 70]
    plan = ops.attn_seq_plan(lengths, H).upload("cuda")
    qkv = rnd((plan.M, 3 * H * 64), torch.bfloat16, 22).cuda()
    o = torch.full((plan.M, H * 64), float("nan"), dtype=torch.bfloat16, device="cuda")
    lse = torch.full((H, plan.M), float("nan"), device="cuda")
    dqkv = torch.full_like(qkv, float("nan"))
    try:
        for bits in (127, 31, 0):
            ops.set_option("attn_v3", bits)
            with pytest.raises(RuntimeError, match="attn_fwd_seqs"):
                ops.attn_fwd_seqs(qkv, o, lse, plan, H, SCALE)
            with pytest.raises(RuntimeError, match="attn_bwd_seqs"):
                ops.attn_bwd_seqs(qkv, o, o, lse, dqkv, plan, H, SCALE)
    finally:
        ops.set_option("attn_v3", 255)
    torch.cuda.synchronize()
    assert torch.isnan(o).all() and torch.isnan(lse).all() and torch.isnan(dqkv).all()
    ops.attn_fwd_seqs(qkv, o, lse, plan, H, SCALE)  # the default form serves it
    assert torch.isfinite(o.float()).all()
