"""The training attention kernels held to float64 at their edges (bounds, families and references: tests/ref_attention.py, whose
accept / reject proof on the CPU is tests/test_attention_bounds_host.py):

  1. the bf16 MFMA backward (mh_attn_bwd_o, mh_attn_bwd_o_scaled, mh_attn_prep_bwd + mh_attn_bwd) in every form the dispatch of
     mh_attn_bwd_mfma / mh_attn_bwd_mfma3 / ops.attn_bwd can reach, at S around the wave (32, 96), key-tile (64) and query-tile (128)
     edges, one to five 128-row tiles, odd and even tile counts, ragged tails, B * H = 1, 8, 9;
  2. the MFMA forward in every form of test_kernels_gpu.ATTN_FORMS at the same S;
  3. the plain thread-per-row kernels in fp32 and bf16;
  4. the token-level kernels (T = 1 .. 8, N * H of every residue mod 4, RoPE, row scale, both backward forms, past the grid cap);
  5. what the entry points refuse (mh_attn_bwd_o under attn_v3 = 7 is refused in
     test_kernels_gpu.py::test_attention_bwd_in_one_call_hands_over_delta_and_says_what_it_does_not_serve).

Every operand and result is a view between NaN-filled guard rows of its allocation, results are pre-filled with NaN, and the guards
are checked after every launch: a read past the end that leaks into a result shows as a NaN or a mismatch, a write past the buffer
shows in the guards.  No input is built to make a kernel read or write outside an allocation.  Every test that sets a kernel option
reads it first and restores it.

Measured on the MI355X, 2026-10-19: the whole file (70 cases) takes 16.4 s of pytest wall time, the slowest case 1.8 s (the first
one, which loads both libraries), a backward case 0.5 s: 9 inputs x 14 forms and 502 backward calls per S.  The worst
err/bound per family and gradient are in the module docstring of ref_attention.py."""
import contextlib

import pytest
import torch

import ref_attention as ra
from test_kernels_gpu import ATTN_FORMS

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")
GUARD = 8        # rows (2-D buffers)
GUARD1 = 64      # elements (the fp32 statistics: keeps their 256-byte alignment)
BH_LIST = [(1, 1), (2, 4), (3, 3)]   # 1, 8 and 9 (batch, head) pairs: 9 is a ragged second group of eight; H = 3: no power of two

# Backward forms, from the dispatch.  ops.attn_bwd: (attn_v3 & 14) == 14 and bit 5 -> one call (mh_attn_bwd_o: delta inside dQ, the
# statistics handed to dK/dV pre-scaled); (attn_v3 & 14) == 14 without it -> mh_attn_prep_bwd (delta) + mh_attn_bwd, transpose reads;
# otherwise the three prepared copies.  mh_attn_bwd_mfma3: attn_v3_wps == 2 picks the dQ kernel's 2-waves-per-SIMD build, every
# other value the 3-waves build (0 and 3 are the same kernel; 2 differs in its register budget only: the same arithmetic).
PROD_FORMS = [(v3, wps) for v3 in (255, 31, 7) for wps in (0, 2, 3)]
# The A/B library alone: a first-form kernel for dQ, dK/dV or both ((attn_v3 & 6) != 6), beside a third-form one from the prepared
# copies (2, 4) or by transpose reads (10, 12: mh_attn_bwd_mfma hands `attn_v3 & 14` on)
AB_FORMS = [(0, 0), (2, 0), (4, 0), (10, 0), (12, 0)]
BWD_FORMS = [(v3, wps, False) for v3, wps in PROD_FORMS] + [(v3, wps, True) for v3, wps in AB_FORMS]


@pytest.fixture(scope="module")
def ops():
    import midi_model_amd.ops as real
    return real


def lib():
    from midi_model_amd.lib import lib as _lib
    return _lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
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


def form_ctx(ops, v3, wps, ab):
    st = contextlib.ExitStack()
    if ab:
        st.enter_context(ops.ab_library())
    st.enter_context(options(ops, attn_v3=v3, attn_v3_wps=wps))
    return st


class Buf:
    """a tensor between NaN guard rows (2-D) / guard elements (1-D fp32) of one allocation"""

    def __init__(self, shape, dtype, fill=NAN, src=None):
        if len(shape) == 2:
            self.g = GUARD
            self.whole = torch.full((shape[0] + 2 * GUARD, shape[1]), NAN, dtype=dtype, device="cuda")
        else:
            self.g = GUARD1
            self.whole = torch.full((shape[0] + 2 * GUARD1,), NAN, dtype=dtype, device="cuda")
        self.t = self.whole[self.g:self.g + shape[0]]
        if src is not None:
            self.t.copy_(src)
        elif fill == fill:
            self.t.fill_(fill)

    def guards_intact(self, what):
        w, g = self.whole, self.g
        assert torch.isnan(w[:g]).all() and torch.isnan(w[-g:]).all(), f"{what}: a guard was written"


def check_guards(what, *bufs):
    for b in bufs:
        b.guards_intact(what)


def pad_mask(B, S, H, Sp):
    m = torch.zeros((B, H, Sp), dtype=torch.bool, device="cuda")
    m[:, :, S:] = True
    return m.view(-1)


# ------------------------------------------------------------------------------------------------ 1. bf16 MFMA backward
class EventCase:
    """one (family, B, S, H) in bf16: guarded inputs on the device, the float64 parts that do not depend on the stored O, and the
    finished references per distinct O (the forward forms differ in a few bits of O; delta comes from the stored one)"""

    def __init__(self, fam, B, S, H, seed, backward=True):
        self.fam, self.B, self.S, self.H = fam, B, S, H
        self.D, self.Sp, self.M = H * 64, (S + 63) // 64 * 64, B * S
        qkv, do = ra.event_inputs(fam, B, S, H, BF16, seed)
        self.qkv, self.do = Buf(qkv.shape, BF16, src=qkv.cuda()), Buf(do.shape, BF16, src=do.cuda())
        self.pad = pad_mask(B, S, H, self.Sp)
        self.n_bwd = 0
        if backward:
            self.base = ra.Bwd64(self.qkv.t, self.do.t, B, S, H)
            self._grads = []
            self.rs = ra.rowscale_input(self.M, seed + 1, "cuda")

    def inputs(self):
        return (self.qkv, self.do)

    def forward(self, ops, what):
        B, S, H = self.B, self.S, self.H
        o, lse = Buf((self.M, self.D), BF16), Buf((B * H * self.Sp,), F32)
        ops.attn_fwd(self.qkv.t, o.t, lse.t, B, S, H, ra.SCALE)
        check_guards(f"{what} forward", o, lse, *self.inputs())
        assert not torch.isnan(o.t).any(), f"{what}: forward left rows of o unwritten (or NaN)"
        # the pad entries [S, Sp) of lse: every forward form stores `if (qrow < S)` only -- untouched
        assert torch.isnan(lse.t[self.pad]).all(), f"{what}: forward wrote lse pad entries"
        assert torch.isfinite(lse.t[~self.pad]).all(), f"{what}: lse"
        return o, lse

    def grads(self, o):
        for oc, G in self._grads:
            if same_bits(oc, o):
                return G
        G = self.base.grads(o)
        self._grads.append((o.clone(), G))
        return G

    def backward(self, v3, o, lse, what, scratch_fill=NAN, cos=None, sin=None, rowscale=None, rows_of=None):
        """ops.attn_bwd's dispatch with the scratch in a guarded buffer of our own (pre-filled); rows_of = b: the launch with
        B = 1 on batch element b's rows alone.  -> dqkv [rows, 3 D] (a view of its guarded buffer)"""
        B, S, H, Sp, D = self.B, self.S, self.H, self.Sp, self.D
        qkv, do, ot, lt = self.qkv.t, self.do.t, o.t, lse.t
        if rows_of is not None:
            b, B = rows_of, 1
            qkv, do, ot, lt = qkv[b * S:(b + 1) * S], do[b * S:(b + 1) * S], ot[b * S:(b + 1) * S], lt[b * H * Sp:(b + 1) * H * Sp]
        fused = (v3 & 14) == 14 and (v3 & 32) != 0
        scratch = Buf(((2 if fused else 1) * B * H * Sp,), F32, fill=scratch_fill)
        dqkv = Buf((B * S, 3 * D), BF16)
        p = lambda t: 0 if t is None else t.data_ptr()
        L, st = lib(), stream()
        copies = None
        if rowscale is not None:
            L.call("mh_attn_bwd_o_scaled", p(qkv), p(ot), p(do), p(lt), p(scratch.t), p(dqkv.t), p(rowscale), B, S, H, ra.SCALE, p(cos), p(sin), 1, st)
        elif fused:
            L.call("mh_attn_bwd_o", p(qkv), p(ot), p(do), p(lt), p(scratch.t), p(dqkv.t), B, S, H, ra.SCALE, p(cos), p(sin), 1, st)
        else:
            qt = kt = dot = None
            if (v3 & 14) != 14:
                copies = Buf((3, B * H * 64 * Sp), BF16)
                qt, kt, dot = copies.t[0], copies.t[1], copies.t[2]
            L.call("mh_attn_prep_bwd", p(qkv), p(ot), p(do), p(scratch.t), p(qt), p(kt), p(dot), B, S, H, 1, st)
            L.call("mh_attn_bwd", p(qkv), p(do), p(lt), p(scratch.t), p(qt), p(kt), p(dot), p(dqkv.t), B, S, H, ra.SCALE, p(cos), p(sin), 1, st)
        self.n_bwd += 1
        check_guards(f"{what} backward", dqkv, scratch, o, lse, *self.inputs(), *([copies] if copies is not None else []))
        assert not torch.isnan(dqkv.t).any(), f"{what}: backward left elements unwritten (or NaN)"
        return dqkv.t


def _bump(worst, fam, r):
    for nm, v in r.items():
        worst[(fam, nm)] = max(worst.get((fam, nm), 0.0), v)


@pytest.mark.parametrize("S", ra.S_LIST)
def test_event_backward_against_float64(ops, S):
    """For (B, H) in BH_LIST x the three families x every backward form (BWD_FORMS; the forward that produces o and lse runs under the
    same option), with lse's pad entries [S, Sp) NaN as the forward leaves them and the delta scratch pre-filled with NaN:
      * dQ, dK, dV inside the bound of ref_attention.mfma_bound; dV also inside 1.25 2^-8 (|g| + R) alone wherever R > 0;
      * bit-identical to the run with those pad entries and the scratch zero, and (gauss) to ops.attn_bwd itself;
      * rotated back through a RopeTable: inside rot_bound against the rotated float64 gradient, dV columns bit-equal to the plain run;
      * rowscale (forms that serve it): scales in [0.5, 1.5] plus exactly 0.0 and -1.0, bound |rowscale| x the unscaled one, the
        zero-scaled row exactly zero; also rotated back;
      * (gauss) every batch element's rows equal, bit for bit, the launch with B = 1 on those rows alone;
      * attn_v3_wps 0 / 2 / 3 of one attn_v3: the same bits (the documented same arithmetic)."""
    from midi_model_amd.engine import RopeTable
    tab = RopeTable(64, 10000.0, "cuda", S + 1)
    cos, sin = tab.cos, tab.sin
    worst, worst_rot, worst_rs, n_bwd = {}, {}, {}, 0
    for B, H in BH_LIST:
        D = H * 64
        for fam in ra.FAMILIES:
            c = EventCase(fam, B, S, H, 5000 + 7 * S + B)
            by_v3 = {}
            for v3, wps, ab in BWD_FORMS:
                what = f"S={S} B={B} H={H} {fam} attn_v3={v3} wps={wps}{' (A/B library)' if ab else ''}"
                with form_ctx(ops, v3, wps, ab):
                    o, lse = c.forward(ops, what)
                    G = c.grads(o.t)
                    got = c.backward(v3, o, lse, what)
                    r = ra.event_check(got, G, D, lambda nm, g, R, F, RA: ra.mfma_bound(g, R, F))
                    assert max(r.values()) <= 1.0, (what, r)
                    _bump(worst, fam, r)
                    g, R, _, _ = G["dv"]
                    strict = ((got[:, 2 * D:].to(F64) - g).abs() <= ra.C_REL * (g.abs() + R)) | (R == 0)
                    assert strict.all(), f"{what}: dV outside 1.25 2^-8 (|g| + R)"
                    # lse pad entries and the scratch zero instead of NaN: the same bits
                    lz = ra_clone(lse)
                    lz.t[c.pad] = 0.0
                    assert same_bits(c.backward(v3, o, lz, what + " zero pads", scratch_fill=0.0), got), f"{what}: NaN pads change the result"
                    # rotated back
                    rot = c.backward(v3, o, lse, what + " rotated", cos=cos, sin=sin)
                    assert same_bits(rot[:, 2 * D:], got[:, 2 * D:]), f"{what}: rotation changed dV"
                    Gr = rotated(G, cos, sin, B, S, H)
                    r = ra.event_check(rot, Gr, D, lambda nm, g, b, *_: b)
                    assert max(r.values()) <= 1.0, (what, "rotated back", r)
                    _bump(worst_rot, fam, r)
                    if ops.attn_bwd_scaled_ok(c.qkv.t):
                        Gs = scaled(G, c.rs)
                        sc = c.backward(v3, o, lse, what + " rowscale", rowscale=c.rs)
                        r = ra.event_check(sc, Gs, D, lambda nm, g, b, *_: b)
                        assert max(r.values()) <= 1.0, (what, "rowscale", r)
                        _bump(worst_rs, fam, r)
                        assert (sc[c.rs == 0] == 0).all(), f"{what}: a zero-scaled row is not zero"
                        scr = c.backward(v3, o, lse, what + " rowscale rotated", rowscale=c.rs, cos=cos, sin=sin)
                        r = ra.event_check(scr, rotated(Gs, cos, sin, B, S, H, bounds=True), D, lambda nm, g, b, *_: b)
                        assert max(r.values()) <= 1.0, (what, "rowscale, rotated back", r)
                    if fam == "gauss":
                        via_ops = torch.full_like(got, NAN)
                        ops.attn_bwd(c.qkv.t, o.t, c.do.t, lse.t, via_ops, B, S, H, ra.SCALE)
                        assert same_bits(via_ops, got), f"{what}: ops.attn_bwd differs from the same calls made here"
                        for b in range(B if B > 1 else 0):
                            one = c.backward(v3, o, lse, what + f" batch element {b} alone", rows_of=b)
                            assert same_bits(one, got[b * S:(b + 1) * S]), f"{what}: batch element {b} alone differs"
                    if not ab:
                        first = by_v3.setdefault(v3, (o, lse, got, wps))
                        if first[3] != wps:
                            o0, lse0, got0, _ = first
                            mine = got if same_bits(o0.t, o.t) and same_bits(lse0.t[~c.pad], lse.t[~c.pad]) else c.backward(v3, o0, lse0, what + " on the first wps' o")
                            assert same_bits(mine, got0), f"{what}: differs from attn_v3_wps={first[3]}"
            n_bwd += c.n_bwd
    print(f"S={S}: {n_bwd} backward calls over {len(BH_LIST) * len(ra.FAMILIES)} inputs x {len(BWD_FORMS)} forms")
    for nm, w in (("plain", worst), ("rotated back", worst_rot), ("rowscale", worst_rs)):
        print(f"S={S} backward {nm}: worst err/bound " + ", ".join(f"{f}/{g} {v:.3f}" for (f, g), v in sorted(w.items())))


def ra_clone(buf):
    return Buf(tuple(buf.t.shape), buf.t.dtype, src=buf.t)


def scaled(G, rs):
    """grads() dict -> {name: (g rs, |rs| x the unscaled bound)}"""
    return {nm: (ra.scale_rows(g, rs), ra.scale_rows(ra.mfma_bound(g, R, F), rs.abs()), None, None) for nm, (g, R, F, RA) in G.items()}


def rotated(G, cos, sin, B, S, H, bounds=False):
    """{name: (rotated-back float64 gradient, its bound)}; bounds: G already holds (g, bound) pairs (scaled())"""
    out = {}
    for nm, (g, R, F, RA) in G.items():
        b = R if bounds else ra.mfma_bound(g, R, F)
        if nm != "dv":
            y = ra.rot_back64(g, cos, sin, B, S, H)
            g, b = y, ra.rot_bound(b, g, y, cos, sin, B, S, H)
        out[nm] = (g, b, None, None)
    return out


# -------------------------------------------------------------------------------------------------- 2. bf16 MFMA forward
@pytest.mark.parametrize("S", ra.S_LIST)
def test_event_forward_against_float64(ops, S):
    """every forward form of ATTN_FORMS x BH_LIST x the three families: o and lse inside ref_attention.fwd_ratios (FWD_BOUND of
    test_cache_attention_gpu.py; module docstring of ref_attention for the P-rounding term), every row of o written, lse's pad
    entries [S, Sp) untouched (NaN sentinel kept), guards intact.  The spike families send the lazy reference maximum through
    its slow path at every row."""
    worst = {}
    for B, H in BH_LIST:
        for fam in ra.FAMILIES:
            c = EventCase(fam, B, S, H, 5000 + 7 * S + B, backward=False)
            ref = ra.fwd64(c.qkv.t, B, S, H)
            for form, (v3, wps) in ATTN_FORMS.items():
                what = f"S={S} B={B} H={H} {fam} {form}"
                with form_ctx(ops, v3, wps, form == "first_form"):
                    o, lse = c.forward(ops, what)
                r = ra.fwd_ratios(o.t, lse.t.view(B, H, c.Sp)[:, :, :S], ref, BF16)
                assert max(r) <= 1.0, (what, r)
                worst[fam] = tuple(max(a, b) for a, b in zip(worst.get(fam, (0.0, 0.0)), r))
    print(f"S={S} forward: worst err/bound (o, lse) " + ", ".join(f"{f} ({v[0]:.3f}, {v[1]:.3f})" for f, v in sorted(worst.items())))


# ----------------------------------------------------------------------------------------------------- 3. plain kernels
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("S", ra.PLAIN_S)
def test_plain_kernels_against_float64(ops, S, dtype):
    """mh_attn_fwd_plain, then mh_attn_prep_bwd (delta only) + mh_attn_bwd_plain on its o and lse.  The kernels compute in fp32 and
    round only what they store (from_f<T>): forward under FWD_BOUND of the dtype, backward under ref_attention.plain_bound with P from
    the lse the kernel is handed (it does not renormalise) and delta from the stored O; bf16 inputs take the same route with E_T = 2^-8."""
    code = 1 if dtype == BF16 else 0
    worst, worst_f = {}, (0.0, 0.0)
    for B, H in [(1, 1), (3, 3)]:
        D, Sp, M = H * 64, (S + 63) // 64 * 64, B * S
        pad = pad_mask(B, S, H, Sp)
        for fam in ra.FAMILIES:
            what = f"plain {dtype} S={S} B={B} H={H} {fam}"
            qkv, do = ra.event_inputs(fam, B, S, H, dtype, 6000 + 7 * S + B)
            qkv, do = Buf(qkv.shape, dtype, src=qkv.cuda()), Buf(do.shape, dtype, src=do.cuda())
            o, lse, delta, dqkv = Buf((M, D), dtype), Buf((B * H * Sp,), F32), Buf((B * H * Sp,), F32), Buf((M, 3 * D), dtype)
            L, st = lib(), stream()
            L.call("mh_attn_fwd_plain", qkv.t.data_ptr(), o.t.data_ptr(), lse.t.data_ptr(), B, S, H, ra.SCALE, code, st)
            L.call("mh_attn_prep_bwd", qkv.t.data_ptr(), o.t.data_ptr(), do.t.data_ptr(), delta.t.data_ptr(), 0, 0, 0, B, S, H, code, st)
            L.call("mh_attn_bwd_plain", qkv.t.data_ptr(), do.t.data_ptr(), lse.t.data_ptr(), delta.t.data_ptr(), dqkv.t.data_ptr(), B, S, H,
                   ra.SCALE, code, st)
            check_guards(what, qkv, do, o, lse, delta, dqkv)
            assert not torch.isnan(o.t).any() and not torch.isnan(dqkv.t).any(), f"{what}: unwritten (or NaN) results"
            assert torch.isnan(lse.t[pad]).all() and torch.isnan(delta.t[pad]).all(), f"{what}: pad entries of lse / delta written"
            lse_v = lse.t.view(B, H, Sp)[:, :, :S]
            r = ra.fwd_ratios(o.t, lse_v, ra.fwd64(qkv.t, B, S, H), dtype)
            assert max(r) <= 1.0, (what, "forward", r)
            worst_f = tuple(max(a, b) for a, b in zip(worst_f, r))
            d64 = (do.t.to(F64) * o.t.to(F64)).view(B, S, H, 64).sum(-1).permute(0, 2, 1)
            derr = (delta.t.view(B, H, Sp)[:, :, :S].to(F64) - d64).abs()
            dabs = (do.t.to(F64) * o.t.to(F64)).abs().view(B, S, H, 64).sum(-1).permute(0, 2, 1)
            assert (derr <= 66 * ra.U24 * dabs).all(), f"{what}: delta"
            G = ra.Bwd64(qkv.t, do.t, B, S, H, lse=lse_v).grads(o.t)
            r = ra.event_check(dqkv.t, G, D, lambda nm, g, R, F, RA: ra.plain_bound(g, R, F, RA, dtype, S))
            assert max(r.values()) <= 1.0, (what, r)
            _bump(worst, fam, r)
    print(f"plain {dtype} S={S}: forward worst err/bound (o, lse) ({worst_f[0]:.3f}, {worst_f[1]:.3f}); backward "
          + ", ".join(f"{f}/{g} {v:.3f}" for (f, g), v in sorted(worst.items())))


# ------------------------------------------------------------------------------------------------------- 4. token level
# (N, H): N * H mod 4 (four waves per workgroup) = 1, 3, 1, 1, 0, 0 and, with (2, 3), 2
TOK_NH = [(1, 1), (1, 3), (5, 1), (3, 3), (2, 4), (37, 4), (2, 3)]


def tok_run(ops, qkv, do, N, T, H, dtype, cos, sin, rowscale, what):
    D = H * ra.THD
    o, dqkv = Buf((N * T, D), dtype), Buf((N * T, 3 * D), dtype)
    ops.tokattn_fwd(qkv.t, o.t, N, T, H, ra.TSCALE, cos, sin)
    ops.tokattn_bwd(qkv.t, do.t, dqkv.t, N, T, H, ra.TSCALE, cos, sin, rowscale=rowscale)
    check_guards(what, qkv, do, o, dqkv)
    assert not torch.isnan(o.t).any() and not torch.isnan(dqkv.t).any(), f"{what}: unwritten (or NaN) results"
    return o.t, dqkv.t


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("T", range(1, 9))
def test_token_attention_against_float64(ops, T, dtype):
    """mh_tokattn_fwd, mh_tokattn_bwd, mh_tokattn_bwd_scaled (T = 8: the octet form, tokattn_bwd_batched 0 and 1; below: the run-time
    form) x TOK_NH x the three families x with / without RoPE: o and dqkv (the gradient with respect to the UNROTATED q, k) inside the
    float64 bounds of ref_attention.Tok64; the row scale in [0.5, 1.5] plus exactly 0.0 and -1.0, a zero-scaled row exactly zero."""
    from midi_model_amd.engine import RopeTable
    tab = RopeTable(256, 10000.0, "cuda", 8)
    worst = {}
    for N, H in TOK_NH:
        for fam in ra.FAMILIES:
            qkv, do = ra.tok_inputs(fam, N, T, H, dtype, 6500 + 10 * T + N)
            qkv, do = Buf(qkv.shape, dtype, src=qkv.cuda()), Buf(do.shape, dtype, src=do.cuda())
            rs = ra.rowscale_input(N * T, 6600 + T, "cuda")
            for rope in (False, True):
                cos, sin = (tab.cos, tab.sin) if rope else (None, None)
                ref = ra.Tok64(qkv.t, do.t, N, T, H, dtype, cos=cos, sin=sin)
                for batched in ((0, 1) if T == 8 else (1,)):
                    with options(ops, tokattn_bwd_batched=batched):
                        for rowscale in (None, rs):
                            what = f"token {dtype} N={N} T={T} H={H} {fam} rope={rope} batched={batched} rowscale={rowscale is not None}"
                            o, dqkv = tok_run(ops, qkv, do, N, T, H, dtype, cos, sin, rowscale, what)
                            r = dict(ref.bwd_ratios(dqkv, rowscale), o=ref.fwd_ratio(o))
                            assert max(r.values()) <= 1.0, (what, r)
                            _bump(worst, fam, r)
                            if rowscale is not None:
                                assert (dqkv[rs == 0] == 0).all(), f"{what}: a zero-scaled row is not zero"
    print(f"token {dtype} T={T}: worst err/bound " + ", ".join(f"{f}/{g} {v:.3f}" for (f, g), v in sorted(worst.items())))


@pytest.mark.parametrize("case", ["runtime_fp32", "runtime_bf16", "octet_bf16"])
def test_token_attention_past_the_grid_cap(ops, case):
    """N * H > 131072 = 32768 workgroups x 4 waves: the grid-stride loop runs a second pass.  Every wave is independent, so the
    launch must equal, bit for bit, two launches over the two halves of N (inputs drawn on the device; with RoPE and the row scale).
    The octet case holds ~1.6 GB per qkv-sized buffer: allocated and freed here."""
    from midi_model_amd.engine import RopeTable
    dtype = F32 if case.endswith("fp32") else BF16
    N, T, H = (32770, 8, 4) if case.startswith("octet") else (131077, 1, 1)
    assert N * H > 131072
    D = H * ra.THD
    g = torch.Generator(device="cuda").manual_seed(77)
    tab = RopeTable(256, 10000.0, "cuda", 8)
    qkv = Buf((N * T, 3 * D), dtype, src=torch.randn((N * T, 3 * D), generator=g, device="cuda", dtype=dtype))
    do = Buf((N * T, D), dtype, src=torch.randn((N * T, D), generator=g, device="cuda", dtype=dtype))
    rs = 0.5 + torch.rand((N * T,), generator=g, device="cuda")
    o, dqkv = tok_run(ops, qkv, do, N, T, H, dtype, tab.cos, tab.sin, rs, case)
    N1 = N // 2
    for lo, hi in ((0, N1), (N1, N)):
        n, r0, r1 = hi - lo, lo * T, hi * T
        o2, dq2 = Buf((n * T, D), dtype), Buf((n * T, 3 * D), dtype)
        ops.tokattn_fwd(qkv.t[r0:r1], o2.t, n, T, H, ra.TSCALE, tab.cos, tab.sin)
        ops.tokattn_bwd(qkv.t[r0:r1], do.t[r0:r1], dq2.t, n, T, H, ra.TSCALE, tab.cos, tab.sin, rowscale=rs[r0:r1].contiguous())
        check_guards(f"{case} rows [{r0}, {r1})", o2, dq2, qkv, do)
        assert same_bits(o2.t, o[r0:r1]), f"{case}: o of sequences [{lo}, {hi}) differs from the launch over them alone"
        assert same_bits(dq2.t, dqkv[r0:r1]), f"{case}: dqkv of sequences [{lo}, {hi}) differs from the launch over them alone"
        del o2, dq2
    del qkv, do, o, dqkv
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------- 5. refusals
def test_training_attention_refuses_what_it_cannot_serve(ops):
    """An error at the call, nothing launched: the token-level entry points with T = 0, T = 9 or N = 0; mh_tokattn_bwd_scaled
    without a row scale; mh_attn_bwd_o in fp32; mh_attn_bwd with S * 3 * H * 64 >= 2^31 (the third-form kernels address a (batch,
    head) panel with 32-bit offsets; mh_attn_bwd_mfma3 checks before its first launch, so tiny dummy buffers are never touched)."""
    L, st = lib(), stream()
    H = 2
    D = H * ra.THD
    for code, dtype in ((0, F32), (1, BF16)):
        qkv, do = torch.zeros((8, 3 * D), dtype=dtype, device="cuda"), torch.zeros((8, D), dtype=dtype, device="cuda")
        o, dqkv = torch.full_like(do, NAN), torch.full_like(qkv, NAN)
        rs = torch.ones(8, device="cuda")
        for N, T in ((1, 0), (1, 9), (0, 8), (0, 1)):
            with pytest.raises(RuntimeError, match="tokattn_fwd: bad shape"):
                L.call("mh_tokattn_fwd", qkv.data_ptr(), o.data_ptr(), N, T, H, ra.TSCALE, 0, 0, code, st)
            with pytest.raises(RuntimeError, match="tokattn_bwd: bad shape"):
                L.call("mh_tokattn_bwd", qkv.data_ptr(), do.data_ptr(), dqkv.data_ptr(), N, T, H, ra.TSCALE, 0, 0, code, st)
            with pytest.raises(RuntimeError, match="tokattn_bwd: bad shape"):
                L.call("mh_tokattn_bwd_scaled", qkv.data_ptr(), do.data_ptr(), dqkv.data_ptr(), rs.data_ptr(), N, T, H, ra.TSCALE, 0, 0, code, st)
        with pytest.raises(RuntimeError, match="rowscale is NULL"):
            L.call("mh_tokattn_bwd_scaled", qkv.data_ptr(), do.data_ptr(), dqkv.data_ptr(), 0, 1, 8, H, ra.TSCALE, 0, 0, code, st)
        torch.cuda.synchronize()
        assert torch.isnan(o).all() and torch.isnan(dqkv).all()
    B, S, He = 1, 8, 1
    qkv = torch.zeros((B * S, 3 * 64), dtype=F32, device="cuda")
    o = torch.zeros((B * S, 64), dtype=F32, device="cuda")
    do = torch.zeros((B * S, 64), dtype=F32, device="cuda")
    dqkv = torch.full((B * S, 3 * 64), NAN, dtype=F32, device="cuda")
    lse, scratch = torch.zeros(64, device="cuda"), torch.zeros(128, device="cuda")
    with pytest.raises(RuntimeError, match="bf16 only"):
        L.call("mh_attn_bwd_o", qkv.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(), scratch.data_ptr(), dqkv.data_ptr(), B, S, He,
               ra.SCALE, 0, 0, 0, st)
    # S * 3 * H * 64 >= 2^31 with S < 2^24 and B * H < 65536: H = 1024, S = 10923 (10922 would pass the check)
    S_big, H_big = 10923, 1024
    assert S_big * 3 * H_big * 64 >= 2 ** 31 > (S_big - 1) * 3 * H_big * 64
    assert ops.get_option("attn_v3") == 255
    tiny = torch.zeros(64, dtype=BF16, device="cuda")
    with pytest.raises(RuntimeError, match="sequence too long"):
        L.call("mh_attn_bwd", tiny.data_ptr(), tiny.data_ptr(), lse.data_ptr(), scratch.data_ptr(), 0, 0, 0, tiny.data_ptr(), 1, S_big, H_big,
               ra.SCALE, 0, 0, 1, st)
    torch.cuda.synchronize()
    assert torch.isnan(dqkv).all() and (tiny == 0).all()
