"""CPU proof of the bounds of tests/ref_attention.py (the GPU file tests/test_attention_train_gpu.py applies the same bounds to
the HIP kernels): the torch restatement of every kernel family lies inside every bound at every listed shape, each named wrong
variant of it lies outside at the shapes where it changes the arithmetic at all (a variant that changes nothing at a shape is
shown to agree bit for bit there), the recorded A_f32 ratios still hold, and the bound is non-zero at S = 1 and S = 2.
Run with -s for the accept / reject table."""
import functools

import pytest
import torch

import ref_attention as ra

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
MODES = {"mfma": (BF16, ra.S_LIST), "plain": (F32, ra.PLAIN_S), "plain_bf16": (BF16, ra.PLAIN_S)}
# wrong variants a mode can show: the plain kernels round nothing but the store and have neither a row scale nor a rotation
ROWSCALE_WRONG, ROT_WRONG = ("rowscale_after_rounding",), ("rot_wrong_sign", "rot_pos_off_by_one")
NO_PLAIN = ("p_not_rounded",) + ROWSCALE_WRONG + ROT_WRONG


def same_bits(a, b):
    v = torch.int16 if a.element_size() == 2 else torch.int32
    return torch.equal(a.contiguous().view(v), b.contiguous().view(v))


@functools.lru_cache(maxsize=None)
def event_case(mode, S, fam):
    dtype = MODES[mode][0]
    kmode = "mfma" if mode == "mfma" else "plain"
    qkv, do = ra.event_inputs(fam, 1, S, 1, dtype, 9000 + S)
    o, lse, o_unr = ra.restate_fwd(qkv, 1, S, 1, dtype)
    G = ra.Bwd64(qkv, do, 1, S, 1, lse=None if kmode == "mfma" else lse).grads(o)
    rs = ra.rowscale_input(S, 9100 + S)
    cos, sin = ra.rope_table(64, S + 1)
    return dict(dtype=dtype, kmode=kmode, qkv=qkv, do=do, o=o, lse=lse, o_unr=o_unr, G=G, rs=rs, cos=cos, sin=sin)


def event_ratios(mode, S, fam, wrong=None, rowscale=False, rot=False):
    """(restated dqkv, {dq, dk, dv: err/bound}) of the restatement (or a wrong variant of it) in one configuration"""
    c = event_case(mode, S, fam)
    kw = dict(rowscale=c["rs"] if rowscale else None, cos=c["cos"] if rot else None, sin=c["sin"] if rot else None)
    got = ra.restate_bwd(c["qkv"], c["o"], c["do"], c["lse"], 1, S, 1, c["dtype"], c["kmode"], wrong=wrong, o_unrounded=c["o_unr"], **kw)

    def bound(nm, g, R, F, RA):
        return ra.mfma_bound(g, R, F) if mode == "mfma" else ra.plain_bound(g, R, F, RA, c["dtype"], S)

    G = c["G"]
    if rowscale or rot:
        G2 = {}
        for nm, (g, R, F, RA) in G.items():
            b = bound(nm, g, R, F, RA)
            if rowscale:
                g, b = ra.scale_rows(g, c["rs"]), ra.scale_rows(b, c["rs"].abs())
            if rot and nm != "dv":
                y = ra.rot_back64(g, c["cos"], c["sin"], 1, S, 1)
                g, b = y, ra.rot_bound(b, g, y, c["cos"], c["sin"], 1, S, 1)
            G2[nm] = (g, b, None, None)
        return got, ra.event_check(got, G2, ra.HD, lambda nm, g, b, *_: b)
    return got, ra.event_check(got, G, ra.HD, bound)


def config_of(wrong):
    return dict(rowscale=wrong in ROWSCALE_WRONG, rot=wrong in ROT_WRONG)


@pytest.mark.parametrize("mode", list(MODES))
def test_event_restatement_is_inside_and_wrong_variants_are_outside(mode):
    """Every S of the GPU file's list x the three families, B * H = 1.  The restatement is inside the bound plain, with the row scale,
    rotated back, and both (MFMA mode).  Every wrong variant is rejected (ratio > 1) by some family at every S >= 33 where it
    changes the arithmetic; where it does not, it equals the restatement bit for bit.  p_not_rounded must be ACCEPTED;
    rowscale_after_rounding is one extra rounding of the stored value (<= 2^-8 of it) and is reported, not required either way."""
    dtype, s_list = MODES[mode]
    worst_ok = worst_fwd = 0.0
    configs = [dict()] if mode != "mfma" else [dict(), dict(rowscale=True), dict(rot=True), dict(rowscale=True, rot=True)]
    for S in s_list:
        for fam in ra.FAMILIES:
            for cfg in configs:
                _, r = event_ratios(mode, S, fam, **cfg)
                assert max(r.values()) <= 1.0, (mode, S, fam, cfg, r)
                worst_ok = max(worst_ok, *r.values())
            c = event_case(mode, S, fam)
            ref = ra.fwd64(c["qkv"], 1, S, 1)
            fwds = []
            if mode != "plain_bf16":   # the forward restatement under FWD_BOUND (bf16: P rounded for the PV product, as the MFMA kernels do)
                fwds.append(("forward", (c["o"], c["lse"])))
            if mode != "mfma":         # the plain kernel's own order (q scale, sequential dot, key-by-key online softmax; only O rounded)
                fwds.append(("forward, kernel order", ra.restate_plain_fwd(c["qkv"], 1, S, 1, dtype)))
            for nm, (o, lse) in fwds:
                fr = ra.fwd_ratios(o, lse, ref, dtype)
                assert max(fr) <= 1.0, (mode, S, fam, nm, fr)
                worst_fwd = max(worst_fwd, *fr)
    print(f"\n{mode}: worst accepted err/bound {worst_ok:.3f} (backward), {worst_fwd:.3f} (forward)")
    wrongs = [w for w in ra.WRONG_EVENT if mode == "mfma" or w not in NO_PLAIN]
    for w in wrongs:
        cfg = config_of(w)
        smallest, at, vacuous = float("inf"), None, []
        for S in s_list:
            best, changed = 0.0, False
            for fam in ra.FAMILIES:
                base, _ = event_ratios(mode, S, fam, **cfg)
                got, r = event_ratios(mode, S, fam, wrong=w, **cfg)
                if same_bits(got, base):
                    continue
                changed = True
                best = max(best, *r.values())
                if w == "rowscale_after_rounding":
                    d = (got.to(F64) - base.to(F64)).abs()
                    assert (d <= 2.0 ** -7 * base.to(F64).abs()).all(), (S, fam)   # one more rounding: at most one ulp
            if not changed:
                vacuous.append(S)
                continue
            if w in ra.ACCEPTED_WRONG:
                assert best <= 1.0, (mode, w, S, best)
            elif S >= 33 and w not in ROWSCALE_WRONG:
                assert best > 1.0, f"{mode}: {w} is not rejected by any family at S = {S} (largest ratio {best:.3f})"
            if S >= 33 and best < smallest:
                smallest, at = best, S
        kind = "largest (must be accepted)" if w in ra.ACCEPTED_WRONG else "smallest rejected"
        print(f"{mode}: {w:26s} {kind} ratio over S >= 33: {smallest:10.3g} at S = {at}; no change (bit-equal) at S = {vacuous}")
        # (fp32 stores O unrounded: the delta variant cannot show there; every other pair must show somewhere)
        assert at is not None or (mode, w) == ("plain", "delta_unrounded_o"), f"{mode}: {w} never changes the arithmetic on the listed shapes"


def test_share_of_wrong_variants_that_gauss_alone_lets_through():
    """What the spike families are for: the (variant, S >= 33) pairs that change the arithmetic and that the gaussian family alone
    does not reject.  The share is printed; every such pair is rejected by another family (test above)."""
    missed, total = [], 0
    for w in ra.WRONG_EVENT:
        if w in ra.ACCEPTED_WRONG or w in ROWSCALE_WRONG:
            continue
        cfg = config_of(w)
        for S in (s for s in ra.S_LIST if s >= 33):
            base, _ = event_ratios("mfma", S, "gauss", **cfg)
            got, r = event_ratios("mfma", S, "gauss", wrong=w, **cfg)
            if same_bits(got, base):
                continue
            total += 1
            if max(r.values()) <= 1.0:
                missed.append((w, S, round(max(r.values()), 3)))
    print(f"\ngauss alone lets through {len(missed)} of {total} (variant, S) pairs: {missed}")
    assert total > 0


@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("mode", list(MODES))
def test_bound_is_not_zero_where_the_restatement_is_not(mode, S):
    """the regression test of the cancellation term: at S = 1 the reference's dS is exactly 0 while dP - delta leaves ~1e-8"""
    for fam in ra.FAMILIES:
        c = event_case(mode, S, fam)
        got, _ = event_ratios(mode, S, fam)
        for n, nm in enumerate(("dq", "dk", "dv")):
            g, R, F, RA = c["G"][nm]
            b = ra.mfma_bound(g, R, F) if mode == "mfma" else ra.plain_bound(g, R, F, RA, c["dtype"], S)
            x = got[:, n * ra.HD:(n + 1) * ra.HD].to(F64)
            assert (b[x != 0] > 0).all(), (mode, S, fam, nm)
        if S == 1 and mode == "mfma":   # the old bound (no cancellation term) is zero here
            g, R, F, RA = c["G"]["dq"]
            assert (ra.C_REL * (g.abs() + R) + ra.C_RMS * ra.rms(g) == 0).all() and (F > 0).all()


def test_recorded_a_f32_ratios_still_hold():
    got = ra.measure_a_f32()
    print("\nmeasured A_f32 ratios:", {k: f"{v:.2e}" for k, v in got.items()})
    for op, v in got.items():
        assert v <= ra.A_TABLE[op][0], f"{op}: measured ratio {v:.3e} above the recorded {ra.A_TABLE[op][0]:.3e}"
        assert v >= 0.1 * ra.A_TABLE[op][0], f"{op}: recorded ratio {ra.A_TABLE[op][0]:.3e} is stale (measured {v:.3e})"


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
def test_token_restatement_is_inside_and_wrong_variants_are_outside(dtype):
    """Every T in 1 .. 8 x the three families x with / without RoPE x with / without the row scale, N = 3, H = 3 (N * H = 9).
    key_i_plus_1_visible changes nothing at T = 1 and t_treated_as_8 nothing at T = 8 (bit-equal); elsewhere some family rejects."""
    N, H = 3, 3
    cos, sin = ra.rope_table(ra.THD, 8)
    worst_ok, smallest = 0.0, {w: (float("inf"), None) for w in ra.WRONG_TOK}
    for T in range(1, 9):
        best = {w: None for w in ra.WRONG_TOK}
        for fam in ra.FAMILIES:
            qkv, do = ra.tok_inputs(fam, N, T, H, dtype, 9200 + T)
            rs = ra.rowscale_input(N * T, 9300 + T)
            for rope in (False, True):
                kw = dict(cos=cos, sin=sin) if rope else {}
                ref = ra.Tok64(qkv, do, N, T, H, dtype, **kw)
                for rowscale in (None, rs):
                    o, dqkv = ra.restate_tok(qkv, do, N, T, H, dtype, rowscale=rowscale, **kw)
                    r = max(ref.fwd_ratio(o), *ref.bwd_ratios(dqkv, rowscale).values())
                    assert r <= 1.0, (T, fam, rope, rowscale is not None, r)
                    worst_ok = max(worst_ok, r)
                if T <= 2:   # non-zero bound wherever the restatement is non-zero
                    o, dqkv = ra.restate_tok(qkv, do, N, T, H, dtype, **kw)
                    assert max(ref.bwd_ratios(dqkv).values()) < float("inf")
                base = ra.restate_tok(qkv, do, N, T, H, dtype, **kw)
                for w in ra.WRONG_TOK:
                    o, dqkv = ra.restate_tok(qkv, do, N, T, H, dtype, wrong=w, **kw)
                    if same_bits(o, base[0]) and same_bits(dqkv, base[1]):
                        continue
                    r = max(ref.fwd_ratio(o), *ref.bwd_ratios(dqkv).values())
                    best[w] = max(best[w] or 0.0, r)
        for w, b in best.items():
            if b is None:
                assert (w, T) in (("key_i_plus_1_visible", 1), ("t_treated_as_8", 8)), (w, T)
                continue
            assert b > 1.0, f"{w} is not rejected by any family at T = {T} (largest ratio {b:.3f})"
            if b < smallest[w][0]:
                smallest[w] = (b, T)
    print(f"\ntoken {dtype}: worst accepted err/bound {worst_ok:.3f}; smallest rejected ratio "
          + ", ".join(f"{w} {b:.3g} at T = {t}" for w, (b, t) in smallest.items()))
