"""mh_sample_top_p_k_rows_logp / mh_sample_top_p_k_seeded_logp on the MI355X: the ids are the plain forms' bit for bit, the new
output is within the derived bound B (tests/ref_logp.py) of the float64 definition, it writes exactly the floats it is handed, and
it is the MODEL's log-probability -- nothing of a row's sampling settings or of its neighbours moves it.  B = 3 rows throughout."""
import pytest
import torch

import midi_model_amd as mm
import ref_logp as rl

pytestmark = pytest.mark.gpu

B = 3
SENT = -7
POISON = 1234.5
TEMP, TOP_P, TOP_K = (0.7, 1.0, 1.6), (0.9, 0.98, 1.0), (5, 20, 64)   # a set of settings per row


@pytest.fixture(scope="module")
def ops():
    import midi_model_amd.ops as real
    return real


@pytest.fixture(scope="module")
def grammar():
    from midi_model_amd.tokenizer import grammar_tables
    tok = mm.MIDITokenizerV2()
    first, lo, hi, arity = grammar_tables(tok)
    return (tok, torch.tensor(first, dtype=torch.uint8), torch.tensor(lo, dtype=torch.int32), torch.tensor(hi, dtype=torch.int32),
            arity)


def dev(v, ty):
    return torch.tensor(v, dtype=ty, device="cuda")


def settings(temp=TEMP, top_p=TOP_P, top_k=TOP_K):
    return dev(temp, torch.float32), dev(top_p, torch.float32), dev(top_k, torch.int32)


def launch(ops, form, logp, logits, first, ban, lo, hi, ev, pos, V, span, max_range, sets=None, seed=(11, 12, 13), ctr=(3, 40, 7),
           q=None, stride=1, fill_rest=0):
    """one launch of the plain form (logp False) or the _logp form over the B rows -> (out, out_b, out_c [, logp buffer [B + 2,
    stride], poisoned]); sentinels around every output are checked"""
    t, p, k = sets if sets is not None else settings()
    buf = torch.full((B + 2, fill_rest + 1), SENT, dtype=torch.int64, device="cuda")
    ob = torch.full((B + 2,), SENT, dtype=torch.int64, device="cuda")
    oc = torch.full((B + 2,), SENT, dtype=torch.int64, device="cuda")
    kw = dict(out_b=ob[1:1 + B], out_c=oc[1:1 + B], first_span=span, max_range=max_range, fill_rest=fill_rest, fill_id=-3)
    noise = (dev(list(seed), torch.int64), dev(list(ctr), torch.int32)) if form == "seeded" else (q,)
    lp = torch.full((B + 2, stride), POISON, dtype=torch.float32, device="cuda")
    name = "sample_top_p_k_" + form + ("_logp" if logp else "")
    extra = (lp[1:1 + B, stride - 1],) if logp else ()
    getattr(ops, name)(logits, first, lo, hi, ev, pos, *noise, buf[1:1 + B, 0], V, t, p, k, ban, *extra, **kw)
    torch.cuda.synchronize()
    assert bool((buf[0] == SENT).all()) and bool((buf[-1] == SENT).all()) and bool((buf[1:1 + B, 1:] == -3).all())
    for o in (ob, oc):
        assert o[0].item() == SENT and o[-1].item() == SENT
    return (buf[1:1 + B, 0].cpu(), ob[1:1 + B].cpu(), oc[1:1 + B].cpu()) + ((lp.cpu(),) if logp else ())


def check_values(lp, stride, logits, ids, V, what):
    """exactly the B addressed floats changed, each within B of logp64; -> the worst fraction of the bound"""
    mask = torch.ones_like(lp, dtype=torch.bool)
    mask[1:1 + B, stride - 1] = False
    assert bool((lp[mask] == POISON).all()), f"{what}: a float outside the B addressed ones was written"
    got = lp[1:1 + B, stride - 1].double()
    z = logits.cpu()
    want, bound = rl.logp64(z, ids, V), rl.bound(z, ids, V)
    frac = ((got - want).abs() / bound)
    print(f"{what}: worst {float(frac.max()):.3f} of the bound")
    assert bool((frac < 1).all()), (what, got.tolist(), want.tolist(), bound.tolist())
    return float(frac.max())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("form", ["rows", "seeded"])
def test_every_position_of_the_v2_grammar(ops, grammar, form, dtype):
    """token positions 0..7 (every TMAX instantiation), V = 3406 in rows of the padded vocabulary with NaN in the padding columns: ids
    bit-equal to the plain form, values under B, poisoned buffers at strides 1 and T"""
    tok, first, lo, hi, arity = grammar
    V, T = tok.vocab_size, tok.max_token_seq
    Vp = (V + 63) // 64 * 64
    span, ranges = ops.mask_spans(first, lo, hi)
    g = torch.Generator().manual_seed(3)
    by_arity = sorted(range(V), key=lambda i: -arity[i])
    small = min((a, i) for i, a in enumerate(arity) if a > 0)[1]   # (row 2 samples the pad id past its few parameters)
    ev = dev([by_arity[0], by_arity[1], small], torch.int64)
    fm = first[None].repeat(B, 1).cuda()
    ban = torch.zeros((B, V), dtype=torch.uint8)
    ban[1, ::3] = 1   # row 1: a ban mask of its own
    ban[1, tok.pad_id] = 0
    ban = ban.cuda()
    lo_d, hi_d = lo.cuda(), hi.cuda()
    spans = set()
    for pos in range(T):
        z = torch.full((B, Vp), float("nan"))
        z[:, :V] = (torch.randn((B, V), generator=g) * 4).bfloat16().float()
        z = z.to(dtype).cuda()
        q = torch.empty((B, V)).exponential_(1.0, generator=g).cuda()
        width = span[1] - span[0] if pos == 0 else ranges[pos]
        spans.add(2 if width <= 128 else 8 if width <= 512 else 32)
        a = (ops, form)
        b = (z, fm, ban, lo_d, hi_d, ev, pos, V, span, ranges[pos])
        fr = T - 1 if pos == 0 else 0
        plain = launch(*a, False, *b, q=q, fill_rest=fr)
        for stride in (1, T):
            got = launch(*a, True, *b, q=q, stride=stride, fill_rest=fr)
            for x, y in zip(plain, got[:3]):
                assert torch.equal(x, y), (pos, stride, x, y)
            check_values(got[3], stride, z, got[0], V, f"{form} pos {pos} stride {stride}")
        assert bool((plain[0] < V).all()) and bool((ban.cpu().gather(1, plain[0][:, None]) == 0).all())
    assert spans == {2, 8, 32}, spans


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("V", [64, 257, 3585, 7169])
def test_synthetic_tables_and_row_kinds(ops, V, dtype):
    """every row kind at the sizes around the 3584-id batch, at position 0 (a first mask per row) and at position 1 (a range table):
    the chosen id at the row's argmax (top_k 1) and away from it (the argmax banned; seeded noise at temperature 3)"""
    n = min(V, 2048)
    first = torch.zeros((B, V), dtype=torch.uint8)
    first[:, V - n:] = 1                      # the last n ids: a span that ends at V
    span = (V - n, V)
    lo = torch.tensor([[0, max(V - 100, 0)]], dtype=torch.int32)
    hi = torch.tensor([[0, V + 5]], dtype=torch.int32)   # (clipped at V by the kernel)
    ev = torch.zeros(B, dtype=torch.int64, device="cuda")
    worst = 0.0
    for k0 in range(0, len(rl.ROW_KINDS), B):
        kinds = rl.ROW_KINDS[k0:k0 + B]
        z = torch.stack([rl.make_row(kind, V, seed=7) for kind in kinds]).to(dtype)
        zc = z.cuda()
        q = torch.empty((B, V)).exponential_(1.0, generator=torch.Generator().manual_seed(V)).cuda()
        for pos, lo_h in ((0, V - n), (1, max(V - 100, 0))):
            am = z[:, lo_h:].float().argmax(1) + lo_h     # the argmax among the candidates (first maximum: lowest id)
            for away in (False, True):
                ban = torch.zeros((B, V), dtype=torch.uint8)
                sets = settings(temp=(1.0, 1.0, 1.0), top_k=(1, 1, 1))   # (temp 1: z / temp rounds nothing, no new ties)
                if away:
                    ban[torch.arange(B), am] = 1
                    sets = settings(temp=(3.0, 3.0, 3.0), top_p=(1.0, 1.0, 1.0), top_k=(64, 64, 64))
                for form in ("rows", "seeded"):
                    b = (zc, first.cuda(), ban.cuda(), lo.cuda(), hi.cuda(), ev, pos, V, span, 105)
                    plain = launch(ops, form, False, *b, sets=sets, q=q)
                    got = launch(ops, form, True, *b, sets=sets, q=q)
                    for x, y in zip(plain, got[:3]):
                        assert torch.equal(x, y)
                    if away:
                        assert bool((got[0] != am).all()) and bool((got[0] >= lo_h).all()) and bool((got[0] < V).all())
                    else:   # (a spike outside the candidates leaves them probabilities that underflow: any of them may be drawn)
                        sure = torch.tensor([kind != "spike90" for kind in kinds])
                        assert torch.equal(got[0][sure], am[sure]), (kinds, pos, got[0], am)
                    worst = max(worst, check_values(got[3], 1, zc, got[0], V, f"V={V} {kinds} pos {pos} away {away} {form}"))
    print(f"V={V}: worst {worst:.3f} of the bound")


@pytest.mark.parametrize("form", ["rows", "seeded"])
def test_value_is_the_models_whatever_the_settings_and_neighbours(ops, grammar, form):
    """a first mask that leaves row 1 ONE id fixes its chosen id: its value is bit-equal whatever its own temp / top-p / top-k are,
    and whatever its neighbours' logits, settings and masks are"""
    tok, first, lo, hi, arity = grammar
    V = tok.vocab_size
    span, ranges = ops.mask_spans(first, lo, hi)
    g = torch.Generator().manual_seed(9)
    z = (torch.randn((B, V), generator=g) * 4).bfloat16()
    only = int(first.nonzero()[5])
    fm = first[None].repeat(B, 1)
    fm[1] = 0
    fm[1, only] = 1
    ban = torch.zeros((B, V), dtype=torch.uint8)
    ev = torch.zeros(B, dtype=torch.int64, device="cuda")
    q = torch.empty((B, V)).exponential_(1.0, generator=g)
    seen = []
    for temp, top_p, top_k, other in (((1.0, 1.0, 1.0), (0.98, 0.98, 0.98), (20, 20, 20), 0), ((1.0, 0.3, 1.0), (0.98, 0.1, 0.98), (20, 1, 20), 0),
                                      ((1.0, 2.5, 1.0), (0.98, 1.0, 0.98), (20, 64, 20), 0), ((0.5, 1.0, 2.0), (0.5, 0.98, 1.0), (1, 20, 64), 1)):
        zz = z.clone()
        bb = ban.clone()
        if other:   # the neighbours' logits and masks change as well
            zz[0] = zz[0] * 2 + 1
            zz[2] = -zz[2]
            bb[0, ::2] = 1
            bb[0, only] = 0
        got = launch(ops, form, True, zz.cuda(), fm.cuda(), bb.cuda(), lo.cuda(), hi.cuda(), ev, 0, V, span, ranges[0],
                     sets=settings(temp, top_p, top_k), q=q.cuda())
        assert int(got[0][1]) == only
        seen.append(float(got[3][2, 0]))
    assert len(set(seen)) == 1, seen
    assert abs(seen[0] - float(rl.logp64(z[1], only))) < float(rl.bound(z[1], only))


def test_entry_points_refuse_a_null_logp_and_a_stride_below_one(ops, grammar):
    from midi_model_amd.lib import MH_F32, lib
    tok, first, lo, hi, arity = grammar
    V = tok.vocab_size
    span, ranges = ops.mask_spans(first, lo, hi)
    z = torch.zeros((B, V), device="cuda")
    fm, ban = first.cuda(), torch.zeros(V, dtype=torch.uint8, device="cuda")
    lo_d, hi_d = lo.cuda(), hi.cuda()
    ev = torch.zeros(B, dtype=torch.int64, device="cuda")
    out = torch.zeros(B, dtype=torch.int64, device="cuda")
    t, p, k = settings()
    q = torch.ones((B, V), device="cuda")
    seed, ctr = dev([1, 2, 3], torch.int64), dev([0, 0, 0], torch.int32)
    lp = torch.full((B,), POISON, device="cuda")
    head = [z.data_ptr(), V, fm.data_ptr(), 0, ban.data_ptr(), 0, span[0], span[1], lo_d.data_ptr(), hi_d.data_ptr(), lo.shape[1],
            ranges[0], ev.data_ptr(), 0]
    tail = [out.data_ptr(), 1, 0, 0, B, V, t.data_ptr(), p.data_ptr(), k.data_ptr(), 0, 0, MH_F32, torch.cuda.current_stream().cuda_stream]
    for name, noise in (("mh_sample_top_p_k_rows_logp", [q.data_ptr()]), ("mh_sample_top_p_k_seeded_logp", [seed.data_ptr(), ctr.data_ptr()])):
        good = head + noise + tail + [lp.data_ptr(), 1]
        lib().call(name, *good)
        torch.cuda.synchronize()
        assert bool((lp != POISON).all())
        lp.fill_(POISON)
        out.fill_(SENT)
        for bad, match in ((good[:-2] + [0, 1], r"logp \(float"), (good[:-1] + [0], "logp_stride=0"), (good[:-1] + [-4], "logp_stride=-4")):
            with pytest.raises(RuntimeError, match=match):
                lib().call(name, *bad)
        torch.cuda.synchronize()
        assert bool((lp == POISON).all()) and bool((out == SENT).all()), "a refusal launched something"
    # the wrappers: a logp of the wrong type or shape never reaches the library
    with pytest.raises(AssertionError, match="logp must"):
        ops.sample_top_p_k_rows_logp(z, fm, lo_d, hi_d, ev, 0, q, out, V, t, p, k, ban, lp.double(), first_span=span, max_range=ranges[0])
    with pytest.raises(AssertionError, match="logp must"):
        ops.sample_top_p_k_seeded_logp(z, fm, lo_d, hi_d, ev, 0, seed, ctr, out, V, t, p, k, ban, lp[:2], first_span=span,
                                       max_range=ranges[0])
