"""A seed per request on the MI355X: mh_sample_noise_seeded against ref_philox bit for bit and against float64 -log(u);
mh_sample_top_p_k_seeded against mh_sample_top_p_k_rows fed the generator's own output (no tolerance: past the variate the code is
the same); the distribution of 4096 seeds; and the production session (bf16 tv2o-medium, captured graphs, folded norms, fused
sampler, no noise graph): a request's ids do not depend on its row, its admission step or its neighbours, the pool equals
generate_ragged, no generator is touched, nothing is recaptured for new seeds."""
import copy

import numpy as np
import pytest
import torch

import midi_model_amd as mm

import ragged_common as rc
import ref_philox
import seeded_common as sc

pytestmark = pytest.mark.gpu

SEEDS = (0, 1, (1 << 64) - 1, 0x243f6a8885a308d3)
CTRS = (0, 1, 4095, (1 << 31) - 1)


@pytest.fixture(scope="module")
def ops():
    import midi_model_amd.ops as real
    return real


@pytest.fixture(scope="module")
def tok():
    return mm.MIDITokenizerV2()


@pytest.fixture(scope="module")
def noise(ops):
    """(bits uint32 [8, 4, 64], q float32 [8, 4, 64]) of mh_sample_noise_seeded for SEEDS x CTRS at every token position,
    computed once"""
    from midi_model_amd.ops_seeded import seed_storage
    seed = torch.tensor(seed_storage(SEEDS), dtype=torch.int64, device="cuda")
    ctr = torch.tensor(CTRS, dtype=torch.int32, device="cuda")
    bits, q = [], []
    for pos in range(8):
        guard_b = torch.full((6, 64), -7, dtype=torch.int32, device="cuda")
        guard_q = torch.full((6, 64), -7.0, dtype=torch.float32, device="cuda")
        ops.sample_noise_seeded(seed, ctr, pos, bits=guard_b[1:5], q=guard_q[1:5])
        torch.cuda.synchronize()
        assert bool((guard_b[0] == -7).all() and (guard_b[5] == -7).all() and (guard_q[0] == -7).all() and (guard_q[5] == -7).all())
        bits.append(guard_b[1:5].cpu().numpy().view(np.uint32))
        q.append(guard_q[1:5].cpu().numpy())
    return np.stack(bits), np.stack(q)


def test_generator_bits_are_philox4x32_10(noise):
    """1. all 64 lanes of 4 rows at the 8 positions equal ref_philox exactly; row 0 / pos 0 / lane 0 is Random123's first known
    answer"""
    bits, _ = noise
    assert int(bits[0, 0, 0]) == 0x6627e8d5
    for pos in range(8):
        want = ref_philox.noise(SEEDS, CTRS, pos)[0]
        assert (bits[pos] == want).all(), (pos, np.argwhere(bits[pos] != want)[:4])


def test_variates_are_the_accurate_log(noise):
    """2. q finite and > 0, and within 8 float32 ulps of float64 -log(u), u rebuilt exactly from the bits.  (The fast intrinsic
    is a scaled v_log_f32: its absolute error of about 2^-22 near u = 1, where q is as small as 6e-8, is thousands of ulps.)"""
    bits, q = noise
    assert np.isfinite(q).all() and (q > 0).all()
    want = ref_philox.q_of_bits(bits)
    ulp = np.spacing(want.astype(np.float32)).astype(np.float64)
    dist = np.abs(q.astype(np.float64) - want) / ulp
    print(f"seeded variates: worst distance {dist.max():.3f} float32 ulps of float64 -log(u) over {dist.size} values, "
          f"q in [{q.min():.3e}, {q.max():.3f}]")
    assert dist.max() <= 8.0, (dist.max(), np.argwhere(dist > 8.0)[:4])


def _grammar(tok):
    from midi_model_amd.tokenizer import grammar_tables
    first, lo, hi, _ = grammar_tables(tok)
    return torch.tensor(first, dtype=torch.uint8), torch.tensor(lo, dtype=torch.int32), torch.tensor(hi, dtype=torch.int32)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_same_sampler_as_the_rows_form(ops, tok, dtype):
    """3. the real tokenizer tables, V = 3406, B = 5, every position 0..7 -- `duration` (2048 ids) and `bpm` among the ranges, so
    all three instantiations and the split-wave form run -- per-row top_k {1, 2, 20, 63, 64}, temperatures, top_p, a banned
    channel on one row: out, out_b, out_c and the filled columns of the seeded form are IDENTICAL to the rows form's on a q whose
    first 64 columns are mh_sample_noise_seeded's output"""
    from midi_model_amd.ops_seeded import seed_storage
    V, T, B = tok.vocab_size, tok.max_token_seq, 5
    assert V == 3406
    first, lo, hi = _grammar(tok)
    span, max_range = ops.mask_spans(first, lo, hi)
    assert {2 if r <= 128 else 8 if r <= 512 else 32 for r in max_range[1:]} == {2, 8, 32} and max(max_range) == 2048
    names = ("note", "set_tempo", "control_change", "patch_change", "note")
    ev = torch.tensor([tok.event_ids[n] for n in names], dtype=torch.int64)
    g = torch.Generator().manual_seed(17)
    logits = (torch.randn((B, V), generator=g) * 2.5).to(dtype).cuda()
    ban = torch.zeros((B, V), dtype=torch.uint8)
    ban[4, tok.parameter_ids["channel"][9]] = 1
    ban[4, tok.parameter_ids["channel"][0]] = 1
    firsts = first[None].repeat(B, 1)
    firsts[1, tok.eos_id] = 0
    dev = lambda v, ty: torch.tensor(v, dtype=ty, device="cuda")
    temp, top_p = dev([1.0, 0.6, 1.7, 1.2, 0.9], torch.float32), dev([0.98, 1.0, 0.5, 0.9, 0.98], torch.float32)
    top_k = dev([1, 2, 20, 63, 64], torch.int32)
    seed = dev(seed_storage([77, 0, (1 << 64) - 1, 1 << 63, 12345678901234567890]), torch.int64)
    ctr = dev([17, 0, 4095, 1, 300], torch.int32)
    lo_d, hi_d, ev_d, firsts_d, ban_d = lo.cuda(), hi.cuda(), ev.cuda(), firsts.cuda(), ban.cuda()
    for pos in range(T):
        q = torch.ones((B, V), dtype=torch.float32, device="cuda")
        q[:, :64] = ops.sample_noise_seeded(seed, ctr, pos)[1]
        fill = T - 1 if pos == 0 else 0
        res = []
        for form in ("rows", "seeded"):
            buf = torch.full((B + 2, T), -7, dtype=torch.int64, device="cuda")
            out_b = torch.full((B + 2,), -7, dtype=torch.int64, device="cuda")
            out_c = torch.full((B + 2,), -7, dtype=torch.int64, device="cuda")
            kw = dict(out_b=out_b[1:1 + B], out_c=out_c[1:1 + B], first_span=span, max_range=max_range[pos], fill_rest=fill,
                      fill_id=tok.pad_id)
            if form == "rows":
                ops.sample_top_p_k_rows(logits, firsts_d, lo_d, hi_d, ev_d, pos, q, buf[1:1 + B, 0], V, temp, top_p, top_k, ban_d, **kw)
            else:
                ops.sample_top_p_k_seeded(logits, firsts_d, lo_d, hi_d, ev_d, pos, seed, ctr, buf[1:1 + B, 0], V, temp, top_p, top_k,
                                          ban_d, **kw)
            torch.cuda.synchronize()
            assert bool((buf[0] == -7).all() and (buf[-1] == -7).all() and (buf[1:1 + B, fill + 1:] == -7).all()), (form, pos)
            assert bool((buf[1:1 + B, 1:fill + 1] == tok.pad_id).all()), (form, pos)
            assert out_b[0] == -7 and out_b[-1] == -7 and out_c[0] == -7 and out_c[-1] == -7
            res.append((buf.cpu(), out_b.cpu(), out_c.cpu()))
        for a, b in zip(*res):
            assert torch.equal(a, b), (pos, a.flatten()[:16], b.flatten()[:16])
        ids = res[1][0][1:1 + B, 0]
        assert torch.equal(ids, res[1][1][1:1 + B]) and torch.equal(ids, res[1][2][1:1 + B])
        if pos == 0:
            assert bool(firsts.gather(1, ids[:, None]).all()) and int(ids[1]) != tok.eos_id
        else:
            assert bool(((ids >= lo[ev, pos]) & (ids < hi[ev, pos])).all()), (pos, ids)
            assert int(ban[4, ids[4]]) == 0
    # the entry point refuses a NULL seed and a NULL ctr by name
    from midi_model_amd.lib import MH_BF16, MH_F32, lib
    out = torch.zeros(B, dtype=torch.int64, device="cuda")
    args = [logits.data_ptr(), logits.stride(0), firsts_d.data_ptr(), V, ban_d.data_ptr(), V, span[0], span[1], lo_d.data_ptr(),
            hi_d.data_ptr(), T, max_range[1], ev_d.data_ptr(), 1, seed.data_ptr(), ctr.data_ptr(), out.data_ptr(), 1, 0, 0, B, V,
            temp.data_ptr(), top_p.data_ptr(), top_k.data_ptr(), 0, 0, MH_F32 if dtype == torch.float32 else MH_BF16,
            torch.cuda.current_stream().cuda_stream]
    lib().call("mh_sample_top_p_k_seeded", *args)
    torch.cuda.synchronize()
    for null_at, match in ((14, "seed"), (15, "ctr"), (22, "temp"), (2, "first_mask")):
        bad = list(args)
        bad[null_at] = 0
        with pytest.raises(RuntimeError, match=match):
            lib().call("mh_sample_top_p_k_seeded", *bad)
    for null_at, match in ((0, "seed"), (1, "ctr"), (4, "bits")):
        bad = [seed.data_ptr(), ctr.data_ptr(), 0, B, out.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream]
        bad[null_at] = 0
        with pytest.raises(RuntimeError, match=match):
            lib().call("mh_sample_noise_seeded", *bad)
    with pytest.raises(AssertionError, match="seed must"):
        ops.sample_noise_seeded(seed.int(), ctr, 0)
    with pytest.raises(AssertionError, match="ctr must"):
        ops.sample_noise_seeded(seed, ctr.long(), 0)


def test_distribution_of_4096_seeds(ops, tok):
    """4. seeded_common.distribution_case: 4096 rows, one logit row, six candidates, seeds 0..4095, ctr 0, top_p 1, top_k 6.  The
    ids' chi-square against the filtered probabilities lies below the 1 - 1e-9 quantile at 5 degrees of freedom (50.69; the run
    is deterministic).  The CPU stand-in (emu_seeded) gives 0.948 on these inputs, counts (1662, 1015, 611, 397, 250, 161)."""
    V = tok.vocab_size
    c = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in sc.distribution_case(V).items()}
    out = torch.zeros(sc.DIST_ROWS, dtype=torch.int64, device="cuda")
    ops.sample_top_p_k_seeded(c["logits"], c["first"], c["tabs"], c["tabs"], c["ev"], 0, c["seed"], c["ctr"], out, V, c["temp"],
                              c["top_p"], c["top_k"], c["ban"], first_span=c["span"], max_range=0)
    torch.cuda.synchronize()
    stat, counts = sc.chi_square(out.cpu().numpy(), V)
    bound = sc.chi_square_bound()
    print(f"seeded sampler, 4096 seeds: chi-square {stat:.3f} (bound {bound:.2f}), counts {counts.tolist()}")
    assert stat < bound, (stat, counts)


@pytest.fixture(scope="module")
def medium_bf16(orc, tok):
    shp = orc.Shape(vocab=tok.vocab_size)
    sd = orc.make_state_dict(shp, seed=0)
    m = mm.MIDIModel(mm.MIDIModelConfig.from_name("tv2o-medium"))
    m.load_state_dict(sd, strict=True)
    return m.to("cuda", torch.bfloat16).eval()


def test_end_to_end_on_the_production_session(orc, tok, medium_bf16):
    """5. bf16 tv2o-medium, graphs on, folded norms, fused sampler, seeded session without a noise graph.  (a) X (17 prompt events,
    24 to generate, temp 1.2, top_k 20, seed 77) admitted alone into row 3 of a 4-row pool of capacity 128 behind other neighbours
    after 1 and after 5 steps, into a reused row, and alone into row 0 of an empty pool: identical ids, no tolerance; (b) seed 78
    gives other ids; the same seed repeats id for id; (c) generate_ragged(seed=...) equals the seeded pool that admits the same
    prompts together; (d) a generator standing nearby and the device's default generator keep their state; one session object and
    the same g_net / g_steps objects serve every pool: nothing is recaptured for other seeds and lengths."""
    m = medium_bf16
    m._sessions.idle.clear()
    g = torch.Generator(device="cuda").manual_seed(11)
    s0, d0 = g.get_state(), torch.cuda.default_generators[0].get_state()
    runs = [sc.run_x(m, orc, tok, case) for case in sc.CASES]
    a, ses, graphs = runs[0]
    assert ses.use_graphs and graphs[0] is not None and graphs[1] is not None, "captured graphs are the production form"
    assert ses.seeded and ses.g_noise is None and ses.q_all is None and ses.gen is None
    assert ses.fold1 is not None and ses.fused_sampler and ses.row_params and ses.B == 4 and ses.cap == 256
    for (out, ses_i, graphs_i), case in zip(runs[1:], sc.CASES[1:]):
        assert (out == a).all(), (case, np.argwhere(out != a)[:4])
        assert ses_i is ses and graphs_i[0] is graphs[0] and graphs_i[1] is graphs[1], "the session was recaptured"
    # (b) other seed, other ids; the same seed again, in other surroundings: id for id
    b = sc.run_x(m, orc, tok, "alone_row0", seed=78)[0]
    assert (a != b).any()
    again = sc.run_x(m, orc, tok, "five_steps", seed=77)[0]
    assert (again == a).all()
    # a second pool, other seeds and lengths: the same session and graphs
    ps = rc.prompts(orc, tok, (3, 40, 130, 8), seed0=51)
    res = sc.pool_together(m, ps, (12, 5, 20, 7), (9, 8, 7, 1 << 63), temp=0.9, top_k=30, ban_eos=True)
    assert [len(r) for r in res] == [15, 45, 150, 15] and all((r[:len(p)] == p).all() for r, p in zip(res, ps))
    assert m._sessions.idle == [ses] and ses.g_net is graphs[0] and ses.g_steps is graphs[1] and ses.g_noise is None
    # (c) the pool against generate_ragged, prompts of different lengths
    ps3 = rc.prompts(orc, tok, (3, 11, 6), seed0=400)
    n_gen, seeds = (9, 4, 12), (5, (1 << 64) - 1, 1 << 63)
    x = m.generate_ragged(ps3, max_len=[len(p) + n for p, n in zip(ps3, n_gen)], temp=1.1, top_k=30, ban_eos=True, seed=list(seeds))
    y = sc.pool_together(m, ps3, n_gen, seeds, temp=1.1, top_k=30, ban_eos=True)
    for u, v, p, n in zip(x, y, ps3, n_gen):
        assert u.shape == (len(p) + n, 8) and (u == v).all(), np.argwhere(u != v)[:4]
    assert all(s.seeded and s.g_noise is None for s in m._sessions.idle) and len(m._sessions.idle) == 2
    # (d) no generator was touched
    assert torch.equal(g.get_state(), s0) and torch.equal(torch.cuda.default_generators[0].get_state(), d0)
    with pytest.raises(ValueError, match="generator"):
        m.decode_pool(4, 128, generator=g, seeded=True)
