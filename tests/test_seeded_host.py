"""A seed per request on the CPU: ref_philox against Random123's known answers, and the seeded decode path -- DecodeSession(seeded=True),
generate_ragged(seed=...), decode_pool(seeded=True) / submit(seed=...), generate_pool -- through the fake backend plus the stand-ins
of tests/emu_seeded.py.  Tiny 4-layer model, fp32.  The kernel and the production session: test_seeded_gpu.py."""
import numpy as np
import pytest
import torch

import midi_model_amd as mm

import emu_pool
import emu_rowparams
import emu_seeded
import ragged_common as rc
import ref_philox
import seeded_common as sc

NEW_OPS = ("sample_top_p_k_seeded", "sample_noise_seeded")


@pytest.fixture(scope="module")
def tok():
    return mm.MIDITokenizerV2()


@pytest.fixture(scope="module")
def tiny(orc, tok):
    shp = orc.Shape(n_layer=4, n_head=4, n_embd=256, n_inner=512, vocab=tok.vocab_size)
    return shp, orc.make_state_dict(shp, seed=0)


def _model(sd):
    m = mm.MIDIModel(mm.MIDIModelConfig.get_config("v2", True, 4, 4, 256, 512))
    m.load_state_dict(sd)
    return m.to(torch.float32)


def test_ref_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10: (counter, key) -> output"""
    f = 0xffffffff
    for ctr, key, want in (
            ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
            ((f, f, f, f), (f, f), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
            ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
             (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))):
        assert tuple(int(v) for v in ref_philox.philox4x32_10(ctr, key)) == want
    # batched = one at a time; the sampler's counter layout; the map's ends
    bits, q = ref_philox.noise([0, (1 << 64) - 1, 0x243f6a8885a308d3], [0, 7, (1 << 31) - 1], 3)
    assert bits.shape == (3, 64) and bits.dtype == np.uint32 and int(ref_philox.noise([0], [0], 0)[0][0, 0]) == 0x6627e8d5
    one = ref_philox.philox4x32_10((7, 3, 41, 0), (f, f))
    assert int(bits[1, 41]) == int(one[0])
    assert int(bits[2, 5]) == int(ref_philox.philox4x32_10(((1 << 31) - 1, 3, 5, 0), (0x85a308d3, 0x243f6a88))[0])
    u = ref_philox.u_of_bits(np.array([0, f, 0x1ff, 0x200], dtype=np.uint32))
    assert u.tolist() == [2.0 ** -24, 1 - 2.0 ** -24, 2.0 ** -24, 3 * 2.0 ** -24]
    assert (u.astype(np.float32).astype(np.float64) == u).all() and np.isfinite(q).all() and (q > 0).all()


def test_a_seeded_request_does_not_depend_on_row_step_or_neighbours(orc, tok, tiny):
    """(a) X (temp 1.2, top_k 20, seed 77: sampled, it reads its noise at all 8 positions of 24 events) admitted alone into row 3
    behind other neighbours after 1 step, after 5 steps, into a reused row, and alone into row 0 of an empty pool: identical ids.
    One pooled seeded session serves the four pools."""
    with emu_seeded.install() as log:
        m = _model(tiny[1])
        runs = [sc.run_x(m, orc, tok, case) for case in sc.CASES]
        assert len(m._sessions.idle) == 1 and m._sessions.idle[0] is runs[0][1] and runs[0][1].seeded
        assert "sample_top_p_k_seeded" in log and "sample_top_p_k_rows" not in log
    a = runs[0][0]
    for (out, ses, graphs), case in zip(runs[1:], sc.CASES[1:]):
        assert (out == a).all(), (case, np.argwhere(out != a)[:4])
        assert ses is runs[0][1]


def test_seeds_matter_and_repeat(orc, tok, tiny):
    """(b) seeds 77 and 78 give X different ids (checked with the stand-in on this prompt: the results part within X's first
    generated events), and seed 77 repeats id for id"""
    with emu_seeded.install():
        m = _model(tiny[1])
        a = sc.run_x(m, orc, tok, "alone_row0", seed=77)[0]
        b = sc.run_x(m, orc, tok, "alone_row0", seed=78)[0]
        c = sc.run_x(m, orc, tok, "one_step", seed=77)[0]
    assert (a != b).any() and (a == c).all()
    print(f"seeds 77 / 78: first difference at event {int(np.argwhere(a != b)[0][0])}, {int((a != b).sum())} ids differ")


def test_pool_equals_generate_ragged(orc, tok, tiny):
    """(c) generate_ragged(prompts, seed=[...]) == a seeded pool of the same row count that admits the same prompts together into
    rows 0..B-1 (prompts of different lengths: both prefill them with the packed forward); scalar settings with a seed run the
    seeded per-row session too"""
    ps = rc.prompts(orc, tok, (3, 11, 6), seed0=400)
    n_gen, seeds = (9, 4, 12), (5, (1 << 64) - 1, 1 << 63)
    with emu_seeded.install() as log:
        m = _model(tiny[1])
        a = m.generate_ragged(ps, max_len=[len(p) + n for p, n in zip(ps, n_gen)], temp=1.1, top_k=30, ban_eos=True, seed=list(seeds))
        assert m._sessions.idle[0].seeded and "sample_top_p_k_seeded" in log and "sample_top_p_k_rows" not in log
        b = sc.pool_together(m, ps, n_gen, seeds, temp=1.1, top_k=30, ban_eos=True)
        # generate_pool: every request with a seed -> a seeded pool, the same ids
        c = m.generate_pool([dict(prompt=p, max_len=len(p) + n, temp=1.1, top_k=30, ban_eos=True, seed=s)
                             for p, n, s in zip(ps, n_gen, seeds)], rows=3)
        # scalars + seed: max_len for all rows
        d = m.generate_ragged(ps, max_len=15, temp=1.1, top_k=30, ban_eos=True, seed=list(seeds))
        e = list(m.generate_stream_ragged(ps, max_len=15, temp=1.1, top_k=30, ban_eos=True, seed=list(seeds)))
    for x, y, z, p, n in zip(a, b, c, ps, n_gen):
        assert x.shape == (len(p) + n, 8) and (x == y).all() and (x == z).all()
    assert all(r.shape == (15, 8) for r in d) and len(e) == 12
    # a row's ids do not depend on the other rows' max_len: the common part of a and d
    for x, y, p, n in zip(a, d, ps, n_gen):
        k = min(len(p) + n, 15)
        assert (x[:k] == y[:k]).all()


def test_no_generator_is_touched_and_nothing_is_drawn(orc, tok, tiny, monkeypatch):
    """(d) a torch.Generator standing nearby and the default generator are in the same state after a seeded pool and a seeded
    generate_ragged have run; no exponential_ draw is made; the seeded session has no noise buffer and no noise graph"""
    draws = []
    real = torch.Tensor.exponential_
    monkeypatch.setattr(torch.Tensor, "exponential_", lambda self, *a, **k: (draws.append(tuple(self.shape)), real(self, *a, **k))[1])
    g = torch.Generator().manual_seed(3)
    s0 = g.get_state()
    ps = rc.prompts(orc, tok, (3, 7), seed0=120)
    with emu_seeded.install() as log:
        m = _model(tiny[1])
        del log[:]
        d0 = torch.default_generator.get_state()
        sc.pool_together(m, ps, (6, 3), (1, 2), temp=1.1)
        m.generate_ragged(ps, max_len=12, seed=[4, 5])
        ses = m._sessions.idle[0]
        assert ses.seeded and ses.q_all is None and ses.g_noise is None and ses.gen is None and ses.seed_rows.shape == (2,)
        assert ses.seed_rows.dtype == torch.int64 and ses.seed_rows.tolist() == [4, 5]
        ses.draw_noise()
        ses.consumed(8)
        assert not ses._noise_pending and not draws, draws[:3]
        assert log.count("sample_top_p_k_seeded") > 0 and "sample_top_p_k_rows" not in log
        assert torch.equal(torch.default_generator.get_state(), d0) and torch.equal(g.get_state(), s0)
        # the unseeded pool on the same model does draw (the patch sees it)
        with m.decode_pool(2, 64, generator=g) as pool:
            pool.submit(ps[0], max_len=5)
            pool.step()
        assert draws
    assert not torch.equal(g.get_state(), s0), "the unseeded pool drew from its generator"


def test_the_unseeded_path_runs_what_it_ran(orc, tok, tiny):
    """(e) with seed=None the call log of generate_ragged (scalar and per-row form) and of the pool holds no new op name, is the
    log under emu_pool alone (this feature's stand-ins not installed), and the ids are the same"""
    ps = rc.prompts(orc, tok, (3, 7, 5), seed0=120)

    def run(m):
        out = m.generate_ragged(ps, max_len=12, generator=torch.Generator().manual_seed(1))
        out += m.generate_ragged(ps, max_len=[12, 10, 9], temp=[1.0, 0.7, 1.2], generator=torch.Generator().manual_seed(2), seed=None)
        with m.decode_pool(2, 64, generator=torch.Generator().manual_seed(3)) as pool:
            ids = [pool.submit(p, max_len=len(p) + 4, temp=1.1, seed=None) for p in ps]
            while pool.pending():
                pool.step()
            out += [pool.result(i) for i in ids]
        assert not any(s.seeded for s in m._sessions.idle) and all(s.q_all is not None for s in m._sessions.idle)
        return out

    with emu_pool.install() as log0:
        m = _model(tiny[1])
        del log0[:]
        a, la = run(m), list(log0)
    with emu_seeded.install() as log1:
        m = _model(tiny[1])
        del log1[:]
        b, lb = run(m), list(log1)
    assert la == lb and not any(n in lb for n in NEW_OPS)
    assert all(x.shape == y.shape and (x == y).all() for x, y in zip(a, b))
    # the session keys of the existing forms are what they were
    from midi_model_amd.decode import DecodeSession
    k = DecodeSession.make_key(m, 2, 256, 1.0, 0.98, 1, 0, True, True)
    assert k[-1] == ("ragged", "row_params") and DecodeSession.make_key(m, 2, 256, 1.0, 0.98, 1, 0, True, True, True)[-1][-1] == "seeded"


def test_argument_errors_come_before_any_backend_call(orc, tok, tiny):
    """(f)"""
    from midi_model_amd.decode import DecodeSession
    ps = rc.prompts(orc, tok, (6, 4), seed0=80)
    g = torch.Generator()
    with emu_seeded.install() as log:
        m = _model(tiny[1])
        del log[:]
        for seed, match in (([1], "sequence of 2"), ([1, 2, 3], "sequence of 2"), (7, "sequence of 2"), ([1, True], "row 1"),
                            ([1.0, 2], "row 0"), ([1, -1], "row 1"), ([1 << 64, 2], "row 0"), ([1, "2"], "row 1"),
                            ([None, 2], "row 0")):
            with pytest.raises(ValueError, match=match):
                m.generate_ragged(ps, max_len=9, seed=seed)
            with pytest.raises(ValueError, match=match):
                m.generate_stream_ragged(ps, max_len=9, seed=seed)
        with pytest.raises(ValueError, match="seed and generator"):
            m.generate_ragged(ps, max_len=9, seed=[1, 2], generator=g)
        with pytest.raises(ValueError, match="seed and generator"):
            m.generate_stream_ragged(ps, max_len=9, seed=[1, 2], generator=g)
        with pytest.raises(ValueError, match="temperature"):   # (the other per-row checks still run)
            m.generate_ragged(ps, max_len=9, temp=0.0, seed=[1, 2])
        with pytest.raises(ValueError, match="seeded=True together with a generator"):
            m.decode_pool(2, 64, generator=g, seeded=True)
        pool = m.decode_pool(2, 64, seeded=True)
        for kw, match in ((dict(), "needs a seed"), (dict(seed=None), "needs a seed"), (dict(seed=True), "row 0"),
                          (dict(seed=1.5), "row 0"), (dict(seed=-3), "row 0"), (dict(seed=1 << 64), "row 0"),
                          (dict(seed=[1]), "one seed"), (dict(seed=1, top_k=65), "top_k")):
            with pytest.raises(ValueError, match=match):
                pool.submit(ps[0], max_len=9, **kw)
        assert pool.pending() == 0
        pool.submit(ps[0], max_len=9, seed=(1 << 64) - 1)
        pool.submit(ps[1], max_len=9, seed=np.int64(4))
        assert pool.pending() == 2 and not log and pool.ses is None
        pool.close()
        plain = m.decode_pool(2, 64)
        with pytest.raises(ValueError, match="seeded=True"):
            plain.submit(ps[0], max_len=9, seed=1)
        plain.close()
        with pytest.raises(ValueError, match="1 of 2 requests carry a seed"):
            m.generate_pool([dict(prompt=ps[0], max_len=9, seed=1), dict(prompt=ps[1], max_len=9)], rows=2)
        with pytest.raises(ValueError, match="generator"):
            m.generate_pool([dict(prompt=ps[0], max_len=9, seed=1)], rows=2, generator=g)
        assert not log and not m._sessions.idle
        # the session itself
        for kw in (dict(), dict(ragged=True), dict(row_params=True)):
            with pytest.raises(ValueError, match="seeded"):
                DecodeSession(m, 2, 64, 1.0, 0.98, 1, seeded=True, **kw)
        with torch.inference_mode():
            ses = DecodeSession(m, 2, 64, 1.0, 0.98, 1, ragged=True, row_params=True, seeded=True)
            plain = DecodeSession(m, 2, 64, 1.0, 0.98, 1, ragged=True, row_params=True)
        del log[:]
        assert ses.key != plain.key and ses.key[:-1] == plain.key[:-1]
        V = tok.vocab_size
        masks, toks = torch.zeros((1, V), dtype=torch.uint8), torch.from_numpy(ps[0])
        with pytest.raises(ValueError, match="seeded=True session only"):
            plain.admit([0], toks, [6], [9], [1.0], [0.98], [1], masks, masks, seeds=[1])
        with pytest.raises(ValueError, match="not a seeded session"):
            plain.set_row_seeds([1, 2])
        for seeds, match in ((None, "no seeds"), ([1, 2], "2 seeds for 1"), ([True], "not an integer"), ([-1], "not an integer")):
            with pytest.raises(ValueError, match=match):
                ses.admit([0], toks, [6], [9], [1.0], [0.98], [1], masks, masks, seeds=seeds)
        with pytest.raises(ValueError, match="1 seeds for 2"):
            ses.set_row_seeds([1])
        with pytest.raises(ValueError, match="draws nothing from a generator"):
            ses.begin(g)
        assert not log
        # the stand-ins refuse what the entry points refuse, by name
        ev = torch.zeros(2, dtype=torch.int64)
        with pytest.raises(RuntimeError, match="seed is NULL"):
            emu_seeded.sample_noise_seeded(None, torch.zeros(2, dtype=torch.int32), 0)
        with pytest.raises(RuntimeError, match="ctr is NULL"):
            emu_seeded.sample_noise_seeded(ev, None, 0)


def test_standin_noise_is_the_reference(tok):
    """the stand-in's window: bits and q of sample_noise_seeded are ref_philox's, and the seeded stand-in is emu_rowparams' chain on
    that q"""
    seed = torch.tensor([0, -1, 77], dtype=torch.int64)
    ctr = torch.tensor([0, 5, 4095], dtype=torch.int32)
    bits, q = emu_seeded.sample_noise_seeded(seed, ctr, 2)
    rb, rq = ref_philox.noise([0, (1 << 64) - 1, 77], [0, 5, 4095], 2)
    assert (bits.numpy().view(np.uint32) == rb).all() and (q.numpy() == rq.astype(np.float32)).all()
    V, B = 200, 3
    gen = torch.Generator().manual_seed(0)
    logits = torch.randn((B, V), generator=gen)
    first = torch.zeros(V, dtype=torch.uint8)
    first[10:90] = 1
    tabs = torch.zeros((4, 8), dtype=torch.int32)
    kw = dict(first_span=(10, 90), max_range=0)
    temp, top_p, top_k = torch.tensor([1.0, 0.7, 1.3]), torch.tensor([0.98, 1.0, 0.5]), torch.tensor([20, 64, 3], dtype=torch.int32)
    ban = torch.zeros(V, dtype=torch.uint8)
    out_a, out_b = torch.zeros(B, dtype=torch.int64), torch.zeros(B, dtype=torch.int64)
    emu_seeded.sample_top_p_k_seeded(logits, first, tabs, tabs, torch.zeros(B, dtype=torch.int64), 0, seed, ctr, out_a, V, temp,
                                     top_p, top_k, ban, **kw)
    qq = torch.ones((B, V))
    qq[:, :64] = emu_seeded.sample_noise_seeded(seed, ctr, 0)[1]
    emu_rowparams.sample_top_p_k_rows(logits, first, tabs, tabs, torch.zeros(B, dtype=torch.int64), 0, qq, out_b, V, temp, top_p,
                                      top_k, ban, **kw)
    assert torch.equal(out_a, out_b) and ((out_a >= 10) & (out_a < 90)).all()
