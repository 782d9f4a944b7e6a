"""generate_ragged with a value per row, on the CPU: the row_params session's bookkeeping (decode.py), the per-row arguments of
model.generate_ragged / generate_stream_ragged and their refusals, through the ragged fake backend plus the stand-in of
mh_sample_top_p_k_rows (tests/emu_rowparams.py).  Tiny 4-layer model, fp32.  The kernel itself: test_rowparams_kernels_gpu.py; the
production session: test_rowparams_gpu.py."""
import numpy as np
import pytest
import torch

import midi_model_amd as mm

import emu_rowparams
import ragged_common as rc

LENGTHS = (1, 5, 17, 20)


def tiny_config():
    return mm.MIDIModelConfig.get_config("v2", True, 4, 4, 256, 512)


@pytest.fixture(scope="module")
def tok():
    return mm.MIDITokenizerV2()


@pytest.fixture(scope="module")
def tiny(orc, tok):
    shp = orc.Shape(n_layer=4, n_head=4, n_embd=256, n_inner=512, vocab=tok.vocab_size)
    return shp, orc.make_state_dict(shp, seed=0)


def _model(sd, dtype=torch.float32):
    m = mm.MIDIModel(tiny_config())
    m.load_state_dict(sd)
    return m.to(dtype)


def test_equal_entries_return_the_scalar_calls_ids(orc, tok, tiny):
    """lists of equal entries run the row_params session and the rows sampler; for the same seeded generator they return the ids
    of the scalar call (the uniform sampler), and both generators end in the same state"""
    ps = rc.prompts(orc, tok, LENGTHS)
    with emu_rowparams.install() as log:
        m = _model(tiny[1])
        g0, g1 = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
        ref = m.generate_ragged(ps, max_len=30, temp=0.9, top_p=0.95, top_k=12, generator=g0)
        assert "sample_top_p_k" in log and "sample_top_p_k_rows" not in log
        del log[:]
        got = m.generate_ragged(ps, max_len=[30] * 4, temp=[0.9] * 4, top_p=[0.95] * 4, top_k=[12] * 4, generator=g1)
        assert "sample_top_p_k_rows" in log and "sample_top_p_k" not in log
    assert len(got) == 4 and all(a.shape == b.shape and (a == b).all() for a, b in zip(got, ref))
    assert torch.equal(g0.get_state(), g1.get_state())
    assert [s.row_params for s in m._sessions.idle] == [False, True]
    # one per-row argument is enough to take the row_params path
    with emu_rowparams.install() as log:
        del log[:]
        g2 = torch.Generator().manual_seed(5)
        one = m.generate_ragged(ps, max_len=30, temp=0.9, top_p=0.95, top_k=np.array([12] * 4), generator=g2)
        assert "sample_top_p_k_rows" in log and "sample_top_p_k" not in log
    assert all((a == b).all() for a, b in zip(one, ref)) and torch.equal(g0.get_state(), g2.get_state())


def test_greedy_rows_inside_a_mixed_batch(orc, tok, tiny):
    """rows with top_k = 1 are greedy whatever their temperature and top-p: inside a batch whose other rows sample at top_k 20 / 64
    and temperatures 0.5 / 1.7 they equal the same rows of an all-greedy call, id for id (rows are independent; EOS banned, so
    every row runs to max_len in both calls)"""
    ps = rc.prompts(orc, tok, LENGTHS)
    with emu_rowparams.install():
        m = _model(tiny[1])
        mixed = m.generate_ragged(ps, max_len=30, temp=[1.7, 0.5, 0.5, 1.7], top_p=[0.3, 0.9, 0.98, 1.0], top_k=[1, 20, 1, 64],
                                  ban_eos=True, generator=torch.Generator().manual_seed(3))
        greedy = m.generate_ragged(ps, max_len=30, top_k=[1] * 4, ban_eos=True, generator=torch.Generator().manual_seed(4))
    assert [len(r) for r in mixed] == [30] * 4
    for b in (0, 2):
        assert (mixed[b] == greedy[b]).all(), b
    for b in (1, 3):  # (the sampled rows did sample: 13 / 10 events x up to 8 tokens all equal to the arg-max would be no draw at all)
        assert (mixed[b] != greedy[b]).any(), b


def test_per_row_max_len(orc, tok, tiny):
    """EOS banned: row b comes back with exactly max_len[b] events, retires at its own step, and the call ends when the longest
    row does; the session's rows end parked at their own limits"""
    ps = rc.prompts(orc, tok, LENGTHS)
    max_len = [12, 9, 30, 24]
    lengths = np.array(LENGTHS)
    with emu_rowparams.install():
        m = _model(tiny[1])
        out = m.generate_ragged(ps, max_len=max_len, top_k=1, ban_eos=True)
        assert [len(r) for r in out] == max_len and all((r[:len(p)] == p).all() for r, p in zip(out, ps))
        ses = m._sessions.idle[0]
        assert ses.row_params and ses.cap == 256 and ses.pos_limit.tolist() == max_len
        # 13 event steps (row 2: 17 + 13 = 30), a net step after each but the last
        assert ses.pos.tolist() == [12, 9, 29, 24]
        steps, rows = 0, [[] for _ in ps]
        for ev, live in m.generate_stream_ragged(ps, max_len=max_len, top_k=1, ban_eos=True):
            assert (live == (lengths + steps < np.array(max_len))).all(), steps
            for b in np.flatnonzero(live):
                rows[b].append(ev[b])
            steps += 1
        assert steps == 13
        assert all((np.stack(r) == o[len(p):]).all() for r, o, p in zip(rows, out, ps))


def test_per_row_masks_and_parameters_follow_the_oracle_chain(orc, tok, tiny):
    """The session driven step by step (test_fused_sampler_inside_graphs_equals_oracle_chain_on_same_noise, per row): rows carry
    ban_eos / disable_patch_change / disable_channels=[9] / nothing and parameters of their own; at every draw row b's id is
    orc.sample_top_p_k's on that row's logits at temp[b], the session's variates and row b's own grammar mask, with top_p[b] and
    top_k[b].  Only an exact probability tie may order two ids differently."""
    from midi_model_amd.decode import DecodeSession
    ps = rc.prompts(orc, tok, LENGTHS)
    B, V = 4, tok.vocab_size
    temp, top_p, top_k = [1.0, 0.8, 1.3, 1.0], [0.98, 0.9, 0.98, 0.95], [20, 10, 64, 5]
    opts = [dict(ban_eos=True), dict(disable_patch_change=True), dict(disable_channels=[9]), dict()]
    with emu_rowparams.install(), torch.inference_mode():
        m = _model(tiny[1])
        rp = m._row_params(ps, 40, temp, top_p, top_k, [True, False, False, False], [False, True, False, False], False,
                           [None, None, [9], None])
        assert rp["chans"] == [[], [], [9], []]
        ses = DecodeSession(m, B, 64, 1.0, 0.98, 1, ragged=True, row_params=True)
        assert ses.fused_sampler and ses.first_mask.shape == (B, V) and ses.ban.shape == (B, V) and ses.pos_limit.shape == (B,)
        m._set_masks_rows(ses, rp)
        ses.set_row_params(temp, top_p, top_k)
        assert int(ses.first_mask[0, tok.eos_id]) == 0 and int(ses.first_mask[1, tok.eos_id]) == 1
        assert ses.ban.sum(1).tolist() == [0, 0, 1, 0] and int(ses.ban[2, tok.parameter_ids["channel"][9]]) == 1
        ses.reset()
        ses.begin(torch.Generator().manual_seed(7))
        ses.set_limit(rp["max_len"])
        ses.prefill_ragged(torch.from_numpy(np.concatenate(ps)), list(LENGTHS))
        n = 0
        for ev_i in range(6):
            names, end = [""] * B, [False] * B
            n_steps, i = tok.max_token_seq, 0
            ses.draw_noise()
            while i < n_steps:
                ses.tok_step(i)
                lg, q, ids = ses.logits[:, :V].float(), ses.q_all[i], ses.seq[:, i].clone()
                for b in range(B):
                    mask = orc.grammar_mask(tok, i, names[b:b + 1], end[b:b + 1], **opts[b])
                    scores = torch.softmax(lg[b:b + 1] / temp[b], dim=-1) * mask
                    want = int(orc.sample_top_p_k(scores[:, None], top_p[b], top_k[b], noise=q[b:b + 1, None])[0, 0])
                    if want != int(ids[b]):  # only an exact probability tie may order two ids differently
                        assert scores[0, want] == scores[0, ids[b]], (ev_i, i, b, want, int(ids[b]))
                    else:
                        n += 1
                if i == 0:
                    names = [tok.id_events.get(int(t), "") for t in ids]
                    end = [int(t) == tok.eos_id for t in ids]
                    n_steps = rc.n_steps(tok, ids.tolist())
                    assert ses.n_steps_of(ids.tolist())[0] == n_steps
                    assert not end[0] and names[1] != "patch_change"
                i += 1
            ses.consumed(n_steps)
            ses.net_step()
        ses.end()
    assert n > 100


def test_refusals_come_before_any_backend_call(orc, tok, tiny):
    with emu_rowparams.install() as log:
        m = _model(tiny[1])
        del log[:]
        p = rc.prompts(orc, tok, (3, 6), seed0=80)
        nan, inf = float("nan"), float("inf")
        for fn in (m.generate_ragged, m.generate_stream_ragged):
            for kw, match in (
                    (dict(temp=[1.0]), "temp holds 1 values for 2"),
                    (dict(top_k=[20, 20, 20]), "top_k holds 3 values for 2"),
                    (dict(max_len=[9]), "max_len holds 1 values for 2"),
                    (dict(ban_eos=[True]), "ban_eos holds 1 values for 2"),
                    (dict(disable_channels=[None]), "disable_channels holds 1 entries for 2"),
                    (dict(temp=[1.0, 0.0]), "row 1: temperature"),
                    (dict(temp=[-1.0, 1.0]), "row 0: temperature"),
                    (dict(temp=[1.0, inf]), "row 1: temperature"),
                    (dict(temp=[nan, 1.0]), "row 0: temperature"),
                    (dict(top_p=[0.9, nan]), "row 1: top_p"),
                    (dict(top_k=[0, 20]), "row 0: top_k"),
                    (dict(top_k=[20, 65]), "row 1: top_k"),
                    (dict(temp=[1.0, 1.0], top_k=65), "row 0: top_k"),   # (no op-by-op fallback on the per-row path)
                    (dict(max_len=[9, 6]), "prompt 1 has 6 events, max_len is 6"),
                    (dict(max_len=[3, 9]), "prompt 0 has 3 events, max_len is 3"),
                    (dict(disable_channels=[None, [16]]), "row 1: .*disable_channels"),
                    (dict(disable_channels=[list(range(16)), None]), "row 0: .*every channel"),
            ):
                with pytest.raises(ValueError, match=match):
                    fn(p, **kw)
                assert not log and not m._sessions.idle, (fn.__name__, match, log[:3])
        from midi_model_amd.decode import DecodeSession
        with pytest.raises(ValueError, match="row_params"):
            DecodeSession.make_key(m, 2, 256, 1.0, 0.98, 1, 256, False, True)
        with pytest.raises(ValueError):
            DecodeSession(m, 2, 256, 1.0, 0.98, 1, shared_capacity=256, ragged=True, row_params=True)
        with pytest.raises(ValueError, match="row_params"):
            DecodeSession(m, 2, 256, 1.0, 0.98, 1, row_params=True)
        with pytest.raises(ValueError, match="fused sampler"):
            DecodeSession(m, 2, 256, 1.0, 0.98, 65, ragged=True, row_params=True)
        assert not log


def test_one_pooled_session_serves_every_setting(orc, tok, tiny):
    from midi_model_amd.decode import DecodeSession
    with emu_rowparams.install():
        m = _model(tiny[1])
        ptr, dt = m._flat.data_ptr(), m._flat.dtype
        # the keys of the forms that existed before row_params are what they were
        plain = (ptr, dt, 3, 256, 1.0, 0.98, 20)
        assert DecodeSession.make_key(m, 3, 256, 1.0, 0.98, 20) == plain
        assert DecodeSession.make_key(m, 3, 256, 1.0, 0.98, 20, 512) == plain + (("shared", 512),)
        assert DecodeSession.make_key(m, 3, 256, 1.0, 0.98, 20, 0, True) == plain + (("ragged",),)
        rows_key = DecodeSession.make_key(m, 3, 256, 0.7, 0.5, 3, 0, True, True)
        assert rows_key == (ptr, dt, 3, 256, ("ragged", "row_params"))
        ps = rc.prompts(orc, tok, (2, 9, 4), seed0=50)
        a = m.generate_ragged(ps, max_len=12, temp=[0.5, 1.0, 1.7], top_k=[20, 1, 64], ban_eos=True)
        assert len(m._sessions.idle) == 1
        ses = m._sessions.idle[0]
        assert ses.row_params and ses.ragged and ses.key == rows_key
        assert ses.temp_rows.tolist() == [0.5, 1.0, pytest.approx(1.7)] and ses.top_k_rows.tolist() == [20, 1, 64]
        ptrs = [t.data_ptr() for t in (ses.temp_rows, ses.top_p_rows, ses.top_k_rows, ses.first_mask, ses.ban, ses.pos_limit)]
        b = m.generate_ragged(ps, max_len=[12, 11, 10], temp=[1.3, 0.6, 1.0], top_p=[0.9, 0.5, 1.0], top_k=5,
                              disable_channels=[[9], None, [0, 1]])
        assert len(m._sessions.idle) == 1 and m._sessions.idle[0] is ses and ses.key == rows_key
        assert ptrs == [t.data_ptr() for t in (ses.temp_rows, ses.top_p_rows, ses.top_k_rows, ses.first_mask, ses.ban, ses.pos_limit)]
        assert ses.top_k_rows.tolist() == [5, 5, 5] and ses.pos_limit.tolist() == [12, 11, 10] and ses.ban.sum(1).tolist() == [1, 0, 2]
        assert [len(r) for r in a] == [12] * 3 and all(len(r) <= n for r, n in zip(b, (12, 11, 10)))
        # a scalar call of the same B does not take it, and keeps the key it always had
        m.generate_ragged(ps, max_len=12, top_k=1, ban_eos=True)
        assert len(m._sessions.idle) == 2 and m._sessions.idle[1].key == (ptr, dt, 3, 256, 1.0, 0.98, 1, ("ragged",))
        # the session refuses what it has no buffers or rows for
        with pytest.raises(ValueError, match="capacity"):
            ses.set_limit([12, 256, 10])
        with pytest.raises(ValueError, match="limits"):
            ses.set_limit([12, 10])
        with pytest.raises(ValueError, match="limits"):
            m._sessions.idle[1].set_limit([12, 10, 10])
        with pytest.raises(ValueError, match="values for a session"):
            ses.set_row_params([1.0], [0.9], [20])
        with pytest.raises(ValueError, match="top_k"):
            ses.set_row_params([1.0] * 3, [0.9] * 3, [20, 0, 20])
        with pytest.raises(ValueError, match="row_params"):
            m._sessions.idle[1].set_row_params([1.0] * 3, [0.9] * 3, [20] * 3)
