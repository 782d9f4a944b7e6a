"""generate_ragged with a value per row on the MI355X (tv2o-medium, bf16): the production row_params session -- captured graphs,
folded norms, mh_sample_top_p_k_rows inside the steps graph -- against the oracle's sampling chain on the session's own noise, the
public call against the scalar call (the rows kernel end to end against the uniform kernel), greedy rows inside a mixed batch,
one pooled session for every setting without a recapture, and per-row max_len."""
import copy

import numpy as np
import pytest
import torch

import midi_model_amd as mm

import ragged_common as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tok():
    return mm.MIDITokenizerV2()


@pytest.fixture(scope="module")
def medium_bf16(orc, tok):
    shp = orc.Shape(vocab=tok.vocab_size)
    sd = orc.make_state_dict(shp, seed=0)
    m = mm.MIDIModel(mm.MIDIModelConfig.from_name("tv2o-medium"))
    m.load_state_dict(sd, strict=True)
    return shp, sd, copy.deepcopy(m).to("cuda", torch.bfloat16).eval()


def test_row_params_session_equals_oracle_chain_on_same_noise(orc, tok, medium_bf16):
    """B = 4, prompts of (1, 5, 127, 300) events, graphs captured, folded norms; rows carry ban_eos / disable_patch_change /
    disable_channels=[9] / nothing and temperature, top-p, top-k of their own.  4 events step by step: after every token step, row
    b's id is orc.sample_top_p_k's on the logits the step produced (divided by temp[b] in bf16, as the reference divides), the
    Exp(1) variates the noise graph drew and row b's own grammar mask.  Only an exact probability tie may order two ids
    differently; more than 100 draws are compared."""
    from midi_model_amd.decode import DecodeSession
    shp, sd, model = medium_bf16
    lengths = (1, 5, 127, 300)
    B, V = 4, tok.vocab_size
    temp, top_p, top_k = [1.0, 0.8, 1.3, 1.0], [0.98, 0.9, 0.98, 0.95], [20, 10, 64, 5]
    opts = [dict(ban_eos=True), dict(disable_patch_change=True), dict(disable_channels=[9]), dict()]
    ps = rc.prompts(orc, tok, lengths)
    with torch.inference_mode():
        rp = model._row_params(ps, 400, temp, top_p, top_k, [True, False, False, False], [False, True, False, False], False,
                               [None, None, [9], None])
        ses = DecodeSession(model, B, 512, 1.0, 0.98, 1, ragged=True, row_params=True)
        assert ses.row_params and ses.g_net is not None and ses.g_steps is not None and ses.g_noise is not None, "captured graphs"
        assert ses.fold1 is not None and ses.lm_fold is not None and ses.fused_sampler, "folded norms + fused sampler"
        model._set_masks_rows(ses, rp)
        ses.set_row_params(temp, top_p, top_k)
        ses.reset()
        ses.begin(torch.Generator(device="cuda").manual_seed(7))
        ses.set_limit(rp["max_len"])
        ses.prefill_ragged(torch.from_numpy(np.concatenate(ps)).cuda(), list(lengths))
        n = 0
        for ev_i in range(4):
            assert ses.pos.tolist() == [L + ev_i for L in lengths] and ses.pos_limit.tolist() == [400] * 4
            names, end = [""] * B, [False] * B
            n_steps, i = tok.max_token_seq, 0
            ses.draw_noise()
            while i < n_steps:
                ses.tok_step(i)
                lg, q, ids = ses.logits[:, :V].cpu(), ses.q_all[i].cpu(), ses.seq[:, i].cpu()
                for b in range(B):
                    mask = orc.grammar_mask(tok, i, names[b:b + 1], end[b:b + 1], **opts[b])
                    scores = torch.softmax((lg[b:b + 1] / temp[b]).float(), dim=-1) * mask
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
    print(f"row_params session: {n} draws equal to the oracle chain")
    assert n > 100


def test_equal_entries_return_the_scalar_calls_rows(orc, tok, medium_bf16):
    """lists of equal entries run mh_sample_top_p_k_rows inside the captured steps, scalars run mh_sample_top_p_k: for the same
    seed the rows are identical and the generators end in the same state"""
    shp, sd, m = medium_bf16
    m._sessions.idle.clear()
    ps = rc.prompts(orc, tok, (3, 40, 17, 130), seed0=51)
    g0, g1 = torch.Generator(device="cuda").manual_seed(9), torch.Generator(device="cuda").manual_seed(9)
    ref = m.generate_ragged(ps, max_len=150, temp=0.9, top_p=0.95, top_k=20, generator=g0)
    got = m.generate_ragged(ps, max_len=[150] * 4, temp=[0.9] * 4, top_p=[0.95] * 4, top_k=[20] * 4, generator=g1)
    assert [s.row_params for s in m._sessions.idle] == [False, True]
    assert all(x.shape == y.shape and (x == y).all() for x, y in zip(got, ref)) and torch.equal(g0.get_state(), g1.get_state())
    assert all(len(p) < len(r) <= 150 for p, r in zip(ps, ref))


def test_greedy_rows_inside_a_mixed_batch(orc, tok, medium_bf16):
    """rows 0 and 2 at top_k = 1 beside rows sampling at top_k 20 / 64 and temperatures 0.5 / 1.7: id for id the rows of the
    all-greedy batch (EOS banned: every row runs to max_len in both calls)"""
    shp, sd, m = medium_bf16
    ps = rc.prompts(orc, tok, (3, 40, 17, 130), seed0=51)
    mixed = m.generate_ragged(ps, max_len=150, temp=[1.7, 0.5, 0.5, 1.7], top_p=[0.3, 0.9, 0.98, 1.0], top_k=[1, 20, 1, 64],
                              ban_eos=True, generator=torch.Generator(device="cuda").manual_seed(3))
    greedy = m.generate_ragged(ps, max_len=150, top_k=[1] * 4, ban_eos=True, generator=torch.Generator(device="cuda").manual_seed(4))
    assert [len(r) for r in mixed] == [150] * 4 and [len(r) for r in greedy] == [150] * 4
    for b in (0, 2):
        assert (mixed[b] == greedy[b]).all(), b
    for b in (1, 3):
        assert (mixed[b] != greedy[b]).any(), b


def test_one_session_serves_every_setting_without_recapture(orc, tok, medium_bf16):
    shp, sd, m = medium_bf16
    m._sessions.idle.clear()
    ps = rc.prompts(orc, tok, (3, 40, 17, 130), seed0=51)
    a = m.generate_ragged(ps, max_len=140, temp=[0.5, 1.0, 1.7, 1.0], generator=torch.Generator(device="cuda").manual_seed(1))
    assert len(m._sessions.idle) == 1
    ses = m._sessions.idle[0]
    g_net, g_steps, g_noise, key = ses.g_net, ses.g_steps, ses.g_noise, ses.key
    assert ses.row_params and g_net is not None and g_steps is not None
    b = m.generate_ragged(ps, max_len=140, temp=[1.3, 0.6, 0.9, 2.0], top_k=[5, 64, 20, 1], disable_channels=[[9], None, None, [0]],
                          generator=torch.Generator(device="cuda").manual_seed(1))
    assert len(m._sessions.idle) == 1 and m._sessions.idle[0] is ses and ses.key == key
    assert ses.g_net is g_net and ses.g_steps is g_steps and ses.g_noise is g_noise, "the session was recaptured"
    assert ses.top_k_rows.tolist() == [5, 64, 20, 1] and ses.ban.sum(1).tolist() == [1, 0, 0, 1]
    assert any(x.shape != y.shape or (x != y).any() for x, y in zip(a, b)), "the second setting changed nothing"
    for rows in (a, b):
        assert all(len(p) < len(r) <= 140 and (r[:len(p)] == p).all() for p, r in zip(ps, rows))


def test_per_row_max_len(orc, tok, medium_bf16):
    """max_len (100, 60, 100, 80) over prompts of (3, 40, 17, 30) events, EOS banned: row b returns max_len[b] events.  97 event
    steps (row 0), a net step after each but the last: rows 1, 2, 3 end parked at their own limits, row 0 -- the row the call
    waited for -- stands one short of its, as the longest row of every generate_ragged call does."""
    shp, sd, m = medium_bf16
    ps = rc.prompts(orc, tok, (3, 40, 17, 30), seed0=71)
    max_len = [100, 60, 100, 80]
    out = m.generate_ragged(ps, max_len=max_len, top_k=[20] * 4, ban_eos=True, generator=torch.Generator(device="cuda").manual_seed(2))
    assert [len(r) for r in out] == max_len and all((r[:len(p)] == p).all() for r, p in zip(out, ps))
    ses = m._sessions.idle[-1]
    assert ses.row_params and ses.pos_limit.tolist() == max_len
    assert ses.pos.tolist() == [99, 60, 100, 80]
