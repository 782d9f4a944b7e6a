"""generate(share_prompt=True) on the MI355X: the shared-prompt decode session (one prompt cached once, per-row suffix caches, the
two-launch attention of shared.py inside the captured net graph) against the CPU oracle, in the patterns of test_decode_gpu.py:
bf16 tv2o-medium through ``DecodeSession`` with the oracle teacher-forced on the device's ids, fp32 ``generate`` id for id, the
accepted prompt forms, the serving form and the reuse of one pooled session for another prompt length."""
import os

import numpy as np
import pytest
import torch

import midi_model_amd as mm

from test_decode_gpu import DRIFT, _n_steps

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tok():
    return mm.MIDITokenizerV2()


@pytest.fixture(scope="module")
def medium(orc, tok):
    shp = orc.Shape(vocab=tok.vocab_size)
    sd = orc.make_state_dict(shp, seed=0)
    m = mm.MIDIModel(mm.MIDIModelConfig.from_name("tv2o-medium"))
    m.load_state_dict(sd, strict=True)
    return shp, sd, m


@pytest.fixture(scope="module")
def medium_bf16(medium):
    import copy
    shp, sd, m = medium
    return shp, sd, copy.deepcopy(m).to("cuda", torch.bfloat16).eval()


@pytest.fixture(scope="module")
def medium_fp32(medium):
    import copy
    shp, sd, m = medium
    return shp, sd, copy.deepcopy(m).to("cuda", torch.float32).eval()


PROMPT_SEED = 31    # generate() tests: the oracle alone checks 2151 / 2160 = 0.996 of the positions of its greedy continuation
SESSION_SEED = 32   # session test: the oracle alone has a safe margin on 37 / 48 (P 300) and 23 / 32 (P 1001); seed 31: 0.54, 0.44


@pytest.mark.parametrize("B,P,n_events,rows", [(4, 300, 8, None), (64, 1001, 4, (0, 9, 18, 27, 36, 45, 54, 63))],
                         ids=["b4_p300", "b64_p1001"])
def test_shared_decode_session_matches_oracle(orc, tok, medium_bf16, golden, B, P, n_events, rows):
    """test_production_decode_session_matches_oracle with a shared-prompt session: ONE prompt of P events (300: two chunks of the
    prefix kernel, the second ragged; 1001: four), B rows, the session built with shared_capacity, its graphs captured, and a
    suffix cache SMALLER than the prompt (256 rows).  After every replayed graph the hidden state / logits are within the
    reference's own bf16 drift (x1.5, medium_long_S2048.npz) of the oracle's cached fp32 forward on the same tokens, and the
    greedy id equals the oracle's masked arg-max wherever its top-2 margin exceeds twice that bound (more than 0.4 of the
    sampling positions: on the CPU the oracle's own greedy continuation of this prompt has 0.77 / 0.72 of them that safe)."""
    from midi_model_amd.decode import DecodeSession
    shp, sd, model = medium_bf16
    g = golden("medium_long_S2048.npz")
    hid_bound = DRIFT * float(g["ref_bf16_hidden_maxerr"])
    log_bound = DRIFT * float(g["ref_bf16_logits_maxerr"])
    V = tok.vocab_size
    scap = 512 if P <= 512 else 1024
    prompt = orc.synthetic_events(tok, 1, P, seed=SESSION_SEED).expand(B, -1, -1).contiguous()
    torch.set_num_threads(min(os.cpu_count() or 8, 32))
    with torch.inference_mode():
        ses = DecodeSession(model, B, 256, 1.0, 0.98, 1, shared_capacity=scap)
        assert ses.kv1.k.shape[-2] == 256 < P and ses.kvp.k.shape[1] == 1 and ses.kvp.k.shape[-2] == scap
        assert ses.g_net is not None and ses.g_steps is not None and ses.g_noise is not None, "captured graphs are the production form"
        assert ses.fold1 is not None and ses.lm_fold is not None and ses.fused_sampler, "folded norms + fused sampler"
        ses.first_mask.copy_(model._grammar()[0])
        ses.ban.zero_()
        ses.reset()
        ses.begin(torch.Generator(device="cuda").manual_seed(1))
        ses.prefill(prompt.cuda())
        assert int(ses.pre_len.item()) == P and ses.kvp.len == P and ses.kv1.len == 0
        R = torch.arange(B) if rows is None else torch.tensor(rows)  # the rows the oracle follows
        Bo = R.numel()
        cache1 = orc.KV()
        hid_o = orc.midi_forward(sd, shp, prompt[R], cache1)[:, -1]
        worst_h, worst_l, checked, total = 0.0, 0.0, 0, 0
        for ev_i in range(n_events):
            assert int(ses.pos.item()) == P + ev_i and int(ses.pre_len.item()) == P and ses.kv1.len == ev_i
            err = (ses.hidden.float().cpu()[R] - hid_o).abs().max().item()
            worst_h = max(worst_h, err)
            assert err <= hid_bound, (ev_i, err, hid_bound)
            cache2 = orc.KV()
            names, end = [""] * Bo, [False] * Bo
            n_steps, i, prev = tok.max_token_seq, 0, None
            while i < n_steps:
                ses.tok_step(i)
                lg = ses.logits[:, :V].float().cpu()[R]
                ids_all = ses.seq[:, i].cpu()
                ids = ids_all[R]
                lo = orc.midi_forward_token(sd, shp, hid_o if i == 0 else None, None if i == 0 else prev[:, None], cache2)[:, -1]
                e = (lg - lo).abs().max().item()
                worst_l = max(worst_l, e)
                assert e <= log_bound, (ev_i, i, e, log_bound)
                mask = orc.grammar_mask(tok, i, names, end).bool()
                legal = lo.masked_fill(~mask, float("-inf"))
                top2 = legal.topk(2, -1)
                margin = top2.values[:, 0] - top2.values[:, 1]
                assert mask.gather(1, ids[:, None]).all(), "the device sampled an id outside the grammar mask"
                safe = margin > 2 * log_bound
                total += Bo
                checked += int(safe.sum())
                assert (ids[safe] == top2.indices[:, 0][safe]).all(), (ev_i, i, ids.tolist(), top2.indices[:, 0].tolist())
                if i == 0:
                    names = [tok.id_events.get(int(t), "") for t in ids]
                    end = [int(t) == tok.eos_id for t in ids]
                    n_steps = _n_steps(tok, ids_all.tolist())
                prev = ids
                i += 1
            ses.consumed(n_steps)
            event = ses.seq.cpu().clone()[R]
            ses.net_step()
            hid_o = orc.midi_forward(sd, shp, event[:, None, :], cache1)[:, -1]
        ses.end()
    print(f"shared session vs oracle (B {B}, P {P}): worst hidden err {worst_h:.4f} (bound {hid_bound:.4f}), worst logits err "
          f"{worst_l:.4f} (bound {log_bound:.4f}); greedy ids checked on {checked}/{total} rows with a safe margin")
    assert checked > 0.4 * total


def _oracle_argmax_check(orc, tok, sd, shp, out, first, margin_min=1e-3):
    """teacher-forced oracle (one uncached pass) over ``out`` (B, L, 8): at every sampling position of events >= ``first`` the
    device's id must be the oracle's grammar-masked arg-max wherever its top-2 margin exceeds margin_min; -> (checked, total)"""
    ids = torch.from_numpy(out)
    B, L, T = ids.shape
    torch.set_num_threads(min(os.cpu_count() or 8, 32))
    with torch.inference_mode():
        hidden = orc.midi_forward(sd, shp, ids[:, :-1])[:, first - 1:]            # hidden i predicts event i + 1
        n = hidden.shape[1]
        tgt = ids[:, first:].reshape(B * n, T)
        logits = orc.midi_forward_token(sd, shp, hidden.reshape(B * n, -1), tgt[:, :-1])
    N = tgt.shape[0]
    names = [tok.id_events[int(t)] for t in tgt[:, 0]]
    bad, checked = [], 0
    for i in range(T):
        mask = orc.grammar_mask(tok, i, names if i else [""] * N, [False] * N, ban_eos=True).bool()
        assert mask.gather(1, tgt[:, i:i + 1]).all(), f"position {i}: an id outside the grammar mask"
        legal = logits[:, i].masked_fill(~mask, float("-inf"))
        top2 = legal.topk(2, -1)
        safe = (top2.values[:, 0] - top2.values[:, 1]) > margin_min
        checked += int(safe.sum())
        wrong = (tgt[:, i] != top2.indices[:, 0]) & safe
        bad += [(int(k), i) for k in wrong.nonzero().flatten()]
    assert not bad, f"device ids differ from the oracle's arg-max at (row*event, position): {bad[:8]}"
    return checked, N * T


def test_generate_share_prompt_fp32_follows_the_oracle_id_for_id(orc, tok, medium_fp32):
    """generate(share_prompt=True) itself: fp32 tv2o-medium, greedy, a 2-D synthetic prompt of 130 events, B = 3, max_len 400 --
    270 generated events, so the suffix cache is the 512-row one (the suffix passes 255) behind a 256-row prompt cache.  Teacher-
    forced oracle as in test_greedy_generate_600_events...: margin 1e-3, checked share > 0.97 (the oracle's own greedy
    continuation of this prompt: 0.996 on the CPU).  The pooled session is the shared one, and a seeded generator is left where
    the plain path leaves it."""
    shp, sd, m = medium_fp32
    P, B, L = 130, 3, 400
    prompt = orc.synthetic_events(tok, 1, P, seed=PROMPT_SEED)[0].numpy()
    gen = torch.Generator(device="cuda").manual_seed(3)
    out = m.generate(prompt, batch_size=B, max_len=L, top_k=1, ban_eos=True, generator=gen, share_prompt=True)
    assert out.shape == (B, L, 8) and out.dtype == np.int64 and (out[:, :P] == prompt[None]).all()
    ses = m._sessions.idle[-1]
    assert ses.shared_capacity >= P and ses.shared_capacity == 256 and ses.kvp.k.shape[1] == 1 and ses.cap == 512
    assert int(ses.pre_len.item()) == P and int(ses.pos.item()) == L - 1 and ses.kv1.len == L - 1 - P
    checked, total = _oracle_argmax_check(orc, tok, sd, shp, out, P)
    assert checked > 0.97 * total, (checked, total)
    gen0 = torch.Generator(device="cuda").manual_seed(3)
    ref = m.generate(prompt, batch_size=B, max_len=L, top_k=1, ban_eos=True, generator=gen0)
    assert torch.equal(gen.get_state(), gen0.get_state()), "the seeded generator ends elsewhere than on the plain path"
    print(f"generate(share_prompt=True), {L - P} events x {B} behind {P}: {checked}/{total} sampling positions checked against the "
          f"oracle's arg-max, all equal; ids equal to the plain path's at {(out == ref).mean():.4f} of the positions")


def test_prompt_forms_and_stream(orc, tok, medium_fp32):
    """2-D, (1, L, 8) and (B, L, 8) equal-rows prompts give identical output; unequal rows raise ValueError before any launch;
    prompt=None with share_prompt=True is the plain call bit for bit; generate_stream(share_prompt=True) yields generate's events
    and the mask options hold on every yielded event"""
    shp, sd, m = medium_fp32
    P, B, L = 130, 3, 140
    p = orc.synthetic_events(tok, 1, P, seed=PROMPT_SEED)[0].numpy()
    kw = dict(batch_size=B, max_len=L, top_k=1, ban_eos=True, share_prompt=True)
    a = m.generate(p, **kw)
    assert (m.generate(p[None], **kw) == a).all() and (m.generate(np.stack([p] * B), **kw) == a).all()
    bad = np.stack([p] * B)
    bad[1, 77, 2] += 1
    n_calls = []
    from midi_model_amd.lib import lib
    lib().profile = n_calls  # (every C-ABI call is recorded while this is a list)
    try:
        with pytest.raises(ValueError, match="row 1 differs"):
            m.generate(bad, **kw)
        assert not n_calls, "unequal rows were refused after a launch"
    finally:
        lib().profile = None
    g0, g1 = torch.Generator(device="cuda").manual_seed(5), torch.Generator(device="cuda").manual_seed(5)
    x = m.generate(None, batch_size=B, max_len=12, generator=g0, share_prompt=True)
    y = m.generate(None, batch_size=B, max_len=12, generator=g1)
    assert (x == y).all() and torch.equal(g0.get_state(), g1.get_state())
    opts = dict(disable_patch_change=True, disable_control_change=True, disable_channels=[0, 9])
    g2, g3 = torch.Generator(device="cuda").manual_seed(6), torch.Generator(device="cuda").manual_seed(6)
    evs = list(m.generate_stream(p, batch_size=B, max_len=L, generator=g2, share_prompt=True, **opts))
    ref = m.generate(p, batch_size=B, max_len=L, generator=g3, share_prompt=True, **opts)
    assert all(e.shape == (B, 8) and e.dtype == np.int64 for e in evs)
    assert (np.stack(evs, 1) == ref[:, P:]).all()
    banned = [tok.parameter_ids["channel"][c] for c in (0, 9)]
    for e in evs:
        assert not np.isin(e[:, 0], [tok.event_ids["patch_change"], tok.event_ids["control_change"]]).any()
        assert not np.isin(e, banned).any()


def test_one_pooled_session_serves_another_prompt_length(orc, tok, medium_fp32):
    """prompts of 130 and then 47 events through ONE pooled shared session (same capacities: 256-row prompt cache, 512-row suffix
    cache), no recapture: the captured net graph reads pos / pre_len from device memory and its launch geometry depends on the
    capacities only.  The second call's first 4 events follow the oracle."""
    shp, sd, m = medium_fp32
    B = 3
    m._sessions.idle.clear()
    p1 = orc.synthetic_events(tok, 1, 130, seed=PROMPT_SEED)[0].numpy()
    m.generate(p1, batch_size=B, max_len=130 + 258, top_k=1, ban_eos=True, share_prompt=True)
    assert len(m._sessions.idle) == 1
    ses = m._sessions.idle[0]
    g_net, g_steps, key = ses.g_net, ses.g_steps, ses.key
    assert (ses.cap, ses.shared_capacity) == (512, 256)
    p2 = orc.synthetic_events(tok, 1, 47, seed=PROMPT_SEED + 1)[0].numpy()
    out = m.generate(p2, batch_size=B, max_len=47 + 258, top_k=1, ban_eos=True, share_prompt=True)
    assert len(m._sessions.idle) == 1 and m._sessions.idle[0] is ses and ses.key == key
    assert ses.g_net is g_net and ses.g_steps is g_steps, "the session was recaptured"
    assert int(ses.pre_len.item()) == 47 and ses.kvp.len == 47
    checked, total = _oracle_argmax_check(orc, tok, sd, shp, out[:, :47 + 4], 47)
    assert checked > 0, (checked, total)
