"""The 8-bit K/V cache end to end on the MI355X, production session: bf16 tv2o-medium with random weights, captured graphs, folded
norms, fused sampler, DecodeSession / DecodePool with kv_dtype="fp8".

  prefill    one admission into an fp8 session and into a bf16 session: every layer's fp8 rows are quantize() of the bf16 rows, hidden is
             bit-equal (the prefill never reads the cache: no tolerance);
  seeded     a request's ids alone and beside neighbours; a child on its parent's seed; held-then-forked against uninterrupted
             (tests/kvq_common.py, the scenarios of fork_common.py) -- no tolerance; the session and its graph objects stay the same;
  accuracy   teacher-forced against the oracle, gated by the reference's own statement of what fp8 K/V does (d_q)."""
import os

import pytest
import torch

import midi_model_amd as mm

import fork_common as fc
import kvq_common as kc
import ragged_common as rc
import ref_kvq

pytestmark = pytest.mark.gpu

CAP = 256
DRIFT = 1.5


@pytest.fixture(scope="module")
def tok():
    return mm.MIDITokenizerV2()


@pytest.fixture(scope="module")
def medium_bf16(orc, tok):
    shp = orc.Shape(vocab=tok.vocab_size)
    sd = orc.make_state_dict(shp, seed=0)
    m = mm.MIDIModel(mm.MIDIModelConfig.from_name("tv2o-medium"))
    m.load_state_dict(sd, strict=True)
    return shp, sd, m.to("cuda", torch.bfloat16).eval()


def _admit(ses, model, rows, prompts, limit=CAP - 1, top_k=1):
    n, V = len(prompts), ses.V
    first = model._grammar()[0].cpu()[None].repeat(n, 1).contiguous()
    ses.admit(rows, torch.cat([torch.as_tensor(p) for p in prompts]), [len(p) for p in prompts], [limit] * n, [1.0] * n, [0.98] * n,
              [top_k] * n, first, torch.zeros((n, V), dtype=torch.uint8))


def test_prefill_quantizes_what_the_bf16_session_stores(orc, tok, medium_bf16):
    from midi_model_amd.decode import DecodeSession
    _, _, model = medium_bf16
    prompts = rc.prompts(orc, tok, (9, 33, 5), seed0=700)
    rows = [2, 0, 3]
    with torch.inference_mode():
        out = []
        for kw in ({}, dict(kv_dtype="fp8")):
            ses = DecodeSession(model, 4, CAP, 1.0, 0.98, 1, ragged=True, row_params=True, **kw)
            ses.reset()
            _admit(ses, model, rows, prompts)
            torch.cuda.synchronize()
            out.append(ses)
        plain, q = out
        assert torch.equal(plain.hidden.view(torch.int16), q.hidden.view(torch.int16)) and plain.pos.tolist() == q.pos.tolist() == [33, 0, 9, 5]
        for r, p in zip(rows, prompts):
            L = len(p)
            for name8, name, j in (("k8", "k", 0), ("v8", "v", 1)):
                codes, s = ref_kvq.quantize(getattr(plain.kv1, name)[:, r, :, :L].cpu())
                assert torch.equal(getattr(q.kv1, name8)[:, r, :, :L].cpu(), codes), (r, name)
                assert torch.equal(q.kv1.sc[:, r, :, :L, j].cpu().view(torch.int32), s.view(torch.int32)), (r, name)
        assert q.kv1.nbytes() * 256 == (plain.kv1.k.numel() + plain.kv1.v.numel()) * 2 * 136, "136 bytes where bf16 holds 256"


@pytest.fixture(scope="module")
def seeded_session(orc, tok, medium_bf16):
    """the pooled seeded fp8 session of 4 rows and its graphs, made by one request that runs two events"""
    m = medium_bf16[2]
    m._sessions.idle.clear()
    with m.decode_pool(fc.ROWS, CAP, seeded=True, kv_dtype="fp8") as pool:
        pool.submit(rc.prompts(orc, tok, (5,), seed0=590)[0], max_len=7, seed=1)
        fc.drain(pool)
        ses = pool.ses
    assert ses.use_graphs and ses.g_net is not None and ses.g_steps is not None, "captured graphs are the production form"
    assert ses.seeded and ses.row_params and ses.fold1 is not None and ses.fused_sampler and ses.B == fc.ROWS and ses.cap == CAP
    assert ses.kv_dtype == "fp8" and ses.kv1.k8.dtype == torch.uint8
    return ses, ses.g_net, ses.g_steps


def _same_session(m, ses, got):
    s, g_net, g_steps = ses
    assert got is s and s.g_net is g_net and s.g_steps is g_steps and s.g_noise is None, "the session was replaced or recaptured"
    assert [x for x in m._sessions.idle if x.kv_dtype == "fp8"] == [s], "one pooled session serves every seeded fp8 pool"


def test_alone_equals_beside_neighbours(orc, tok, medium_bf16, seeded_session):
    m = medium_bf16[2]
    _same_session(m, seeded_session, kc.alone_equals_beside_neighbours(m, orc, tok, CAP))


def test_a_child_repeats_its_parent(orc, tok, medium_bf16, seeded_session):
    m = medium_bf16[2]
    _same_session(m, seeded_session, kc.child_repeats_parent(m, orc, tok, CAP))


@pytest.mark.parametrize("alone", (False, True))
def test_a_held_request_forked_later_equals_an_uninterrupted_one(orc, tok, medium_bf16, seeded_session, alone):
    m = medium_bf16[2]
    _same_session(m, seeded_session, kc.held_then_forked_equals_uninterrupted(m, orc, tok, CAP, 5, alone))


def _n_steps(tok, ids):
    alive = [len(tok.events[tok.id_events[t]]) for t in ids if t != tok.eos_id]
    if not alive:
        return 2
    return alive[0] + 1 if all(a == alive[0] for a in alive) else tok.max_token_seq


def test_fp8_session_matches_oracle_within_the_references_own_fp8_effect(orc, tok, medium_bf16, golden):
    """The schedule of test_production_decode_session_matches_oracle at B = 4, P = 65, 4 events, on an fp8 session (filled by
    admit).  The oracle is driven twice on the device's ids: with orc.KV, and with a subclass whose update stores D(Q(.)) of every new
    K and V row per head; d_q = the largest difference of the two oracles' hidden states (likewise the logits) -- the reference's own
    statement of what fp8 K/V does.  Gate: the device within 1.5 ref_bf16_maxerr + 1.5 d_q of the EXACT-cache oracle, hidden and
    logits, and the greedy id equal to that oracle's wherever its top-2 margin exceeds twice the logits bound.
    Measured on the MI355X (printed): d_q 0.1298 (hidden) and 0.1115 (logits); worst hidden error 0.0786 against a bound
    of 0.3506, worst logits error 0.0557 against 0.2606; 24 of 96 ids had the margin and equalled the oracle's."""
    from midi_model_amd.decode import DecodeSession
    shp, sd, model = medium_bf16
    B, P, n_events = 4, 65, 4

    class QuantKV(orc.KV):
        def update(self, layer, k, v):
            return super().update(layer, ref_kvq.dequantize(*ref_kvq.quantize(k)), ref_kvq.dequantize(*ref_kvq.quantize(v)))

    g = golden("medium_long_S2048.npz")
    ref_h, ref_l = float(g["ref_bf16_hidden_maxerr"]), float(g["ref_bf16_logits_maxerr"])
    V = tok.vocab_size
    prompt = orc.synthetic_events(tok, B, P, seed=31)
    torch.set_num_threads(min(os.cpu_count() or 8, 32))
    hid_dev, log_dev, hid_o, hid_q, log_o, log_q, picks = [], [], [], [], [], [], []
    with torch.inference_mode():
        ses = DecodeSession(model, B, CAP, 1.0, 0.98, 1, ragged=True, row_params=True, kv_dtype="fp8")
        assert ses.g_net is not None and ses.g_noise is not None and ses.fold1 is not None and ses.fused_sampler
        graphs = (ses.g_net, ses.g_noise)
        ses.reset()
        ses.begin(torch.Generator(device="cuda").manual_seed(1))
        _admit(ses, model, list(range(B)), list(prompt))
        cache_o, cache_q = orc.KV(), QuantKV()
        ho = orc.midi_forward(sd, shp, prompt, cache_o)[:, -1]
        hq = orc.midi_forward(sd, shp, prompt, cache_q)[:, -1]
        for ev_i in range(n_events):
            assert ses.pos.tolist() == [P + ev_i] * B
            hid_dev.append(ses.hidden.float().cpu())
            hid_o.append(ho)
            hid_q.append(hq)
            c2o, c2q = orc.KV(), orc.KV()
            names, end = [""] * B, [False] * B
            n_steps, i, prev = tok.max_token_seq, 0, None
            while i < n_steps:
                ses.tok_step(i)
                ids = ses.seq[:, i].cpu()
                log_dev.append(ses.logits[:, :V].float().cpu())
                tin = None if i == 0 else prev[:, None]
                lo = orc.midi_forward_token(sd, shp, ho if i == 0 else None, tin, c2o)[:, -1]
                log_o.append(lo)
                log_q.append(orc.midi_forward_token(sd, shp, hq if i == 0 else None, tin, c2q)[:, -1])
                mask = orc.grammar_mask(tok, i, names, end).bool()
                assert mask.gather(1, ids[:, None]).all(), "the device sampled an id outside the grammar mask"
                top2 = lo.masked_fill(~mask, float("-inf")).topk(2, -1)
                picks.append((ids, top2.indices[:, 0], top2.values[:, 0] - top2.values[:, 1]))
                if i == 0:
                    names = [tok.id_events.get(int(t), "") for t in ids]
                    end = [int(t) == tok.eos_id for t in ids]
                    n_steps = _n_steps(tok, ids.tolist())
                prev = ids
                i += 1
            ses.consumed(n_steps)
            event = ses.seq.cpu().clone()
            ses.net_step()
            ho = orc.midi_forward(sd, shp, event[:, None, :], cache_o)[:, -1]
            hq = orc.midi_forward(sd, shp, event[:, None, :], cache_q)[:, -1]
        ses.end()
        assert (ses.g_net, ses.g_noise) == graphs
    dq_h = max(float((a - b).abs().max()) for a, b in zip(hid_o, hid_q))
    dq_l = max(float((a - b).abs().max()) for a, b in zip(log_o, log_q))
    err_h = max(float((a - b).abs().max()) for a, b in zip(hid_dev, hid_o))
    err_l = max(float((a - b).abs().max()) for a, b in zip(log_dev, log_o))
    hid_bound, log_bound = DRIFT * ref_h + DRIFT * dq_h, DRIFT * ref_l + DRIFT * dq_l
    safe = sum(int((m > 2 * log_bound).sum()) for _, _, m in picks)
    print(f"fp8 session vs oracle: d_q hidden {dq_h:.4f} logits {dq_l:.4f}; worst hidden err {err_h:.4f} (bound {hid_bound:.4f}), "
          f"worst logits err {err_l:.4f} (bound {log_bound:.4f}); {safe} of {sum(len(p[0]) for p in picks)} ids checked")
    assert err_h <= hid_bound, (err_h, hid_bound, dq_h)
    assert err_l <= log_bound, (err_l, log_bound, dq_l)
    for ids, best, margin in picks:
        ok = margin > 2 * log_bound
        assert (ids[ok] == best[ok]).all(), (ids.tolist(), best.tolist())
