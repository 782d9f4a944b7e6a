"""generate_ragged on the MI355X: B prompts of B lengths in one decode batch.  The per-row decode schedule against the uniform one
bit for bit, the production session (bf16, captured graphs, folded norms, fused sampler, a position per row) against the CPU oracle
following every row through its own cache, fp32 ``generate_ragged`` id for id against the teacher-forced oracle (one row retires
after 10 events while another runs 139), and determinism / reuse of the pooled session for another mix of lengths."""
import copy
import os

import numpy as np
import pytest
import torch

import midi_model_amd as mm
from midi_model_amd import engine

import ragged_common as rc

pytestmark = pytest.mark.gpu

DRIFT = 1.5   # x the reference's own bf16 error (medium_long_S2048.npz), as test_decode_gpu.py


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
    shp, sd, m = medium
    return shp, sd, copy.deepcopy(m).to("cuda", torch.bfloat16).eval()


@pytest.fixture(scope="module")
def medium_fp32(medium):
    shp, sd, m = medium
    return shp, sd, copy.deepcopy(m).to("cuda", torch.float32).eval()


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def test_stack_decode_rows_equals_uniform_bit_for_bit(medium_bf16):
    """tv2o-medium bf16, B = 4, rows at positions (0, 5, 127, 300), the folded-skinny form, caches of seeded random values: row b of
    stack_decode(row_pos=...) and the K/V rows it writes, in every layer, against the uniform stack_decode run at the same B (every
    projection the same instantiation, rows independent) on a copy of the caches with kv.len = pos_b.  Identical bits."""
    shp, sd, m = medium_bf16
    spec, W = m._specs["net"], m._W["net"]
    B, cap, positions = 4, 512, (0, 5, 127, 300)
    g = torch.Generator(device="cuda").manual_seed(21)
    with torch.inference_mode():
        folded = engine.fold_norm_weights(W)
        rope = engine.RopeTable(spec.hd, spec.theta, "cuda", cap)
        kv = engine.KVState(spec, B, cap, m._flat)
        kv.k.copy_(torch.randn(kv.k.shape, generator=g, device="cuda"))
        kv.v.copy_(torch.randn(kv.v.shape, generator=g, device="cuda"))
        k0, v0 = kv.k.clone(), kv.v.clone()
        x = torch.randn((B, spec.D), generator=g, device="cuda").to(torch.bfloat16)
        row_pos = torch.tensor(positions, dtype=torch.int32, device="cuda")
        y = engine.stack_decode(spec, W, x, rope, kv, folded=folded, row_pos=row_pos)
        assert kv.len == 0 and torch.isfinite(y.float()).all()
        ek, ev = k0.clone(), v0.clone()
        for b, p in enumerate(positions):
            kvu = engine.KVState(spec, B, cap, m._flat)
            kvu.k.copy_(k0), kvu.v.copy_(v0)
            kvu.len = p
            yu = engine.stack_decode(spec, W, x, rope, kvu, folded=folded)
            assert torch.equal(bits(y[b]), bits(yu[b])), (b, p, (y[b].float() - yu[b].float()).abs().max().item())
            assert torch.equal(bits(kv.k[:, b, :, p]), bits(kvu.k[:, b, :, p])) and torch.equal(bits(kv.v[:, b, :, p]), bits(kvu.v[:, b, :, p]))
            ek[:, b, :, p], ev[:, b, :, p] = kvu.k[:, b, :, p], kvu.v[:, b, :, p]
        assert torch.equal(bits(kv.k), bits(ek)) and torch.equal(bits(kv.v), bits(ev)), "a cache row other than row_pos[b] changed"


def test_ragged_decode_session_matches_oracle(orc, tok, medium_bf16, golden):
    """test_shared_decode_session_matches_oracle with a ragged session: prompts of (1, 5, 127, 300) events (seeds 41 + b), B = 4,
    graphs captured, folded norms, fused sampler, 4 events, the oracle following each row through its OWN cache.  After every
    replayed graph the hidden state / logits of every row are within the reference's own bf16 drift (x1.5, medium_long_S2048.npz) of
    the oracle's fp32 forward on the same tokens, every sampled id is inside the grammar mask, and it equals the oracle's masked
    arg-max wherever the oracle's top-2 margin exceeds twice the logits bound (the bounds hold at every position, so no minimum
    share of checked ids is asked for)."""
    from midi_model_amd.decode import DecodeSession
    shp, sd, model = medium_bf16
    g = golden("medium_long_S2048.npz")
    hid_bound = DRIFT * float(g["ref_bf16_hidden_maxerr"])
    log_bound = DRIFT * float(g["ref_bf16_logits_maxerr"])
    V = tok.vocab_size
    lengths, n_events, max_len = (1, 5, 127, 300), 4, 400
    B = len(lengths)
    ps = [torch.from_numpy(p) for p in rc.prompts(orc, tok, lengths)]
    torch.set_num_threads(min(os.cpu_count() or 8, 32))
    with torch.inference_mode():
        ses = DecodeSession(model, B, 512, 1.0, 0.98, 1, ragged=True)
        assert ses.ragged and ses.pos.shape == (B,) and ses.kvp is None
        assert ses.g_net is not None and ses.g_steps is not None and ses.g_noise is not None, "captured graphs are the production form"
        assert ses.fold1 is not None and ses.lm_fold is not None and ses.fused_sampler, "folded norms + fused sampler"
        ses.first_mask.copy_(model._grammar()[0])
        ses.ban.zero_()
        ses.reset()
        ses.begin(torch.Generator(device="cuda").manual_seed(1))
        ses.set_limit(max_len)
        ses.prefill_ragged(torch.cat(ps).cuda(), lengths)
        caches = [orc.KV() for _ in range(B)]
        hid_o = torch.cat([orc.midi_forward(sd, shp, p[None], c)[:, -1] for p, c in zip(ps, caches)])
        worst_h, worst_l, checked, total = 0.0, 0.0, 0, 0
        for ev_i in range(n_events):
            assert ses.pos.tolist() == [L + ev_i for L in lengths] and int(ses.pos_limit.item()) == max_len
            err = (ses.hidden.float().cpu() - hid_o).abs().max(-1).values
            worst_h = max(worst_h, err.max().item())
            assert err.max().item() <= hid_bound, (ev_i, err.tolist(), hid_bound)
            cache2 = orc.KV()
            names, end = [""] * B, [False] * B
            n_steps, i, prev = tok.max_token_seq, 0, None
            while i < n_steps:
                ses.tok_step(i)
                lg = ses.logits[:, :V].float().cpu()
                ids = ses.seq[:, i].cpu()
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
                total += B
                checked += int(safe.sum())
                assert (ids[safe] == top2.indices[:, 0][safe]).all(), (ev_i, i, ids.tolist(), top2.indices[:, 0].tolist())
                if i == 0:
                    names = [tok.id_events.get(int(t), "") for t in ids]
                    end = [int(t) == tok.eos_id for t in ids]
                    n_steps = rc.n_steps(tok, ids.tolist())
                prev = ids
                i += 1
            ses.consumed(n_steps)
            event = ses.seq.cpu().clone()
            ses.net_step()
            hid_o = torch.cat([orc.midi_forward(sd, shp, event[b][None, None, :], caches[b])[:, -1] for b in range(B)])
        ses.end()
    print(f"ragged session vs oracle (lengths {lengths}): worst hidden err {worst_h:.4f} (bound {hid_bound:.4f}), worst logits err "
          f"{worst_l:.4f} (bound {log_bound:.4f}); greedy ids checked on {checked}/{total} rows with a safe margin")


def test_generate_ragged_fp32_follows_the_oracle_id_for_id(orc, tok, medium_fp32):
    """generate_ragged itself: fp32 tv2o-medium, greedy, EOS banned, prompts of (1, 5, 127, 130) events, max_len 140 -- the inputs
    of the host test.  Every row comes back with 140 events behind its intact prompt; teacher-forced oracle per row, margin 1e-3,
    checked share above 0.97 (the oracle's own greedy continuation of these inputs on the CPU: 2367 of 2376, 0.996; every row at
    least 0.995).  Row 3 retires after 10 events and stays parked for 129 more while row 0 runs 139."""
    shp, sd, m = medium_fp32
    ps = rc.prompts(orc, tok)
    out = m.generate_ragged(ps, max_len=rc.MAX_LEN, top_k=1, ban_eos=True)
    ses = m._sessions.idle[-1]
    assert ses.ragged and ses.cap == 256 and ses.pos.tolist() == [rc.MAX_LEN - 1] + [rc.MAX_LEN] * 3
    checked = total = 0
    for b, (row, p) in enumerate(zip(out, ps)):
        assert row.shape == (rc.MAX_LEN, 8) and row.dtype == np.int64 and (row[:len(p)] == p).all(), b
        c, t = rc.oracle_argmax_check(orc, tok, sd, shp, row, len(p))
        checked, total = checked + c, total + t
    print(f"generate_ragged fp32 (tv2o-medium): {checked}/{total} sampling positions checked against the oracle's arg-max, all equal")
    assert total == 2376 and checked > 0.97 * total, (checked, total)


def test_determinism_and_pooled_session_reuse(orc, tok, medium_bf16):
    """bf16, top_k 20: two calls with generators seeded alike give identical rows and leave the generators in the same state; a
    second mix of lengths (same B, same capacity) runs on the SAME pooled session without a recapture -- the captured graphs read
    pos and pos_limit from device memory and their launch geometry depends on B and the capacity only."""
    shp, sd, m = medium_bf16
    m._sessions.idle.clear()
    ps = rc.prompts(orc, tok, (3, 40, 17, 130), seed0=51)
    g0, g1 = torch.Generator(device="cuda").manual_seed(9), torch.Generator(device="cuda").manual_seed(9)
    a = m.generate_ragged(ps, max_len=150, top_k=20, generator=g0)
    assert len(m._sessions.idle) == 1
    ses = m._sessions.idle[0]
    g_net, g_steps, key = ses.g_net, ses.g_steps, ses.key
    assert ses.ragged and g_net is not None and g_steps is not None
    b = m.generate_ragged(ps, max_len=150, top_k=20, generator=g1)
    assert all(x.shape == y.shape and (x == y).all() for x, y in zip(a, b)) and torch.equal(g0.get_state(), g1.get_state())
    for row, p in zip(a, ps):
        assert len(p) < len(row) <= 150 and (row[:len(p)] == p).all()
    ps2 = rc.prompts(orc, tok, (90, 2, 61, 8), seed0=61)
    c = m.generate_ragged(ps2, max_len=100, top_k=20, ban_eos=True, generator=g0)
    assert [len(r) for r in c] == [100] * 4 and all((r[:len(p)] == p).all() for r, p in zip(c, ps2))
    assert len(m._sessions.idle) == 1 and m._sessions.idle[0] is ses and ses.key == key
    assert ses.g_net is g_net and ses.g_steps is g_steps, "the session was recaptured"
    assert ses.pos.tolist() == [100, 99, 100, 100] and int(ses.pos_limit.item()) == 100
