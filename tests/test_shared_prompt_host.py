"""generate(share_prompt=True) on the CPU: the schedule of engine.stack_decode(shared=...), the session bookkeeping of
decode.py / model._checkout_session and the prompt-form validation, through the fake backend (tests/emu_ops.py) plus the float64
stand-ins of the two shared-prefix ops (tests/emu_shared.py).  The kernels themselves: test_shared_prefix_kernels_gpu.py."""
import numpy as np
import pytest
import torch

import midi_model_amd as mm
from midi_model_amd import engine
from midi_model_amd.shared import SharedPrefix, workspace_floats

import emu_shared


def tiny_config():
    return mm.MIDIModelConfig.get_config("v2", True, 4, 4, 256, 512)


@pytest.fixture(scope="module")
def tok():
    return mm.MIDITokenizerV2()


@pytest.fixture(scope="module")
def tiny_sd(orc, tok):
    shp = orc.Shape(n_layer=4, n_head=4, n_embd=256, n_inner=512, vocab=tok.vocab_size)
    return orc.make_state_dict(shp, seed=1)


def _model(sd, dtype=torch.float32):
    m = mm.MIDIModel(tiny_config())
    m.load_state_dict(sd)
    return m.to(dtype)


@pytest.mark.parametrize("P", [1, 5])
@pytest.mark.parametrize("form", ["fp32-general", "bf16-skinny", "bf16-folded"])
def test_stack_decode_shared_equals_plain_on_replicated_cache(tiny_sd, P, form):
    """B rows behind one prompt of P positions, 3 decoded positions with DIFFERENT inputs per row: the shared form (prompt cached
    once, suffix per row) against the plain form on a cache that holds the prompt B times.  fp32: round-off of the float64
    stand-ins against the fp32 emulator (1e-5 on values of order 1); bf16: both sides round every activation to bf16 (2^-8
    relative per rounding, a handful of roundings per layer x 4 layers: 0.06 on values of order 1)."""
    B, steps = 3, 3
    dt = torch.float32 if form.startswith("fp32") else torch.bfloat16
    tol = 1e-5 if dt == torch.float32 else 0.06
    with emu_shared.install(), torch.no_grad():
        m = _model(tiny_sd, dt)
        spec, W = m._specs["net"], m._W["net"]
        folded = engine.fold_norm_weights(W) if form == "bf16-folded" else None
        g = torch.Generator().manual_seed(10 + P)
        xp = torch.randn((P, spec.D), generator=g).to(dt)
        rope = engine.RopeTable(spec.hd, spec.theta, xp.device, 64)
        kv = engine.KVState(spec, B, 16, xp)
        engine.stack_prefill(spec, W, xp.repeat(B, 1), B, P, rope, kv)
        kvp = engine.KVState(spec, 1, 8, xp)
        engine.stack_prefill(spec, W, xp, 1, P, rope, kvp)
        kvs = engine.KVState(spec, B, 4, xp)
        ws = torch.full((workspace_floats(B, spec.H, kvp.cap),), float("nan"))
        for i in range(steps):
            x1 = torch.randn((B, spec.D), generator=g).to(dt)
            y0 = engine.stack_decode(spec, W, x1, rope, kv, folded=folded)
            y1 = engine.stack_decode(spec, W, x1, rope, kvs, folded=folded, shared=SharedPrefix(kvp, None, ws))
            assert torch.isfinite(y1.float()).all()
            assert (y1.float() - y0.float()).abs().max().item() <= tol, (i, (y1.float() - y0.float()).abs().max().item())
            assert kvs.len == i + 1 and kvp.len == P and kv.len == P + i + 1
        # the suffix rows are the plain cache's rows behind the prompt (layer 0 sees identical inputs: bit-equal there)
        assert torch.equal(kvs.k[0][:, :, :steps], kv.k[0][:, :, P:P + steps])
        assert torch.equal(kvs.v[0][:, :, :steps], kv.v[0][:, :, P:P + steps])
        assert (kvs.k[:, :, :, :steps].float() - kv.k[:, :, :, P:P + steps].float()).abs().max().item() <= tol
        # ... and the prompt's cache is row 0 of the plain one (a CPU matmul over B x P rows rounds unlike one over P rows)
        assert (kvp.k[:, 0, :, :P].float() - kv.k[:, 0, :, :P].float()).abs().max().item() <= tol
        assert (kvp.v[:, 0, :, :P].float() - kv.v[:, 0, :, :P].float()).abs().max().item() <= tol


def test_stack_decode_shared_device_positions(tiny_sd):
    """pos / pre_len from (device) int32 tensors -- the form a captured graph replays -- give what the host values give"""
    B, P = 2, 5
    with emu_shared.install(), torch.no_grad():
        m = _model(tiny_sd)
        spec, W = m._specs["net"], m._W["net"]
        g = torch.Generator().manual_seed(3)
        xp, x1 = torch.randn((P, spec.D), generator=g), torch.randn((B, spec.D), generator=g)
        rope = engine.RopeTable(spec.hd, spec.theta, xp.device, 64)
        outs = []
        for dev in (False, True):
            kvp, kvs = engine.KVState(spec, 1, 8, xp), engine.KVState(spec, B, 4, xp)
            kvs.k.zero_(), kvs.v.zero_()
            engine.stack_prefill(spec, W, xp, 1, P, rope, kvp)
            ws = torch.zeros((workspace_floats(B, spec.H, kvp.cap),))
            pos, pre = torch.tensor([P], dtype=torch.int32), torch.tensor([P], dtype=torch.int32)
            sh = SharedPrefix(kvp, pre if dev else None, ws)
            outs.append((engine.stack_decode(spec, W, x1, rope, kvs, pos_dev=pos if dev else None, shared=sh), kvs.k.clone()))
            assert kvs.len == (0 if dev else 1)  # (with device positions kv.len is the caller's)
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_session_bookkeeping_and_capacities(tiny_sd, orc, tok):
    with emu_shared.install():
        m = _model(tiny_sd)
        from midi_model_amd.decode import DecodeSession
        # capacities: both by the doubling rule from 256; the plain key keeps its form, the shared key gains the prompt capacity
        plain = DecodeSession.make_key(m, 2, 256, 1.0, 0.98, 20)
        assert len(plain) == 7 and DecodeSession.make_key(m, 2, 256, 1.0, 0.98, 20, 0) == plain
        ses = m._checkout_session(2, 700, 1.0, 0.98, 20, shared_need=300)
        assert (ses.cap, ses.shared_capacity) == (1024, 512) and ses.key == plain[:3] + (1024,) + plain[4:] + (("shared", 512),)
        assert ses.kvp.k.shape[1] == 1 and ses.kvp.cap == 512 and ses.kv1.cap == 1024 and ses.kv1.k.shape[1] == 2
        assert ses.ws.numel() == workspace_floats(2, 4, 512) and ses.rope1.n >= 1024 + 512
        assert m._checkout_session(2, 257, 1.0, 0.98, 20).kvp is None
        # a prompt longer than the session's prompt cache is refused
        with pytest.raises(ValueError, match="shared capacity"):
            ses.prefill(torch.zeros((2, 513, 8), dtype=torch.long))
        # one generate call: prompt of 5 events, 3 rows, 4 new events
        prompt = orc.synthetic_events(tok, 1, 5, seed=7)[0].numpy()
        gen = torch.Generator().manual_seed(5)
        out = m.generate(prompt, batch_size=3, max_len=9, top_k=1, ban_eos=True, generator=gen, share_prompt=True)
        gen0 = torch.Generator().manual_seed(5)
        ref = m.generate(prompt, batch_size=3, max_len=9, top_k=1, ban_eos=True, generator=gen0)
        assert out.shape == ref.shape == (3, 9, 8) and out.dtype == ref.dtype and (out[:, :5] == prompt[None]).all()
        assert (out == ref).all()                       # (fp32 on the CPU: greedy ids agree with the plain path)
        assert torch.equal(gen.get_state(), gen0.get_state())
        ses = [s for s in m._sessions.idle if s.kvp is not None][-1]
        assert ses.shared_capacity == 256 and ses.cap == 256 and ses.kvp.len == 5 and int(ses.pre_len.item()) == 5
        # 4 events sampled, a net step after each but the last: suffix rows 0..2, position 5 + 3
        assert ses.kv1.len == 3 and int(ses.pos.item()) == 8
        # the suffix cache holds each row's own rows; the prompt cache one sequence
        assert ses.kv1.k.shape[1:4] == (3, 4, 256) and ses.kvp.k.shape[1:4] == (1, 4, 256)
        # the same pooled session serves another prompt length
        n_idle = len(m._sessions.idle)
        p2 = orc.synthetic_events(tok, 1, 3, seed=8)[0].numpy()
        out2 = m.generate(p2, batch_size=3, max_len=6, top_k=1, ban_eos=True, share_prompt=True)
        assert (out2 == m.generate(p2, batch_size=3, max_len=6, top_k=1, ban_eos=True)).all()
        assert len([s for s in m._sessions.idle if s.kvp is not None]) == 1 and len(m._sessions.idle) == n_idle
        assert m._sessions.idle[-1] is not None and ses.kvp.len == 3 and int(ses.pre_len.item()) == 3


def test_prompt_forms(tiny_sd, orc, tok):
    with emu_shared.install():
        m = _model(tiny_sd)
        p = orc.synthetic_events(tok, 1, 6, seed=9)[0].numpy()
        kw = dict(batch_size=3, max_len=9, top_k=1, ban_eos=True, share_prompt=True)
        a = m.generate(p, **kw)
        assert (m.generate(p[None], **kw) == a).all() and (m.generate(np.stack([p] * 3), **kw) == a).all()
        assert (m.generate(p[:, :5], **kw) == m.generate(p[:, :5], **{**kw, "share_prompt": False})).all()  # (T' < 8: padded)
        bad = np.stack([p] * 3)
        bad[2, 4, 1] += 1
        with pytest.raises(ValueError, match="row 2 differs"):
            m.generate(bad, **kw)
        with pytest.raises(ValueError, match="row 1 differs"):
            next(m.generate_stream(np.stack([p, p[::-1], p[::-1]]), batch_size=3, max_len=9, share_prompt=True))
        with pytest.raises(ValueError, match="invalid shape"):
            m.generate(np.stack([p] * 2), **kw)
        # nothing to share without a prompt: the plain path, bit for bit, and no shared session is made
        n_shared = len([s for s in m._sessions.idle if s.kvp is not None])
        g0, g1 = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
        assert (m.generate(None, batch_size=2, max_len=8, generator=g0, share_prompt=True)
                == m.generate(None, batch_size=2, max_len=8, generator=g1)).all()
        assert len([s for s in m._sessions.idle if s.kvp is not None]) == n_shared
        # the serving form yields generate()'s events, under the mask options too
        evs = list(m.generate_stream(p, batch_size=3, max_len=9, top_k=1, share_prompt=True, disable_patch_change=True,
                                     disable_channels=[0]))
        ref = m.generate(p, batch_size=3, max_len=9, top_k=1, share_prompt=True, disable_patch_change=True, disable_channels=[0])
        assert (np.stack(evs, 1) == ref[:, 6:]).all()
        assert not np.isin(np.stack(evs, 1)[:, :, 0], [tok.event_ids["patch_change"]]).any()
        assert not np.isin(np.stack(evs, 1), [tok.parameter_ids["channel"][0]]).any()


def test_stand_ins_refuse_what_the_entry_points_refuse():
    from emu_shared import attn_decode_append_shared, attn_prefix_partial
    z = torch.zeros
    B, H = 1, 1
    cos, sin = z((8, 32)), z((8, 32))
    ws = z((66,))
    for hd in (32, 128, 256):
        with pytest.raises(RuntimeError, match="head_dim"):
            attn_prefix_partial(z((B, 3 * hd)), cos, sin, z((H, 4, hd)), z((H, 4, hd)), ws, B, H, hd, 4, 1, 1, 0.125)
    q, kp, ks = z((B, 192)), z((H, 4, 64)), z((B, H, 2, 64))
    for pre, pos in ((0, 1), (5, 5), (3, 2)):
        with pytest.raises(RuntimeError, match="bad args"):
            attn_prefix_partial(q, cos, sin, kp, kp, ws, B, H, 64, 4, pre, pos, 0.125)
        with pytest.raises(RuntimeError, match="bad args"):
            attn_decode_append_shared(q, cos, sin, ks, ks, ws, z((B, 64)), B, H, 64, 2, 4, pre, pos, 0.125)
    with pytest.raises(RuntimeError, match="bad args"):  # a full suffix
        attn_decode_append_shared(q, cos, sin, ks, ks, ws, z((B, 64)), B, H, 64, 2, 4, 2, 4, 0.125)
