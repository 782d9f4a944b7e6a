"""generate_ragged on the CPU: the schedules of engine.stack_decode(row_pos=...) and engine.stack_prefill_seqs, the ragged session's
bookkeeping (decode.py, model._checkout_session), the lockstep / retirement / live-rows-only break rule of model.generate_ragged and
its refusals, through the packed fake backend plus the stand-ins of the four new ops (tests/emu_ragged.py).  The kernels themselves:
test_ragged_kernels_gpu.py; the production session: test_ragged_gpu.py."""
import numpy as np
import pytest
import torch

import midi_model_amd as mm
from midi_model_amd import engine, ops

import emu_ragged
import ragged_common as rc


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


def _form(form):
    dt = torch.float32 if form.startswith("fp32") else torch.bfloat16
    # the tolerances test_shared_prompt_host.py derives: fp32 round-off of the float64 stand-ins against the fp32 emulator on
    # values of order 1; bf16: 2^-8 relative per rounding, a handful of roundings per layer x 4 layers
    return dt, (1e-5 if dt == torch.float32 else 0.06)


def _maxdiff(a, b):
    return (a.float() - b.float()).abs().max().item()


@pytest.mark.parametrize("form", ["fp32-general", "bf16-skinny", "bf16-folded"])
def test_stack_decode_rows_equals_uniform_per_row(tiny, form):
    """B = 4 rows at positions (0, 5, 17, 40), caches filled by stack_prefill_seqs, three decoded positions with different inputs
    per row: row b of the per-row form against the uniform form run (at the same B, same inputs) on a copy of the caches with
    kv.len = pos_b.  Layer 0 sees identical inputs on both sides: its written K/V rows are bit-equal."""
    B, steps, cap = 4, 3, 64
    positions = (0, 5, 17, 40)
    dt, tol = _form(form)
    with emu_ragged.install(), torch.no_grad():
        m = _model(tiny[1], dt)
        spec, W = m._specs["net"], m._W["net"]
        folded = engine.fold_norm_weights(W) if form == "bf16-folded" else None
        g = torch.Generator().manual_seed(11)
        lengths = [max(p, 1) for p in positions]   # (a sequence needs a row: position 0 overwrites it)
        xp = torch.randn((sum(lengths), spec.D), generator=g).to(dt)
        rope = engine.RopeTable(spec.hd, spec.theta, xp.device, cap)
        kv = engine.KVState(spec, B, cap, xp)
        kv.k.zero_(), kv.v.zero_()
        plan = ops.attn_seq_plan(lengths, spec.H).upload(xp.device)
        engine.stack_prefill_seqs(spec, W, xp, plan, rope, kv)
        assert kv.len == 0
        xs = [torch.randn((B, spec.D), generator=g).to(dt) for _ in range(steps)]
        uni = []
        for b, p in enumerate(positions):  # the uniform form first, on copies of the caches as the prefill left them
            kvu = engine.KVState(spec, B, cap, xp)
            kvu.k.copy_(kv.k), kvu.v.copy_(kv.v)
            kvu.len = p
            uni.append(([engine.stack_decode(spec, W, x, rope, kvu, folded=folded)[b].clone() for x in xs], kvu))
        pos = torch.tensor(positions, dtype=torch.int32)
        for i, x in enumerate(xs):
            y = engine.stack_decode(spec, W, x, rope, kv, folded=folded, row_pos=pos)
            assert torch.isfinite(y.float()).all() and kv.len == 0   # (with per-row positions kv.len is the caller's)
            for b in range(B):
                assert _maxdiff(y[b], uni[b][0][i]) <= tol, (form, i, b, _maxdiff(y[b], uni[b][0][i]))
            pos += 1
        for b, p in enumerate(positions):
            kvu = uni[b][1]
            assert torch.equal(kv.k[0, b, :, p:p + steps], kvu.k[0, b, :, p:p + steps])
            assert torch.equal(kv.v[0, b, :, p:p + steps], kvu.v[0, b, :, p:p + steps])
            assert _maxdiff(kv.k[:, b, :, :p + steps], kvu.k[:, b, :, :p + steps]) <= tol
            assert _maxdiff(kv.v[:, b, :, :p + steps], kvu.v[:, b, :, :p + steps]) <= tol
            assert (kv.k[:, b, :, p + steps:] == 0).all() and (kv.v[:, b, :, p + steps:] == 0).all()  # nothing behind the rows written


def test_stack_decode_rows_refuses_shared_and_pos_dev(tiny):
    from midi_model_amd.shared import SharedPrefix
    with emu_ragged.install(), torch.no_grad():
        m = _model(tiny[1])
        spec, W = m._specs["net"], m._W["net"]
        x = torch.zeros((2, spec.D))
        rope = engine.RopeTable(spec.hd, spec.theta, x.device, 8)
        kv, kvp = engine.KVState(spec, 2, 8, x), engine.KVState(spec, 1, 8, x)
        pos = torch.zeros(2, dtype=torch.int32)
        with pytest.raises(AssertionError):
            engine.stack_decode(spec, W, x, rope, kv, row_pos=pos, shared=SharedPrefix(kvp, None, torch.zeros(1)))
        with pytest.raises(AssertionError):
            engine.stack_decode(spec, W, x, rope, kv, row_pos=pos, pos_dev=torch.zeros(1, dtype=torch.int32))


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_stack_prefill_seqs_equals_prefill_per_sequence(tiny, dt):
    """lengths (1, 5, 17, 40) laid end to end through stack_prefill_seqs against stack_prefill sequence by sequence: cache rows
    [0, L_b) and the last hidden rows within the tolerances above; rows at or past L_b keep their sentinel."""
    lengths, cap, sentinel = (1, 5, 17, 40), 64, -3.0
    tol = 1e-5 if dt == torch.float32 else 0.06
    with emu_ragged.install(), torch.no_grad():
        m = _model(tiny[1], dt)
        spec, W = m._specs["net"], m._W["net"]
        g = torch.Generator().manual_seed(12)
        x = torch.randn((sum(lengths), spec.D), generator=g).to(dt)
        rope = engine.RopeTable(spec.hd, spec.theta, x.device, cap)
        kv = engine.KVState(spec, len(lengths), cap, x)
        kv.k.fill_(sentinel), kv.v.fill_(sentinel)
        plan = ops.attn_seq_plan(lengths, spec.H).upload(x.device)
        y = engine.stack_prefill_seqs(spec, W, x, plan, rope, kv)
        a = 0
        for b, L in enumerate(lengths):
            kv1 = engine.KVState(spec, 1, cap, x)
            y1 = engine.stack_prefill(spec, W, x[a:a + L], 1, L, rope, kv1)
            assert _maxdiff(y[a + L - 1], y1[L - 1]) <= tol, (b, _maxdiff(y[a + L - 1], y1[L - 1]))
            assert _maxdiff(kv.k[:, b, :, :L], kv1.k[:, 0, :, :L]) <= tol and _maxdiff(kv.v[:, b, :, :L], kv1.v[:, 0, :, :L]) <= tol
            assert (kv.k[:, b, :, L:] == sentinel).all() and (kv.v[:, b, :, L:] == sentinel).all()
            a += L
        # the store refuses a sequence the cache has no rows for (from the plan's host lengths, before the call)
        with pytest.raises(ValueError, match="rows in a cache"):
            ops.kv_store_seqs(torch.zeros((plan.M, 3 * spec.D), dtype=dt), plan, kv.k[0][:, :, :32], kv.v[0][:, :, :32], spec.H, spec.hd, 32)


def test_stand_ins_refuse_what_the_entry_points_refuse():
    z = torch.zeros
    pos = z(1, dtype=torch.int32)
    for hd in (32, 128, 256):
        c = z((8, hd // 2))
        kc = z((1, 1, 4, hd))
        with pytest.raises(RuntimeError, match="head_dim"):
            emu_ragged.kv_append_rows(z((1, 3 * hd)), c, c, kc, kc, 1, 1, hd, 4, pos)
        with pytest.raises(RuntimeError, match="head_dim"):
            emu_ragged.attn_decode_rows(z((1, 3 * hd)), kc, kc, z((1, hd)), 1, 1, hd, 4, 0.125, pos)
        with pytest.raises(RuntimeError, match="head_dim"):
            emu_ragged.attn_decode_append_rows(z((1, 3 * hd)), c, c, kc, kc, z((1, hd)), 1, 1, hd, 4, 0.125, pos)
    c, kc = z((8, 32)), z((1, 1, 4, 64))
    with pytest.raises(RuntimeError, match="NULL"):
        emu_ragged.attn_decode_append_rows(z((1, 192)), c, c, kc, kc, z((1, 64)), 1, 1, 64, 4, 0.125, None)


def test_generate_ragged_fp32_follows_the_oracle(orc, tok, tiny):
    """prompts of (1, 5, 127, 130) events, max_len 140, greedy, EOS banned: every row comes back with 140 events and its prompt in
    front, and the teacher-forced oracle agrees per row: the device's id is the oracle's masked arg-max wherever its top-2 margin
    exceeds 1e-3, and more than 0.95 of the positions are that safe (the oracle's own greedy continuation of these inputs:
    2335 of 2376, 0.983; the weakest row 0.975).  Row 3 retires after 10 events while row 0 runs 139: parking and the
    live-rows-only break rule are both on the path."""
    shp, sd = tiny
    ps = rc.prompts(orc, tok)
    with emu_ragged.install():
        m = _model(sd)
        out = m.generate_ragged(ps, max_len=rc.MAX_LEN, top_k=1, ban_eos=True)
    assert len(out) == 4
    checked = total = 0
    for b, (row, p) in enumerate(zip(out, ps)):
        assert row.shape == (rc.MAX_LEN, 8) and row.dtype == np.int64 and (row[:len(p)] == p).all(), b
        c, t = rc.oracle_argmax_check(orc, tok, sd, shp, row, len(p))
        assert t == (rc.MAX_LEN - len(p)) * 8
        checked, total = checked + c, total + t
    print(f"generate_ragged fp32 (tiny): {checked}/{total} sampling positions checked against the oracle's arg-max, all equal")
    assert total == 2376 and checked > 0.95 * total, (checked, total)


def test_session_bookkeeping(orc, tok, tiny):
    from midi_model_amd.decode import DecodeSession
    with emu_ragged.install():
        m = _model(tiny[1])
        plain = DecodeSession.make_key(m, 3, 256, 1.0, 0.98, 1)
        ragged = DecodeSession.make_key(m, 3, 256, 1.0, 0.98, 1, 0, True)
        assert ragged == plain + (("ragged",),) and ragged != plain
        with pytest.raises(ValueError, match="ragged"):
            DecodeSession.make_key(m, 3, 256, 1.0, 0.98, 1, 256, True)
        with pytest.raises(ValueError, match="ragged"):
            m._checkout_session(3, 100, 1.0, 0.98, 1, shared_need=10, ragged=True)
        with pytest.raises(ValueError, match="ragged"):
            DecodeSession(m, 3, 256, 1.0, 0.98, 1, shared_capacity=256, ragged=True)
        ps = rc.prompts(orc, tok, (2, 9, 4), seed0=50)
        out = m.generate_ragged(ps, max_len=12, top_k=1, ban_eos=True)
        assert [len(o) for o in out] == [12, 12, 12]
        assert len(m._sessions.idle) == 1
        ses = m._sessions.idle[0]
        assert ses.ragged and ses.key == ragged and ses.cap == 256 and ses.kvp is None
        assert ses.pos.shape == (3,) and ses.pos.dtype == torch.int32 and int(ses.pos_limit.item()) == 12
        # 10 event steps (row 0: 2 + 10 = 12), a net step after each but the last: rows 1, 2 are parked at max_len, row 0
        # stands at max_len - 1
        assert ses.pos.tolist() == [11, 12, 12]
        # other lengths, same B and capacity: the pooled session, not a new one
        ps2 = rc.prompts(orc, tok, (7, 1, 3), seed0=60)
        out2 = m.generate_ragged(ps2, max_len=9, top_k=1, ban_eos=True)
        assert [len(o) for o in out2] == [9, 9, 9]
        assert len(m._sessions.idle) == 1 and m._sessions.idle[0] is ses
        assert ses.pos.tolist() == [9, 8, 9] and int(ses.pos_limit.item()) == 9
        # a plain call of the same B does not take the ragged session
        m.generate(ps2[0], batch_size=3, max_len=9, top_k=1, ban_eos=True)
        assert len(m._sessions.idle) == 2 and sum(s.ragged for s in m._sessions.idle) == 1
        # equal lengths: the rule generate() runs, hence its ids (fp32, greedy) and its generator state
        g0, g1 = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
        p = rc.prompts(orc, tok, (6,), seed0=70)[0]
        a = m.generate_ragged([p, p, p], max_len=11, top_k=1, generator=g0)
        ref = m.generate(p, batch_size=3, max_len=11, top_k=1, generator=g1)
        assert all((a[b] == ref[b]).all() for b in range(3)) and torch.equal(g0.get_state(), g1.get_state())
        # a session refuses a limit or a prompt it has no cache row for
        with pytest.raises(ValueError, match="capacity"):
            ses.set_limit(256)
        with pytest.raises(ValueError, match="capacity"):
            ses.prefill_ragged(torch.zeros((258, 8), dtype=torch.long), [256, 1, 1])


def test_refusals_come_before_any_backend_call(orc, tok, tiny):
    with emu_ragged.install() as log:
        m = _model(tiny[1])
        del log[:]
        p = rc.prompts(orc, tok, (3, 6), seed0=80)
        V = tok.vocab_size
        bad_id, neg = p[1].copy(), p[1].copy()
        bad_id[2, 1], neg[0, 0] = V, -1
        for fn in (m.generate_ragged, m.generate_stream_ragged):
            for prompts, kw, match in (
                    ([], {}, "no prompts"),
                    ([p[0], p[1][:0]], {}, "shape"),
                    ([p[0], p[1]], dict(max_len=6), "nothing to generate"),
                    ([p[0], p[1]], dict(max_len=5), "nothing to generate"),
                    ([p[0], bad_id], {}, "outside"),
                    ([neg, p[1]], {}, "outside"),
                    ([p[0], p[1]], dict(disable_channels=[16]), "disable_channels"),
                    ([p[0], p[1]], dict(disable_channels=list(range(16))), "every channel"),
            ):
                with pytest.raises(ValueError, match=match):
                    fn(prompts, **kw)
                assert not log and not m._sessions.idle, (fn.__name__, match, log[:3])
        # the messages are _generate_events' own
        with pytest.raises(ValueError) as e0:
            list(m.generate_stream(p[0], max_len=9, disable_channels=[16]))
        with pytest.raises(ValueError) as e1:
            m.generate_ragged(p, max_len=9, disable_channels=[16])
        assert str(e0.value) == str(e1.value)


def test_stream_form_and_mask_options(orc, tok, tiny):
    with emu_ragged.install():
        m = _model(tiny[1])
        ps = [q[:, :t] for q, t in zip(rc.prompts(orc, tok, (2, 9, 4), seed0=90), (8, 5, 8))]   # (T' < 8: padded)
        opts = dict(max_len=14, top_k=1, disable_patch_change=True, disable_control_change=True, disable_channels=[0, 9])
        ref = m.generate_ragged(ps, **opts)
        rows = [[] for _ in ps]
        banned = [tok.parameter_ids["channel"][c] for c in (0, 9)]
        steps = 0
        for ev, live in m.generate_stream_ragged(ps, **opts):
            assert ev.shape == (3, 8) and ev.dtype == np.int64 and live.shape == (3,) and live.dtype == np.bool_
            assert (live == (np.array([2, 9, 4]) + steps < 14)).all()
            for b in np.flatnonzero(live):
                rows[b].append(ev[b])
                assert ev[b, 0] not in (tok.event_ids["patch_change"], tok.event_ids["control_change"])
                assert not np.isin(ev[b], banned).any()
            steps += 1
        for b, p in enumerate(ps):
            assert (ref[b][:len(p), :p.shape[1]] == p).all() and (ref[b][:len(p), p.shape[1]:] == tok.pad_id).all()
            assert (np.stack(rows[b]) == ref[b][len(p):]).all()
        # the stream form crops a prompt to its last 4096 events before it looks at max_len; generate_ragged does not crop
        long = np.repeat(ps[0][:1], 4100, axis=0)
        assert m._ragged_prompts([long, ps[1]], 4098, 4096)[0].shape == (4096, 8)
        with pytest.raises(ValueError, match="nothing to generate"):
            m.generate_ragged([long, ps[1]], max_len=4098, top_k=1)
