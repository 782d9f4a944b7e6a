"""Event log-likelihoods on the CPU: DecodeSession(logprobs=True) / DecodePool(logprobs=True) / generate_pool(logprobs=True) and
MIDIModel.score, through the fake backend plus the stand-ins of the two ``_logp`` sampler forms (tests/emu_logp.py).  Tiny 4-layer
model, fp32 (bf16 for the fp8-cache form).  The kernels: test_logp_kernels_gpu.py; the production session: test_logp_pool_gpu.py."""
import numpy as np
import pytest
import torch

import midi_model_amd as mm
from midi_model_amd.decode import DecodeSession

import emu_kvq
import emu_logp
import emu_poolshare
import fork_common as fc
import logp_common as lc
import ragged_common as rc
import ref_logp

LOGP_OPS = ("sample_top_p_k_rows_logp", "sample_top_p_k_seeded_logp")


@pytest.fixture(scope="module")
def tok():
    return mm.MIDITokenizerV2()


@pytest.fixture(scope="module")
def tiny(orc, tok):
    shp = orc.Shape(n_layer=4, n_head=4, n_embd=256, n_inner=512, vocab=tok.vocab_size)
    return shp, orc.make_state_dict(shp, seed=0)


def _model(sd, dtype=torch.float32):
    m = mm.MIDIModel(mm.MIDIModelConfig.get_config("v2", True, 4, 4, 256, 512))
    m.load_state_dict(sd)
    return m.to(dtype)


def test_refusals_come_before_any_launch(orc, tok, tiny):
    p = rc.prompts(orc, tok, (5,), seed0=600)[0]
    with emu_logp.install() as log:
        m = _model(tiny[1])
        del log[:]
        for args in ((m, 4, 256, 1.0, 0.98, 1, 0, True, False), (m, 4, 256, 1.0, 0.98, 1, 0, False, False),
                     (m, 4, 256, 1.0, 0.98, 1, 64, False, False)):
            with pytest.raises(ValueError, match="row_params"):
                DecodeSession.make_key(*args, logprobs=True)
            with pytest.raises(ValueError, match="row_params"):
                DecodeSession(*args, logprobs=True)
        with m.decode_pool(4, 64) as pool:
            rid = pool.submit(p, max_len=8)
            with pytest.raises(ValueError, match="logprobs=True"):
                pool.logprobs(rid)
        with pytest.raises(ValueError, match="events >= 2"):
            m.score(torch.zeros((1, 1, 8), dtype=torch.long))
        with pytest.raises(ValueError, match="lengths"):
            m.score(torch.zeros((2, 3, 8), dtype=torch.long), lengths=[3])
        with pytest.raises(ValueError, match="lengths"):
            m.score(torch.zeros((2, 3, 8), dtype=torch.long), lengths=[3, 4])
        assert log == [], log
    # the entry points' own two refusals, as the stand-ins restate them
    B, V = 2, 64
    z = torch.zeros((B, V))
    one = torch.ones(V, dtype=torch.uint8)
    tabs = torch.zeros((V, 8), dtype=torch.int32)
    args = (z, one, tabs, tabs, torch.zeros(B, dtype=torch.int64), 0, torch.ones((B, V)), torch.zeros(B, dtype=torch.int64), V,
            torch.ones(B), torch.ones(B), torch.ones(B, dtype=torch.int32), torch.zeros(V, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="logp is NULL"):
        emu_logp.sample_top_p_k_rows_logp(*args, None, first_span=(0, V))
    with pytest.raises(RuntimeError, match="logp_stride"):
        emu_logp.sample_top_p_k_rows_logp(*args, torch.zeros(1).expand(B), first_span=(0, V))


def test_session_keys(orc, tok, tiny):
    with emu_logp.install():
        m, mb = _model(tiny[1]), _model(tiny[1], torch.bfloat16)
        for seeded in (False, True):
            form = ("ragged", "row_params", "seeded") if seeded else ("ragged", "row_params")
            plain = DecodeSession.make_key(m, 4, 256, 1.0, 0.98, 1, 0, True, True, seeded)
            assert plain == (m._flat.data_ptr(), m._flat.dtype, 4, 256, form), "the key without the option is what it was"
            assert DecodeSession.make_key(m, 4, 256, 1.0, 0.98, 1, 0, True, True, seeded, logprobs=False) == plain
            assert DecodeSession.make_key(m, 4, 256, 1.0, 0.98, 1, 0, True, True, seeded, logprobs=True) == \
                plain[:4] + (form + (("logp",),),)
            slots = DecodeSession.make_key(m, 4, 256, 1.0, 0.98, 1, 0, True, True, seeded, 2, 64)
            assert slots == plain[:4] + (form + (("slots", 2, 64),),)
            assert DecodeSession.make_key(m, 4, 256, 1.0, 0.98, 1, 0, True, True, seeded, 2, 64, logprobs=True) == \
                plain[:4] + (form + (("slots", 2, 64), ("logp",)),)
            q = DecodeSession.make_key(mb, 4, 256, 1.0, 0.98, 1, 0, True, True, seeded, kv_dtype="fp8")
            assert q == (mb._flat.data_ptr(), mb._flat.dtype, 4, 256, form + (("kv", "fp8"),))
            assert DecodeSession.make_key(mb, 4, 256, 1.0, 0.98, 1, 0, True, True, seeded, kv_dtype="fp8", logprobs=True) == \
                q[:4] + (form + (("kv", "fp8"), ("logp",)),)
        # the uniform, ragged and shared keys are untouched
        assert DecodeSession.make_key(m, 4, 256, 1.0, 0.98, 20) == (m._flat.data_ptr(), m._flat.dtype, 4, 256, 1.0, 0.98, 20)
        p = rc.prompts(orc, tok, (5,), seed0=601)[0]
        keys = []
        for kw in ({}, dict(logprobs=True)):
            with m.decode_pool(4, 64, **kw) as pool:
                pool.submit(p, max_len=8, top_k=1)
                pool.step()
                keys.append(pool.ses.key)
                assert pool.ses.logprobs == bool(kw) and (pool.ses.logp_rows is not None) == bool(kw)
        assert keys[0] != keys[1] and len(m._sessions.idle) == 2, "a pool with the option never takes a session without it"


def _run(m, orc, tok, seeded, **kw):
    p, q = rc.prompts(orc, tok, (7, 4), seed0=560)
    gen = {} if seeded else dict(generator=torch.Generator().manual_seed(5))
    with m.decode_pool(5, 64, seeded=seeded, **gen, **kw) as pool:
        s = (lambda *v: dict(seed=list(v) if len(v) > 1 else v[0])) if seeded else (lambda *v: {})
        a, b, c = pool.submit(p, max_len=14, n=3, **s(1, 2, 3), **fc.KW)
        pool.submit(q, max_len=9, **s(4), **fc.KW)
        for _ in range(3):
            pool.step()
        kid, = pool.fork(a, **s(9))
        fc.drain(pool)
        return [pool.result(i) for i in (a, b, c, kid)]


@pytest.mark.parametrize("seeded", (False, True))
def test_call_log(orc, tok, tiny, seeded):
    """a pool without the option logs what it logs without this feature's stand-ins installed, and no _logp op; with the option the
    _logp forms replace the plain samplers one for one and nothing else moves -- the ids included"""
    plain = "sample_top_p_k_seeded" if seeded else "sample_top_p_k_rows"
    with emu_kvq.install() as log0:
        m = _model(tiny[1])
        del log0[:]
        a, la = _run(m, orc, tok, seeded), list(log0)
    with emu_logp.install() as log:
        m = _model(tiny[1])
        del log[:]
        b, lb = _run(m, orc, tok, seeded), list(log)
        assert la == lb and not any(n in lb for n in LOGP_OPS) and all(fc.same(x, y) for x, y in zip(a, b))
        del log[:]
        c, lq = _run(m, orc, tok, seeded, logprobs=True), list(log)
    assert all(fc.same(x, y) for x, y in zip(b, c)), "the option changes no id"
    assert plain not in lq and lq.count(plain + "_logp") == lb.count(plain) > 0
    assert [n[:-5] if n in LOGP_OPS else n for n in lq] == lb


@pytest.mark.parametrize("seeded", (False, True))
def test_pool_logprobs_against_the_oracle(orc, tok, tiny, seeded):
    """3e-5 per token: the gate test_host_logic.py holds this backend's loss to"""
    shp, sd = tiny
    kw = dict(seeded=True) if seeded else dict(generator=torch.Generator().manual_seed(11))
    with emu_logp.install():
        worst = lc.pool_against_oracle(_model(sd), orc, tok, sd, shp, 3e-5, **kw)
    print(f"worst |logprobs - oracle|: {worst:.3f} of 3e-5 per token")


def test_prefix_slots_and_fp8_sessions(orc, tok, tiny):
    """the option rides on the two other session forms: the same ids as without it, one value per generated event"""
    p = rc.prompts(orc, tok, (6,), seed0=610)[0]
    for base, dtype, kw, sub in ((emu_poolshare.install, torch.float32, dict(prefix_slots=2, prefix_capacity=16), dict(share_prefix=True)),
                                 (emu_kvq.install, torch.bfloat16, dict(kv_dtype="fp8"), {})):
        with emu_logp.install(base) as log:
            m = _model(tiny[1], dtype)
            out = []
            for opt in ({}, dict(logprobs=True)):
                del log[:]
                with m.decode_pool(4, 64, seeded=True, **kw, **opt) as pool:
                    ids = pool.submit(p, max_len=10, n=2, seed=[3, 4], **sub, **fc.KW)
                    fc.drain(pool)
                    out.append([pool.result(i) for i in ids])
                    if opt:
                        assert all(pool.logprobs(i).shape == (4,) and (pool.logprobs(i) < 0).all() for i in ids)
                assert ("sample_top_p_k_seeded_logp" in log) == bool(opt) and ("sample_top_p_k_seeded" in log) != bool(opt)
            assert all(fc.same(x, y) for x, y in zip(*out))


def test_eos_counts_position_zero_alone(orc, tok, tiny):
    shp, sd = tiny
    p = rc.prompts(orc, tok, (4,), seed0=620)[0]
    with emu_logp.install():
        m = _model(sd)
        arity = m._grammar()[3]
        with m.decode_pool(2, 64, seeded=True, logprobs=True) as pool:
            rid = pool.submit(p, max_len=20, seed=8, **lc.KW)
            pool.step()
            pool.step()
            # from here on the row's first-token mask allows EOS alone: the next event is EOS
            with torch.inference_mode():
                pool.ses.first_mask[0].zero_()
                pool.ses.first_mask[0, tok.eos_id] = 1
            (_, ev, done), = pool.step()
            assert done and int(ev[0]) == tok.eos_id and pool.pending() == 0
            res, lp = pool.result(rid), pool.logprobs(rid)
    assert lp.shape == (3,)
    tokens = lc.oracle_token_logp(orc, sd, shp, res, len(p))
    assert abs(float(lp[-1]) - tokens[-1, 0]) <= 3e-5, "position 0 alone"
    assert abs(float(lp[-1]) - tokens[-1, :2].sum()) > 1e-2, "... and not the pad behind it"
    want, n = lc.oracle_ll(orc, tok, sd, shp, res, len(p), arity)
    assert n[-1] == 1 and (np.abs(lp - want) <= 3e-5 * n).all()


def test_fork_hold_release_bookkeeping(orc, tok, tiny):
    shp, sd = tiny
    p, q, r = rc.prompts(orc, tok, (5, 3, 4), seed0=630)
    with emu_logp.install():
        m = _model(sd)
        arity = m._grammar()[3]
        with m.decode_pool(3, 64, seeded=True, logprobs=True) as pool:
            par = pool.submit(p, max_len=8, seed=1, hold=True, ban_eos=True, **lc.KW)
            oth = pool.submit(q, max_len=5, seed=2, ban_eos=True, **lc.KW)
            assert pool.logprobs(par).shape == (0,), "queued: nothing yet"
            pool.step()
            pool.step()
            assert pool.logprobs(par).shape == (2,) and pool.logprobs(oth).shape == (2,)
            kid, = pool.fork(par, seed=1, max_len=12)
            assert pool.logprobs(kid).shape == (0,), "the inherited events are the child's prompt"
            assert pool.requests[kid].row == 1, "the row oth left a step ago"
            pool.step()   # par holds 8 events and is held
            assert pool.held() == [par] and pool.logprobs(par).shape == (3,) and pool.logprobs(kid).shape == (1,)
            kept = pool.logprobs(par).copy()
            fc.drain(pool)
            assert pool.logprobs(kid).shape == (5,)
            late = pool.submit(r, max_len=7, seed=3, ban_eos=True, **lc.KW)
            fc.drain(pool)
            assert pool.logprobs(late).shape == (3,), "row 1 again, after oth and kid: a reused row starts empty"
            assert (pool.logprobs(par) == kept).all(), "a held request keeps its array"
            assert pool.logprobs(oth).shape == (2,)
            # the child on its parent's seed repeated the parent's third event: the same ids, the same value
            assert (pool.result(kid)[7] == pool.result(par)[7]).all() and pool.logprobs(kid)[0] == kept[2]
            pool.drop(par)
            for rid, first in ((par, 5), (oth, 3), (kid, 7), (late, 4)):
                res, lp = pool.result(rid), pool.logprobs(rid)
                want, n = lc.oracle_ll(orc, tok, sd, shp, res, first, arity)
                assert lp.shape == want.shape and (np.abs(lp - want) <= 3e-5 * n).all(), rid


def test_generate_pool_returns_pairs(orc, tok, tiny):
    shp, sd = tiny
    ps = rc.prompts(orc, tok, (4, 6, 3), seed0=640)
    reqs = [dict(prompt=p, max_len=len(p) + 3, seed=50 + k, **lc.KW) for k, p in enumerate(ps)]
    with emu_logp.install():
        m = _model(sd)
        plain = m.generate_pool(reqs, rows=2)
        pairs = m.generate_pool(reqs, rows=2, logprobs=True)
        arity = m._grammar()[3]
    assert len(pairs) == 3 and all(isinstance(x, tuple) and len(x) == 2 for x in pairs)
    for p, ev0, (ev, lp) in zip(ps, plain, pairs):
        assert fc.same(ev0, ev) and lp.dtype == np.float32 and lp.shape == (len(ev) - len(p),)
        want, n = lc.oracle_ll(orc, tok, sd, shp, ev, len(p), arity)
        assert (np.abs(lp - want) <= 3e-5 * n).all()


def test_score(orc, tok, golden):
    """-score.sum() / (non-pad targets) is the golden training loss; lengths and pad events give exact zeros"""
    shp = orc.Shape(n_layer=4, n_head=4, n_embd=256, n_inner=512, vocab=tok.vocab_size)
    sd = orc.make_state_dict(shp, seed=1)
    batch = orc.synthetic_events(tok, 2, 17, seed=2)
    batch[1, 14:] = tok.pad_id   # (the batch of tiny_train.npz: test_host_logic.py)
    g = golden("tiny_train.npz")
    with emu_logp.install() as log:
        m = _model(sd)
        del log[:]
        s = m.score(batch)
        assert s.shape == (2, 16) and s.dtype == torch.float32 and not s.requires_grad
        n = int((batch[:, 1:] != tok.pad_id).sum())
        assert abs(float(-s.double().sum() / n) - float(g["loss"])) < 3e-5
        assert (s[1, 13:] == 0).all() and (s[1, :13] < 0).all() and (s[0] < 0).all(), "pad events give exact zeros"
        assert "cross_entropy" in log and not any("bwd" in n for n in log)
        # per event against the oracle's teacher-forced ll
        arity = m._grammar()[3]
        for b, L in ((0, 17), (1, 14)):
            want, k = lc.oracle_ll(orc, tok, sd, shp, batch[b, :L].numpy(), 1, arity)
            assert (np.abs(s[b, :L - 1].double().numpy() - want) <= 3e-5 * k).all()
        cut = m.score(batch, lengths=[9, 14])
        assert (cut[0, 8:] == 0).all() and (cut[0, :8] == s[0, :8]).all() and (cut[1] == s[1]).all()
        assert (m.score(batch, lengths=[0, 1]) == 0).all()
