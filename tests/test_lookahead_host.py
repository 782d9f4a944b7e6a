"""Lookahead decoding in the decode pool on the CPU: DecodePool(lookahead=k) (pool.py), DecodeSession(lookahead=k) (decode.py),
engine.stack_decode(row_cache=...) and the wrappers of ops_lookahead.py, through the fake backend plus the stand-ins of
mh_kv_append_rows_via / mh_attn_decode_rows_via (tests/emu_lookahead.py).  Tiny 4-layer model, fp32.  The kernels themselves:
test_lookahead_kernels_gpu.py; the production session: test_lookahead_pool_gpu.py."""
import numpy as np
import pytest
import torch

import midi_model_amd as mm
from midi_model_amd.pool import DecodePool, propose_ngram

import emu_fork
import emu_logp
import emu_lookahead
import fork_common as fc
import lookahead_common as lk
import ragged_common as rc

VIA = ("kv_append_rows_via", "attn_decode_rows_via")


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


def _ev(*toks):
    e = np.zeros(8, dtype=np.int64)
    e[:len(toks)] = toks
    return e


# ---------------------------------------------------------------------------------------------------------------- construction
def test_refusals_come_before_any_backend_call(orc, tok, tiny):
    """at least this one fails without the feature: decode_pool(..., lookahead=2) was a TypeError"""
    from midi_model_amd import engine, ops
    from midi_model_amd.decode import DecodeSession
    with emu_lookahead.install() as log:
        m = _model(tiny[1])
        del log[:]
        pool = m.decode_pool(2, 64, seeded=True, lookahead=2)
        assert pool.lookahead == 2 and pool.rows == 2 and pool.ses is None and pool.proposer is propose_ngram
        pool.close()
        for kw, match in ((dict(lookahead=2), "seeded=True"),
                          (dict(lookahead=2, generator=torch.Generator()), "seeded=True"),
                          (dict(seeded=True, lookahead=2, prefix_slots=1, prefix_capacity=16), "prefix_slots, kv_dtype or lora_slots"),
                          (dict(seeded=True, lookahead=2, lora_slots=4, lora_rank=64), "prefix_slots, kv_dtype or lora_slots"),
                          (dict(seeded=True, lookahead=0), "k >= 1"), (dict(seeded=True, lookahead=-1), "k >= 1"),
                          (dict(seeded=True, lookahead=True), "k >= 1"), (dict(seeded=True, lookahead=1.0), "k >= 1")):
            with pytest.raises(ValueError, match=match):
                m.decode_pool(2, 64, **kw)
        with pytest.raises(ValueError, match="kv_dtype"):   # (whichever of the two refusals of this pair comes first)
            m.decode_pool(2, 64, seeded=True, lookahead=2, kv_dtype="fp8")
        for rows, k in ((65, 3), (129, 1), (2, 128), (256, 1)):
            with pytest.raises(ValueError, match="at most 256"):
                m.decode_pool(rows, 64, seeded=True, lookahead=k)
        m.decode_pool(64, 64, seeded=True, lookahead=3).close()   # 256 rows: allowed
        with pytest.raises(ValueError, match="seeded=True"):
            m.generate_pool([dict(prompt=None, max_len=4)], rows=1, lookahead=2)
        # ---- the session and its key
        for kw, match in ((dict(ragged=True, row_params=True), "seeded"), (dict(), "seeded"),
                          (dict(ragged=True, row_params=True, seeded=True, kv_dtype="fp8"), "not available"),
                          (dict(ragged=True, row_params=True, seeded=True, prefix_slots=1, prefix_capacity=8), "not available"),
                          (dict(ragged=True, row_params=True, seeded=True, lora_slots=4, lora_rank=64), "not available")):
            with pytest.raises(ValueError, match=match):
                DecodeSession.make_key(m, 6, 64, 1.0, 0.98, 1, lookahead=2, **kw)
        for B, k, match in ((7, 2, "whole groups"), (260, 1, "at most"), (6, 0.5, "integer"), (6, True, "integer"), (6, -2, "integer")):
            with pytest.raises(ValueError, match=match):
                DecodeSession.make_key(m, B, 64, 1.0, 0.98, 1, ragged=True, row_params=True, seeded=True, lookahead=k)
        assert not log
        # ---- stack_decode: every other form refuses the row map before any launch
        with torch.inference_mode():
            ses = DecodeSession(m, 6, 64, 1.0, 0.98, 1, ragged=True, row_params=True, seeded=True, lookahead=2)
            plain = DecodeSession(m, 6, 64, 1.0, 0.98, 1, ragged=True, row_params=True, seeded=True)
            assert ses.kv1.B == 2 and ses.kv2.B == 6 and ses.row_cache.tolist() == [-1] * 6 and plain.row_cache is None
            del log[:]
            spec, W = m._specs["net"], m._W["net"]
            x = torch.zeros((6, spec.D))
            rc32 = torch.zeros(6, dtype=torch.int32)
            for kw in (dict(), dict(pos_dev=rc32[:1]), dict(row_pos=rc32, shared=("kvp", rc32, None))):
                with pytest.raises(ValueError, match="row map"):
                    engine.stack_decode(spec, W, x, ses.rope1, ses.kv1, row_cache=rc32, **kw)
            with pytest.raises(ValueError, match="not a lookahead session"):
                plain.set_inputs([0], np.zeros((1, 8)), [0], [0])
            for call in (lambda: ses.prefill(torch.zeros((6, 2, 8), dtype=torch.long)),
                         lambda: ses.prefill_ragged(torch.zeros((12, 8), dtype=torch.long), [2] * 6)):
                with pytest.raises(ValueError, match="admit"):
                    call()
            ev = np.zeros((2, 8), dtype=np.int64)
            for rows, e, pos, cache, match in (([0, 6], ev, [0, 0], [0, 0], "outside"), ([0, 1], ev, [0], [0, 0], "positions"),
                                               ([0, 1], ev, [3, 3], [0, 0], "one position"), ([0, 3], ev, [3, 3], [0, 0], "own group"),
                                               ([0, 1], ev, [3, 64], [0, 0], "capacity"), ([0, 1], ev, [3, -1], [0, 0], "capacity"),
                                               ([0, 1], ev - 1, [3, 4], [0, 0], "token id")):
                with pytest.raises(ValueError, match=match):
                    ses.set_inputs(rows, e, pos, cache)
            ses.set_inputs([0, 1, 2], np.zeros((3, 8), dtype=np.int64), [3, 3, 3], [0, -1, -1])   # inactive rows stand anywhere
            assert ses.pos.tolist()[:3] == [3, 3, 3] and ses.row_cache.tolist() == [0, -1, -1, -1, -1, -1]
            assert not any(n in VIA for n in log)
            # ---- the wrappers' own checks (the real ones: they refuse before lib().call)
            from midi_model_amd import ops_lookahead as ol
            q, kc, o = torch.zeros((3, 3 * 128)), torch.zeros((2, 2, 16, 64)), torch.zeros((3, 128))
            pos = torch.zeros(3, dtype=torch.int32)
            for args, match in (((q, None, None, kc, kc, 3, 2, 64, 16, pos, None), "row_cache"),
                                ((q, None, None, kc, kc, 3, 2, 64, 16, pos.long(), pos), "row_pos"),
                                ((q, None, None, kc, kc, 3, 2, 64, 16, pos, pos[:2]), "row_cache"),
                                ((q, None, None, kc[0], kc[0], 3, 2, 64, 16, pos, pos), "whole sequences"),
                                ((q, None, None, kc, kc.double(), 3, 2, 64, 16, pos, pos), "whole sequences"),
                                ((q[:, :-1], None, None, kc, kc, 3, 2, 64, 16, pos, pos), "qkv")):
                with pytest.raises(ValueError, match=match):
                    ol.kv_append_rows_via(*args)
            with pytest.raises(ValueError, match="o \\["):
                ol.attn_decode_rows_via(q, kc, kc, o[:2], 3, 2, 64, 16, 0.125, pos, pos)
            assert ops.kv_append_rows_via is not ol.kv_append_rows_via, "the stand-in is installed"


def test_session_key_rules(tiny):
    from midi_model_amd.decode import DecodeSession
    m = _model(tiny[1])
    base = (m._flat.data_ptr(), m._flat.dtype)
    mk = DecodeSession.make_key
    # no existing key changes
    assert mk(m, 6, 64, 1.0, 0.98, 1) == base + (6, 64, 1.0, 0.98, 1)
    assert mk(m, 6, 64, 1.0, 0.98, 1, 0, True, True) == base + (6, 64, ("ragged", "row_params"))
    seeded = mk(m, 6, 64, 1.0, 0.98, 1, 0, True, True, True)
    assert seeded == base + (6, 64, ("ragged", "row_params", "seeded"))
    assert mk(m, 6, 64, 1.0, 0.98, 1, 0, True, True, True, logprobs=True) == base + (6, 64, ("ragged", "row_params", "seeded", ("logp",)))
    # the new form: its own key, the option at the end
    k2 = mk(m, 6, 64, 1.0, 0.98, 1, 0, True, True, True, lookahead=2)
    assert k2 == base + (6, 64, ("ragged", "row_params", "seeded", ("lookahead", 2)))
    assert mk(m, 6, 64, 1.0, 0.98, 1, 0, True, True, True, lookahead=1) != k2 != seeded
    assert mk(m, 6, 64, 1.0, 0.98, 1, 0, True, True, True, logprobs=True, lookahead=2) == \
        base + (6, 64, ("ragged", "row_params", "seeded", ("logp",), ("lookahead", 2)))
    assert mk(m, 6, 64, 1.0, 0.98, 1, 0, True, True, True, lookahead=0) == seeded


def test_a_plain_pool_logs_what_it_logged_and_a_lookahead_step_is_the_pair(orc, tok, tiny):
    p, q = rc.prompts(orc, tok, (7, 4), seed0=560)

    def plain(m):
        with m.decode_pool(3, 64, seeded=True) as pool:
            ids = [pool.submit(x, max_len=len(x) + n, seed=s, **fc.KW) for x, n, s in ((p, 5, 1), (q, 3, 2), (p, 4, 3), (q, 6, 4))]
            fc.drain(pool)
            assert pool.ses.lookahead == 0 and pool.ses.row_cache is None and pool.ses.kv1.B == 3
            return [pool.result(i) for i in ids]

    with emu_fork.install() as log0:
        m = _model(tiny[1])
        del log0[:]
        a, la = plain(m), list(log0)
    with emu_lookahead.install() as log:
        m = _model(tiny[1])
        del log[:]
        b, lb = plain(m), list(log)
        assert la == lb and not any(n in VIA for n in lb) and all(fc.same(x, y) for x, y in zip(a, b))
        # a lookahead pool: the net step's attention is the pair, once per layer, and the per-row forms are not called
        with m.decode_pool(2, 64, seeded=True, lookahead=2) as pool:
            pool.submit(p, max_len=20, seed=1, **fc.KW)
            pool.step()
            del log[:]
            pool.step()
            step = list(log)
        layers = len(m._W["net"].layers)
        assert step.count(VIA[0]) == layers and step.count(VIA[1]) == layers
        assert [n for n in step if n in VIA] == list(VIA) * layers, "the append completes before the attention of its layer"
        assert not any(n in ("kv_append_rows", "attn_decode_rows", "attn_decode_append_rows") for n in step)


# ---------------------------------------------------------------------------------------------------------------- bookkeeping
def test_group_bookkeeping(orc, tok, tiny):
    """admit, release, fork, hold, drop and n=k siblings, in units of groups: R = 3 requests of k + 1 = 3 rows"""
    p, q = rc.prompts(orc, tok, (4, 6), seed0=570)
    none = lambda h, k: np.zeros((0, 8), dtype=np.int64)   # noqa: E731
    with emu_lookahead.install():
        m = _model(tiny[1])
        with m.decode_pool(3, 64, seeded=True, lookahead=2) as pool:
            pool.proposer = none
            a = pool.submit(p, max_len=7, seed=1, hold=True, **fc.KW)      # 3 events, then held in group 0
            b = pool.submit(q, max_len=30, seed=2, **fc.KW)                # group 1
            pool.step()
            ses = pool.ses
            assert ses.B == 9 and ses.groups == 3 and ses.kv1.B == 3 and ses.kv2.B == 9 and ses.key[-1][-1] == ("lookahead", 2)
            assert pool.occupied == {0: a, 1: b} and pool.free == [2]
            assert ses.row_cache.tolist() == [0, -1, -1, 1, -1, -1, -1, -1, -1]
            assert ses.pos.tolist()[0::3] == [5, 7, 0] and ses.pos_limit.tolist() == [7] * 3 + [30] * 3 + [0] * 3
            # the draft rows carry their leader's settings
            for buf in (ses.temp_rows, ses.top_p_rows, ses.top_k_rows, ses.seed_rows, ses.first_mask, ses.ban):
                for g in (0, 1):
                    assert all(torch.equal(buf[3 * g], buf[3 * g + j]) for j in (1, 2))
            assert ses.seed_rows.tolist()[:6] == [1, 1, 1, 2, 2, 2]
            # a sibling group of two does not fit one free group: it waits whole
            g = pool.submit(q, max_len=12, seed=[5, 6], n=2, **fc.KW)
            pool.step()
            assert list(pool.queue) == g and pool.free == [2]
            out = pool.step()   # a reaches max_len 7: held, its group is kept
            assert [(r, d) for r, _, d in out] == [(a, True), (b, False)]
            assert pool.held() == [a] and pool.held_rows == {0: a} and pool.free == [2] and pool.pending() == 3
            assert ses.pos.tolist()[0] == 7 and ses.row_cache.tolist()[:3] == [0, -1, -1]
            pool.step()
            assert ses.pos.tolist()[0] == 7, "a held leader stays parked at its max_len"
            child, = pool.fork(a, max_len=10, seed=1)   # the lowest free GROUP, ahead of the queue
            assert pool.occupied == {1: b, 2: child} and pool.free == [] and ses.row_cache.tolist()[6:] == [2, -1, -1]
            assert ses.pos.tolist()[6] == 7 and ses.pos_limit.tolist()[6:] == [10] * 3 and ses.seed_rows.tolist()[6:] == [1] * 3
            with pytest.raises(ValueError, match="0 are free"):
                pool.fork(a, max_len=10, seed=1)
            for _ in range(3):
                pool.step()
            assert pool.requests[child].done and pool.free == [2] and ses.row_cache.tolist()[6:] == [-1] * 3
            assert ses.pos.tolist()[6:] == [0] * 3 and ses.pos_limit.tolist()[6:] == [0] * 3
            assert len(pool.result(child)) == 10 and (pool.result(child)[:7] == pool.result(a)).all()
            pool.drop(a)
            assert pool.held() == [] and pool.free == [0, 2] and ses.row_cache.tolist()[:3] == [-1] * 3
            pool.step()   # the sibling group goes in whole: groups 0 and 2, one prefill and one fork
            assert pool.occupied == {1: b, 0: g[0], 2: g[1]} and ses.row_cache.tolist() == [0, -1, -1, 1, -1, -1, 2, -1, -1]
            assert ses.seed_rows.tolist() == [5] * 3 + [2] * 3 + [6] * 3
            fc.drain(pool)
            assert all(len(pool.result(i)) <= 12 for i in g) and pool.free == [0, 1, 2]
            assert ses.row_cache.tolist() == [-1] * 9


# ---------------------------------------------------------------------------------------------------------------- acceptance
def test_the_acceptance_rule():
    EOS, k = 2, 3
    s = np.stack([_ev(10 + j, 1, 2, 3, 4, 5, 6, 7) for j in range(k + 1)])
    acc = DecodePool.accept
    none = s[:0]
    assert acc(s, none, 5, 40, EOS) == 1, "no drafts: m = 0"
    wrong = s[:3] + 1
    assert acc(s, wrong, 5, 40, EOS) == 1, "m = 0"
    assert acc(s, s[:3], 5, 40, EOS) == 4, "m = k"
    assert acc(s, s[:2], 5, 40, EOS) == 3, "fewer drafts than rows"
    d = s[:3].copy()
    d[1, 7] += 1
    assert acc(s, d, 5, 40, EOS) == 2, "a mismatch in token 7 only"
    d = s[:3].copy()
    d[0, 7] += 1
    assert acc(s, d, 5, 40, EOS) == 1, "... of the first draft: what lies behind it is dropped although it matches"
    e = s.copy()
    e[1] = _ev(EOS)
    assert acc(e, e[:3], 5, 40, EOS) == 2, "EOS as s_1 with a matching draft behind it"
    e = s.copy()
    e[0] = _ev(EOS)
    assert acc(e, e[:3], 5, 40, EOS) == 1
    assert acc(s, s[:3], 37, 40, EOS) == 3, "a run crossing max_len: events 37, 38, 39 and no more"
    assert acc(s, s[:3], 39, 40, EOS) == 1 and acc(s, s[:3], 36, 40, EOS) == 4


def test_step_reports_an_accepted_run_in_order(orc, tok, tiny):
    """scripted sampler outputs through step(): a request id several times in one step, done on the last alone, EOS inside a run,
    max_len inside a run"""
    p = rc.prompts(orc, tok, (4,), seed0=575)[0]
    EOS = tok.eos_id
    with emu_lookahead.install():
        m = _model(tiny[1])
        ids0 = [t for t in range(tok.vocab_size) if t not in (EOS, tok.pad_id)][:12]
        S = [_ev(ids0[j], 1, 2, 3, 4, 5, 6, 7) for j in range(12)]
        script = []

        def scripted(ses):
            def sample_event(then_net=False, live=None):
                assert then_net is False
                out = np.zeros((ses.B, 8), dtype=np.int64)
                rows = script.pop(0)
                out[:len(rows)] = rows
                ses.last_logp = np.zeros((ses.B, 8), dtype=np.float32)
                return out, False
            return sample_event

        with m.decode_pool(1, 64, seeded=True, lookahead=3) as pool:
            drafts = []
            pool.proposer = lambda h, k: np.stack(drafts.pop(0))
            rid = pool.submit(p, max_len=4 + 9, seed=1, **fc.KW)
            with torch.inference_mode():
                ses = pool._session()
            ses.sample_event = scripted(ses)
            try:
                # step 1: nothing was drafted before the admission: m = 0
                script.append([S[0], S[9], S[9], S[9]])
                drafts.append([S[1], S[2], S[3]])
                assert [(r, int(e[0]), d) for r, e, d in pool.step()] == [(rid, ids0[0], False)]
                assert pool.ses.pos.tolist() == [5, 6, 7, 8] and pool.ses.row_cache.tolist() == [0, 0, 0, 0]
                # step 2: m = k
                script.append([S[1], S[2], S[3], S[4]])
                drafts.append([S[5], S[6][:7].tolist() + [0], S[7]])
                assert [(r, int(e[0]), d) for r, e, d in pool.step()] == [(rid, ids0[j], False) for j in (1, 2, 3, 4)]
                assert pool.ses.pos.tolist() == [9, 10, 11, 12]
                # step 3: a mismatch in token 7 of the second draft: m = 1; the third row's sample is dropped though its draft matched
                script.append([S[5], S[6], S[7], S[8]])
                drafts.append([S[7], S[8]])
                assert [int(e[0]) for _, e, _ in pool.step()] == [ids0[5], ids0[6]]
                assert len(pool.result(rid)) == 4 + 7 and pool.ses.pos.tolist() == [11, 12, 1, 1]
                assert pool.ses.row_cache.tolist() == [0, 0, -1, -1], "two events are left: one draft row can still sample below max_len"
                # step 4: max_len inside the run
                script.append([S[7], S[8], S[9], S[9]])
                assert [(int(e[0]), d) for _, e, d in pool.step()] == [(ids0[7], False), (ids0[8], True)]
                assert pool.requests[rid].done and not pool.requests[rid].eos and len(pool.result(rid)) == 13 and pool.free == [0]
                # EOS as s_1 with a matching draft behind it
                rid = pool.submit(p, max_len=40, seed=1, **fc.KW)
                script.append([S[0], S[9], S[9], S[9]])
                drafts.append([_ev(EOS), S[2], S[3]])
                pool.step()
                script.append([_ev(EOS), S[2], S[3], S[4]])
                assert [(int(e[0]), d) for _, e, d in pool.step()] == [(EOS, True)]
                rid = pool.submit(p, max_len=40, seed=1, **fc.KW)
                script.append([S[0], S[9], S[9], S[9]])
                drafts.append([S[1], _ev(EOS), S[3]])
                pool.step()
                script.append([S[1], _ev(EOS), S[3], S[4]])
                assert [(int(e[0]), d) for _, e, d in pool.step()] == [(ids0[1], False), (EOS, True)]
                assert pool.requests[rid].eos and len(pool.result(rid)) == 4 + 3 and not script and not drafts
                # a proposer that returns something that is no guess: refused in step(), before the scatter
                pool.submit(p, max_len=40, seed=1, **fc.KW)
                for bad in (np.zeros((4, 8), dtype=np.int64), np.zeros((2, 7), dtype=np.int64), np.zeros((1, 8)),
                            np.full((1, 8), tok.vocab_size), np.full((1, 8), -1)):
                    pool.proposer = lambda h, k, bad=bad: bad
                    script.append([S[0], S[9], S[9], S[9]])
                    with pytest.raises(ValueError, match="proposer"):
                        pool.step()
                    r = pool.requests[max(pool.requests)]
                    assert not r.events and not r.done and len(r.drafts) == 0, "a refused step leaves the request as it was"
            finally:
                del pool.ses.sample_event


# ---------------------------------------------------------------------------------------------------------------- the proposer
def test_the_built_in_proposer():
    A, B, C, D, E = (_ev(10 + j, j, j, j) for j in range(5))
    empty = lambda d: d.shape == (0, 8) and d.dtype == np.int64   # noqa: E731
    loop = np.stack([D, A, B, C, A, B, C, A, B, C])   # a loop of period 3
    d = propose_ngram(loop, 7)
    assert d.dtype == np.int64 and (d == np.stack([A, B, C])).all(), "the most recent earlier occurrence, and what followed it"
    assert (propose_ngram(loop, 2) == np.stack([A, B])).all()
    assert (propose_ngram(loop[:-1], 3) == np.stack([C, A, B])).all()
    assert empty(propose_ngram(np.stack([A, B, C, D, E]), 3)), "no match"
    assert empty(propose_ngram(np.stack([A, B, A, C, E, B]), 3)), "a single event that repeats is no match"
    # n = 3 fails, n = 2 matches; the continuation is shorter than k
    h = np.stack([E, B, C, D, A, B, C])
    assert (propose_ngram(h, 3) == np.stack([D, A, B])).all()
    assert (propose_ngram(np.stack([D, E, B, C, A, B, C]), 5) == np.stack([A, B, C])).all(), "shorter than k"
    assert (propose_ngram(np.stack([A, A, A]), 3) == np.stack([A])).all(), "n = 2 on a history of 3: the overlap is allowed"
    # a history shorter than n
    assert empty(propose_ngram(np.stack([A, A]), 3)) and empty(propose_ngram(np.stack([A]), 3)) and empty(propose_ngram(np.zeros((0, 8), dtype=np.int64), 3))
    # equality is over all 8 tokens
    A7 = A.copy()
    A7[7] = 99
    assert empty(propose_ngram(np.stack([A7, B, C, A, B, E, A, B]), 3)) is False   # (A, B) matches at n = 2
    assert empty(propose_ngram(np.stack([A7, B, E, A, B]), 3)), "token 7 differs: (A7, B) is not (A, B)"
    out = propose_ngram(loop, 3)
    out[:] = 0
    assert (loop[1] == A).all(), "the guess is a copy"


# ---------------------------------------------------------------------------------------------------------------- the promise
def test_ids_and_logprobs_do_not_depend_on_the_drafts(orc, tok, tiny):
    with emu_logp.install(base=emu_lookahead.install):
        m = _model(tiny[1])
        lk.drafts_do_not_matter(m, orc, tok, 64, rows=2, k=3)


def test_a_held_request_forked_later_equals_an_uninterrupted_one(orc, tok, tiny):
    with emu_logp.install(base=emu_lookahead.install):
        m = _model(tiny[1])
        lk.held_then_forked_equals_uninterrupted(m, orc, tok, 64, rows=3, k=3)
