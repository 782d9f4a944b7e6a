"""The decode pool on the CPU: DecodeSession.admit / release (decode.py), engine.stack_prefill_seqs(rows=...), DecodePool's
bookkeeping (pool.py) and MIDIModel.decode_pool / generate_pool with their refusals, through the row_params fake backend plus the
stand-in of mh_kv_store_seqs_rows (tests/emu_pool.py).  Tiny 4-layer model, fp32.  The kernel itself: test_pool_kernels_gpu.py; the
production session: test_pool_gpu.py."""
import numpy as np
import pytest
import torch

import midi_model_amd as mm
from midi_model_amd import engine, ops

import emu_pool
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


def _drain(pool):
    steps = 0
    while pool.pending():
        pool.step()
        steps += 1
    return steps


def test_stack_prefill_seqs_into_chosen_rows(tiny):
    """lengths (1, 5, 17) into rows (4, 1, 2) of a cache of 6 sequences: the named sequences hold exactly what the plain packed
    prefill leaves in sequences (0, 1, 2) of a cache of 3, the last hidden rows are the same, and the three unnamed sequences and
    rows >= L_s of the named ones keep their sentinel; the live cache is not grown"""
    lengths, rows, cap, sentinel = (1, 5, 17), (4, 1, 2), 32, -3.0
    with emu_pool.install() as log, torch.no_grad():
        m = _model(tiny[1])
        spec, W = m._specs["net"], m._W["net"]
        x = torch.randn((sum(lengths), spec.D), generator=torch.Generator().manual_seed(13))
        rope = engine.RopeTable(spec.hd, spec.theta, x.device, cap)
        plan = ops.attn_seq_plan(lengths, spec.H).upload(x.device)
        ref = engine.KVState(spec, 3, cap, x)
        y0 = engine.stack_prefill_seqs(spec, W, x, plan, rope, ref)
        assert "kv_store_seqs_rows" not in log
        kv = engine.KVState(spec, 6, cap, x)
        kv.k.fill_(sentinel), kv.v.fill_(sentinel)
        y1 = engine.stack_prefill_seqs(spec, W, x, plan, rope, kv, rows=rows)
        assert log.count("kv_store_seqs_rows") == spec.L and torch.equal(y0, y1) and kv.cap == cap
        for s, (r, L) in enumerate(zip(rows, lengths)):
            assert torch.equal(kv.k[:, r, :, :L], ref.k[:, s, :, :L]) and torch.equal(kv.v[:, r, :, :L], ref.v[:, s, :, :L])
            assert (kv.k[:, r, :, L:] == sentinel).all() and (kv.v[:, r, :, L:] == sentinel).all()
        for r in (0, 3, 5):
            assert (kv.k[:, r] == sentinel).all() and (kv.v[:, r] == sentinel).all()
        for bad, match in (((4, 1, 6), "outside"), ((4, 1, -1), "outside"), ((4, 1, 4), "twice"), ((4, 1), "cache rows for")):
            with pytest.raises(ValueError, match=match):
                engine.stack_prefill_seqs(spec, W, x, plan, rope, kv, rows=bad)
        with pytest.raises(ValueError, match="live cache"):
            engine.stack_prefill_seqs(spec, W, x, plan, rope, engine.KVState(spec, 6, 16, x), rows=rows)


def test_pool_fp32_follows_the_oracle(orc, tok, tiny):
    """two rows, the four prompts of the generate_ragged oracle test ((1, 5, 127, 130) events), each with max_len 140, greedy, EOS
    banned, submitted together: requests 2 and 3 are admitted mid-run into the rows requests 1 and 0 leave.  Every result has 140
    events behind its intact prompt, and the teacher-forced oracle agrees per request: the device's id is the oracle's masked
    arg-max wherever its top-2 margin exceeds 1e-3, on more than 0.95 of the 2376 positions (test_ragged_host.py's condition on
    these inputs)."""
    shp, sd = tiny
    ps = rc.prompts(orc, tok)
    with emu_pool.install():
        m = _model(sd)
        with m.decode_pool(2, rc.MAX_LEN + 1) as pool:
            ids = [pool.submit(p, max_len=rc.MAX_LEN, top_k=1, ban_eos=True) for p in ps]
            homes = {}
            while pool.pending():
                pool.step()
                for row, rid in pool.occupied.items():
                    homes.setdefault(rid, (row, sum(len(pool.requests[i].events) for i in ids)))
            out = [pool.result(i) for i in ids]
    # request 1 (135 events) leaves row 1 to request 2, request 0 (139 events) leaves row 0 to request 3: both rows are reused
    assert {rid: row for rid, (row, _) in homes.items()} == {0: 0, 1: 1, 2: 1, 3: 0}
    checked = total = 0
    for rid, (row, p) in enumerate(zip(out, ps)):
        assert row.shape == (rc.MAX_LEN, 8) and row.dtype == np.int64 and (row[:len(p)] == p).all(), rid
        c, t = rc.oracle_argmax_check(orc, tok, sd, shp, row, len(p))
        assert t == (rc.MAX_LEN - len(p)) * 8
        checked, total = checked + c, total + t
    print(f"decode pool fp32 (tiny): {checked}/{total} sampling positions checked against the oracle's arg-max, all equal")
    assert total == 2376 and checked > 0.95 * total, (checked, total)


def _run_x(m, orc, tok, case):
    """request X (17 events, 24 to generate, greedy) admitted ALONE into row 3 of a 4-row pool, in three surroundings"""
    x = rc.prompts(orc, tok, (17,), seed0=300)[0]
    with m.decode_pool(4, 128) as pool:
        if case == "one_step":       # three other requests have run one step
            for p in rc.prompts(orc, tok, (3, 9, 30), seed0=310):
                pool.submit(p, max_len=len(p) + 40, top_k=20, temp=1.2, ban_eos=True)
            before = 1
        elif case == "five_steps":   # three DIFFERENT requests have run five steps
            for p in rc.prompts(orc, tok, (12, 2, 21), seed0=320):
                pool.submit(p, max_len=len(p) + 33, top_k=1, ban_eos=True)
            before = 5
        else:                        # row 3 first hosted a longer request, which finished
            for p, n in zip(rc.prompts(orc, tok, (5, 8, 11, 40), seed0=330), (40, 40, 40, 3)):
                pool.submit(p, max_len=len(p) + n, top_k=1, ban_eos=True)
            before = 3
        for _ in range(before):
            pool.step()
        assert sorted(pool.occupied) == [0, 1, 2] and pool.free == [3], case
        rid = pool.submit(x, max_len=17 + 24, top_k=1, ban_eos=True)
        pool.step()
        assert pool.occupied[3] == rid
        while not pool.requests[rid].done:
            pool.step()
        out = pool.result(rid)
    assert out.shape == (41, 8) and (out[:17] == x).all()
    return out


def test_a_request_does_not_depend_on_its_neighbours(orc, tok, tiny):
    """X's ids are identical whatever its neighbours are and whatever its row held before: its prefill is the packed forward over
    X alone, every decode kernel treats rows independently, and cache rows at or past its position are never read"""
    with emu_pool.install():
        m = _model(tiny[1])
        a, b, c = (_run_x(m, orc, tok, case) for case in ("one_step", "five_steps", "reused_row"))
        assert len(m._sessions.idle) == 1
    assert (a == b).all() and (a == c).all()


def test_fifo_admission_and_released_rows(orc, tok, tiny):
    with emu_pool.install() as log:
        m = _model(tiny[1])
        pool = m.decode_pool(2, 64)
        del log[:]
        # an empty pool's step launches nothing and takes no session
        assert pool.step() == [] and not log and pool.ses is None and not m._sessions.idle
        ps = rc.prompts(orc, tok, (3, 6, 4), seed0=90)
        ids = [pool.submit(p, max_len=len(p) + n, top_k=1, ban_eos=True) for p, n in zip(ps, (2, 4, 3))]
        assert ids == [0, 1, 2] and not log and pool.ses is None and pool.pending() == 3
        out = pool.step()   # requests 0, 1 -> rows 0, 1 (FIFO, lowest row first); request 2 waits
        ses = pool.ses
        assert [(r, d) for r, _, d in out] == [(0, False), (1, False)] and pool.occupied == {0: 0, 1: 1} and list(pool.queue) == [2]
        assert all(e.shape == (8,) and e.dtype == np.int64 for _, e, _ in out)
        assert ses.pos.tolist() == [4, 7] and ses.pos_limit.tolist() == [5, 10]
        out = pool.step()   # request 0 holds 5 events: done, row 0 released
        assert [(r, d) for r, _, d in out] == [(0, True), (1, False)] and pool.free == [0] and pool.occupied == {1: 1}
        assert ses.pos.tolist() == [0, 8] and ses.pos_limit.tolist() == [0, 10]
        out = pool.step()   # request 2 -> row 0
        assert [(r, d) for r, _, d in out] == [(1, False), (2, False)] and pool.occupied == {1: 1, 0: 2}
        assert ses.pos.tolist() == [5, 9] and ses.pos_limit.tolist() == [7, 10]
        assert _drain(pool) == 2 and pool.free == [0, 1] and not pool.occupied
        assert ses.pos.tolist() == [0, 0] and ses.pos_limit.tolist() == [0, 0]
        res = pool.results()
        assert sorted(res) == ids and [len(res[i]) for i in ids] == [5, 10, 7]
        assert all((res[i][:len(p)] == p).all() for i, p in zip(ids, ps))
        del log[:]
        assert pool.step() == [] and not log   # drained: nothing is launched
        assert (pool.result(0, forget=True) == res[0]).all() and sorted(pool.results()) == [1, 2]
        # close() hands the session back, once
        assert not m._sessions.idle
        pool.close()
        pool.close()
        assert m._sessions.idle == [ses] and pool.ses is None
        with pytest.raises(ValueError, match="closed"):
            pool.submit(ps[0], max_len=9)
        with pytest.raises(ValueError, match="closed"):
            pool.step()
        # generate_pool: the same requests through the convenience form, on the same pooled session (capacity 64 -> 256)
        reqs = [dict(prompt=p, max_len=len(p) + n, top_k=1, ban_eos=True) for p, n in zip(ps, (2, 4, 3))]
        again = m.generate_pool(reqs, rows=2)
        assert all((a == res[i]).all() for a, i in zip(again, ids)) and m._sessions.idle == [ses]
        assert m.generate_pool([], rows=2) == []


def test_one_session_serves_every_setting_and_each_reaches_its_row_alone(orc, tok, tiny):
    V = tok.vocab_size
    chan = tok.parameter_ids["channel"]
    with emu_pool.install():
        m = _model(tiny[1])
        ps = rc.prompts(orc, tok, (2, 9, 4), seed0=50)
        with m.decode_pool(3, 40) as pool:
            pool.submit(ps[0], max_len=12, temp=0.5, top_p=0.9, top_k=5, ban_eos=True)
            pool.submit(ps[1], max_len=14, temp=1.7, top_k=64, disable_channels=[9, 0], disable_patch_change=True, ban_eos=True)
            pool.step()
            ses = pool.ses
            assert ses.row_params and ses.ragged and ses.B == 3 and ses.cap == 256
            grammar = m._grammar()[0]
            assert ses.temp_rows.tolist()[:2] == [0.5, pytest.approx(1.7)] and ses.top_k_rows.tolist()[:2] == [5, 64]
            assert ses.top_p_rows.tolist()[:2] == [pytest.approx(0.9), pytest.approx(0.98)]
            assert int(ses.first_mask[0, tok.eos_id]) == 0 and int(ses.first_mask[1, tok.eos_id]) == 0 and int(ses.first_mask[2, tok.eos_id]) == 1
            assert int(ses.first_mask[1, tok.event_ids["patch_change"]]) == 0 and int(ses.first_mask[0, tok.event_ids["patch_change"]]) == 1
            assert ses.ban.sum(1).tolist() == [0, 2, 0] and int(ses.ban[1, chan[9]]) == 1 and int(ses.ban[1, chan[0]]) == 1
            # the free row keeps what the session was built with
            assert torch.equal(ses.first_mask[2], grammar) and ses.top_k_rows.tolist()[2] == 1 and ses.pos.tolist()[2] == 0
            rows01 = [t[:2].clone() for t in (ses.temp_rows, ses.top_p_rows, ses.top_k_rows, ses.first_mask, ses.ban, ses.pos_limit)]
            ptrs = [t.data_ptr() for t in (ses.temp_rows, ses.top_p_rows, ses.top_k_rows, ses.first_mask, ses.ban, ses.pos_limit, ses.pos)]
            pool.submit(ps[2], max_len=10, temp=1.3, top_k=20, disable_control_change=True, disable_channels=[3])
            pool.step()   # admitted into row 2 alone: rows 0 and 1 keep every value
            now01 = [t[:2] for t in (ses.temp_rows, ses.top_p_rows, ses.top_k_rows, ses.first_mask, ses.ban, ses.pos_limit)]
            assert [torch.equal(a, b) for a, b in zip(rows01, now01)] == [True] * 6
            assert ses.top_k_rows.tolist()[2] == 20 and ses.ban.sum(1).tolist() == [0, 2, 1] and int(ses.ban[2, chan[3]]) == 1
            assert int(ses.first_mask[2, tok.event_ids["control_change"]]) == 0 and int(ses.first_mask[2, tok.eos_id]) == 1
            assert ses.pos_limit.tolist()[:2] == [12, 14]   # (request 2 may sample EOS: it alone is not banned from it)
            assert ptrs == [t.data_ptr() for t in (ses.temp_rows, ses.top_p_rows, ses.top_k_rows, ses.first_mask, ses.ban, ses.pos_limit, ses.pos)]
            banned = [chan[9], chan[0]]
            while pool.pending():
                for rid, ev, _ in pool.step():
                    if rid == 0:
                        assert ev[0] != tok.eos_id
                    if rid == 1:
                        assert ev[0] != tok.event_ids["patch_change"] and not np.isin(ev, banned).any()
                    if rid == 2:
                        assert ev[0] != tok.event_ids["control_change"] and chan[3] not in ev
            assert len(pool.result(0)) == 12
        # another pool of the same (rows, capacity class), other settings: the pooled session, no second DecodeSession
        assert m._sessions.idle == [ses]
        with m.decode_pool(3, 200) as pool:
            pool.submit(ps[1], max_len=150, temp=0.8, top_k=3)
            pool.step()
            assert pool.ses is ses and not m._sessions.idle
        assert m._sessions.idle == [ses] and ses.first_mask.shape == (3, V)


def test_same_seed_and_schedule_give_the_same_outputs_and_generator_state(orc, tok, tiny):
    ps = rc.prompts(orc, tok, (3, 7, 5, 2, 9), seed0=120)

    def run(seed):
        g = torch.Generator().manual_seed(seed)
        with m.decode_pool(2, 64, generator=g) as pool:
            ids = [pool.submit(p, max_len=len(p) + n, temp=1.1, top_k=20) for p, n in zip(ps[:3], (6, 3, 8))]
            for _ in range(4):
                pool.step()
            ids += [pool.submit(p, max_len=len(p) + n, temp=0.9, top_k=30) for p, n in zip(ps[3:], (5, 4))]
            _drain(pool)
            return [pool.result(i) for i in ids], g

    with emu_pool.install():
        m = _model(tiny[1])
        a, ga = run(5)
        b, gb = run(5)
        c, gc = run(6)
    assert all(x.shape == y.shape and (x == y).all() for x, y in zip(a, b)) and torch.equal(ga.get_state(), gb.get_state())
    assert not torch.equal(ga.get_state(), torch.Generator().manual_seed(5).get_state()), "the pool drew from the generator"
    assert any(x.shape != y.shape or (x != y).any() for x, y in zip(a, c)), "another seed, other draws"


def test_an_eos_event_ends_a_request_and_frees_its_row(orc, tok, tiny):
    """row 1's first-token mask is cut down to EOS after its first event: the next event is EOS, it is the request's last (as in
    generate), the row is released and the queued request takes it; the other row runs on"""
    ps = rc.prompts(orc, tok, (3, 6, 4), seed0=140)
    with emu_pool.install():
        m = _model(tiny[1])
        with m.decode_pool(2, 64) as pool:
            ids = [pool.submit(p, max_len=30, top_k=1, ban_eos=(i != 1)) for i, p in enumerate(ps)]
            pool.step()
            with torch.inference_mode():
                pool.ses.first_mask[1].zero_()
                pool.ses.first_mask[1, tok.eos_id] = 1
            out = dict((rid, (ev, done)) for rid, ev, done in pool.step())
            assert out[1][1] and out[1][0][0] == tok.eos_id and not out[0][1]
            assert pool.free == [1] and pool.ses.pos.tolist()[1] == 0 and pool.ses.pos_limit.tolist()[1] == 0
            out = pool.step()
            assert [r for r, _, _ in out] == [0, 2] and pool.occupied == {0: 0, 1: 2}
            assert int(pool.ses.first_mask[1, tok.eos_id]) == 0, "the admission overwrote the row's mask"
            _drain(pool)
            res = [pool.result(i) for i in ids]
    assert len(res[1]) == 6 + 2 and res[1][-1, 0] == tok.eos_id and [len(res[0]), len(res[2])] == [30, 30]


def test_refusals_come_before_any_backend_call(orc, tok, tiny):
    from midi_model_amd.decode import DecodeSession
    with emu_pool.install() as log:
        m = _model(tiny[1])
        del log[:]
        p = rc.prompts(orc, tok, (6,), seed0=80)[0]
        V = tok.vocab_size
        bad_id, neg = p.copy(), p.copy()
        bad_id[2, 1], neg[0, 0] = V, -1
        nan, inf = float("nan"), float("inf")
        for bad in (0, -1, 1.5):
            with pytest.raises(ValueError, match="decode_pool"):
                m.decode_pool(bad, 64)
        with pytest.raises(ValueError, match="decode_pool"):
            m.decode_pool(2, 1)
        pool = m.decode_pool(2, 64)
        for prompt, kw, match in (
                (p, dict(temp=0.0), "temperature"),
                (p, dict(temp=-1.0), "temperature"),
                (p, dict(temp=inf), "temperature"),
                (p, dict(temp=nan), "temperature"),
                (p, dict(top_p=nan), "top_p"),
                (p, dict(top_k=0), "top_k"),
                (p, dict(top_k=65), "top_k"),
                (p, dict(max_len=9.5), "not an integer"),
                (p, dict(max_len=6), "nothing to generate"),
                (p, dict(max_len=5), "nothing to generate"),
                (p, dict(max_len=64), "capacity 64"),
                (p[:0], dict(max_len=9), "shape"),
                (bad_id, dict(max_len=9), "outside"),
                (neg, dict(max_len=9), "outside"),
                (p, dict(max_len=9, disable_channels=[16]), "disable_channels"),
                (p, dict(max_len=9, disable_channels=list(range(16))), "every channel"),
                (p, dict(max_len=9, disable_channels=[[9]]), "flat sequence"),
                (p, dict(max_len=9, disable_channels=3), "flat sequence"),
                (p, dict(max_len=9, temp=[1.0]), "one value per option"),
                (p, dict(max_len=[9]), "one value per option"),
                (p, dict(max_len=9, ban_eos=True, disable_patch_change=True, disable_control_change=True), None),
        ):
            if match is None:   # (these options leave the note events: accepted)
                pool.submit(prompt, **kw)
                continue
            with pytest.raises(ValueError, match=match):
                pool.submit(prompt, **kw)
            assert not log and pool.ses is None and not m._sessions.idle, (match, log[:3])
        assert pool.pending() == 1
        with pytest.raises(ValueError, match="temperature"):
            m.generate_pool([dict(prompt=p, max_len=9), dict(prompt=p, max_len=9, temp=0.0)], rows=2)
        assert not log
        pool.close()
        assert not log and not m._sessions.idle
        # the messages are generate_ragged's own
        with pytest.raises(ValueError) as e0:
            m.generate_ragged([p], max_len=[9], top_k=[65])
        with pytest.raises(ValueError) as e1:
            m.decode_pool(2, 64).submit(p, max_len=9, top_k=65)
        assert str(e0.value) == str(e1.value)
        # admit / release: a session without row_params, and what a row_params session has no rows or cache for
        masks = torch.zeros((1, V), dtype=torch.uint8)
        toks = torch.from_numpy(p)
        with torch.inference_mode():
            plain = DecodeSession(m, 2, 64, 1.0, 0.98, 1, ragged=True)
            ses = DecodeSession(m, 2, 64, 1.0, 0.98, 1, ragged=True, row_params=True)
        del log[:]
        with pytest.raises(ValueError, match="row_params"):
            plain.admit([0], toks, [6], [9], [1.0], [0.98], [1], masks, masks)
        with pytest.raises(ValueError, match="row_params"):
            plain.release([0])
        for rows, lengths, limits, k, fm, match in (
                ([2], [6], [9], [1], masks, "outside"),
                ([-1], [6], [9], [1], masks, "outside"),
                ([0, 0], [3, 3], [9, 9], [1, 1], masks.repeat(2, 1), "twice"),
                ([0, 1], [6], [9], [1], masks, "cache rows for"),
                ([0], [5], [9], [1], masks, "summing"),
                ([0], [6], [5], [1], masks, "capacity"),
                ([0], [6], [64], [1], masks, "capacity"),
                ([0], [6], [9], [0], masks, "top_k"),
                ([0], [6], [9], [1], masks[:, :-1], "uint8"),
                ([0], [6], [9], [1], masks.long(), "uint8"),
        ):
            n = len(lengths)
            with pytest.raises(ValueError, match=match):
                ses.admit(rows, toks, lengths, limits, [1.0] * n, [0.98] * n, k, fm, masks.repeat(n, 1))
        with pytest.raises(ValueError, match="outside"):
            ses.release([2])
        assert not log
