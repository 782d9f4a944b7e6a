"""The decode pool on the MI355X: requests admitted into free rows of a running batch (pool.py, DecodeSession.admit / release).
fp32 tv2o-medium against the teacher-forced oracle with two requests admitted mid-run into reused rows; on the production session
(bf16, captured graphs, folded norms, fused per-row sampler) a request's ids do not depend on its neighbours or on what its row held
before; admissions and releases recapture nothing; a pooled session serves other lengths and limits within its capacity."""
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


def test_pool_fp32_follows_the_oracle_id_for_id(orc, tok, medium_fp32):
    """two rows, the four prompts of test_generate_ragged_fp32_follows_the_oracle_id_for_id ((1, 5, 127, 130) events), each with
    max_len 140, greedy, EOS banned, submitted together: requests 2 and 3 are admitted mid-run into the rows requests 1 and 0
    leave.  Every result has 140 events behind its intact prompt; teacher-forced oracle per request, margin 1e-3, checked share
    above 0.97 of 2376 (the oracle's own greedy continuation of these inputs on the CPU reaches 2367)."""
    shp, sd, m = medium_fp32
    ps = rc.prompts(orc, tok)
    homes = {}
    with m.decode_pool(2, rc.MAX_LEN + 1) as pool:
        ids = [pool.submit(p, max_len=rc.MAX_LEN, top_k=1, ban_eos=True) for p in ps]
        while pool.pending():
            pool.step()
            for row, rid in pool.occupied.items():
                homes.setdefault(rid, row)
        out = [pool.result(i) for i in ids]
    assert homes == {0: 0, 1: 1, 2: 1, 3: 0}, "requests 2 and 3 take the rows requests 1 and 0 leave"
    checked = total = 0
    for rid, (row, p) in enumerate(zip(out, ps)):
        assert row.shape == (rc.MAX_LEN, 8) and row.dtype == np.int64 and (row[:len(p)] == p).all(), rid
        c, t = rc.oracle_argmax_check(orc, tok, sd, shp, row, len(p))
        checked, total = checked + c, total + t
    print(f"decode pool fp32 (tv2o-medium): {checked}/{total} sampling positions checked against the oracle's arg-max, all equal")
    assert total == 2376 and checked > 0.97 * total, (checked, total)


def _run_x(m, orc, tok, case):
    """request X (17 events, 24 to generate, greedy) admitted ALONE into row 3 of a 4-row pool, in three surroundings; -> (X's
    result, the session it ran on, that session's graphs before the run)"""
    x = rc.prompts(orc, tok, (17,), seed0=300)[0]
    g = torch.Generator(device="cuda").manual_seed(11)
    with m.decode_pool(4, 128, generator=g) as pool:
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
        pool.step()
        ses = pool.ses
        graphs = (ses.g_net, ses.g_steps, ses.g_noise)
        for _ in range(before - 1):
            pool.step()
        assert sorted(pool.occupied) == [0, 1, 2] and pool.free == [3], case
        rid = pool.submit(x, max_len=17 + 24, top_k=1, ban_eos=True)
        pool.step()
        assert pool.occupied[3] == rid
        while not pool.requests[rid].done:
            pool.step()
        out = pool.result(rid)
        assert pool.ses is ses
    assert out.shape == (41, 8) and (out[:17] == x).all()
    return out, ses, graphs


def test_a_request_does_not_depend_on_its_neighbours(orc, tok, medium_bf16):
    """bf16 tv2o-medium, graphs on: X's ids are IDENTICAL whatever its neighbours are and whatever its row held before -- its
    prefill is the packed forward over X alone, every kernel of the decode step is bit-equal per row, a greedy
    row does not read the noise, and cache rows at or past its position are never read.  No tolerance."""
    shp, sd, m = medium_bf16
    m._sessions.idle.clear()
    runs = [_run_x(m, orc, tok, case) for case in ("one_step", "five_steps", "reused_row")]
    (a, ses, graphs), (b, ses_b, _), (c, ses_c, _) = runs
    assert all(g is not None for g in graphs), "captured graphs are the production form"
    assert ses.fold1 is not None and ses.fused_sampler and ses.row_params
    assert (a == b).all(), np.argwhere(a != b)[:4]
    assert (a == c).all(), np.argwhere(a != c)[:4]
    # one pooled session served the three pools, and no admission or release recaptured anything
    assert ses_b is ses and ses_c is ses and m._sessions.idle == [ses]
    assert ses.g_net is graphs[0] and ses.g_steps is graphs[1], "the session was recaptured"


def test_no_recapture_and_other_lengths_within_the_capacity(orc, tok, medium_bf16):
    """a run that admits (twice, one group of three and one request alone) and releases, then a second pool of the same rows whose
    requests have other lengths and a max_len up to the capacity's last row: the same session, the same graph objects, every
    result as long as asked (EOS banned) behind its intact prompt; seeded alike, the run repeats id for id and leaves the
    generator in the same state."""
    shp, sd, m = medium_bf16
    m._sessions.idle.clear()
    ps = rc.prompts(orc, tok, (3, 40, 17, 130, 8), seed0=51)
    gens = (12, 5, 9, 20, 7)

    def run(seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        with m.decode_pool(3, 200, generator=g) as pool:
            ids = [pool.submit(p, max_len=len(p) + n, top_k=20, ban_eos=True) for p, n in zip(ps, gens)]
            pool.step()
            ses, graphs = pool.ses, (pool.ses.g_net, pool.ses.g_steps)
            while pool.pending():
                pool.step()
            assert pool.ses is ses and (ses.g_net, ses.g_steps) == graphs and pool.free == [0, 1, 2]
            assert ses.pos.tolist() == [0, 0, 0] and ses.pos_limit.tolist() == [0, 0, 0]
            return [pool.result(i) for i in ids], g, ses, graphs

    a, ga, ses, graphs = run(9)
    assert ses.cap == 256 and graphs[0] is not None and graphs[1] is not None
    for row, p, n in zip(a, ps, gens):
        assert row.shape == (len(p) + n, 8) and (row[:len(p)] == p).all()
    b, gb, ses_b, graphs_b = run(9)
    assert ses_b is ses and graphs_b[0] is graphs[0] and graphs_b[1] is graphs[1], "the session was recaptured"
    assert all((x == y).all() for x, y in zip(a, b)) and torch.equal(ga.get_state(), gb.get_state())
    # other lengths, a limit on the capacity's last row (max_len + 1 == 256), same rows: the same session
    ps2 = rc.prompts(orc, tok, (200, 2), seed0=61)
    with m.decode_pool(3, 256) as pool:
        i0 = pool.submit(ps2[0], max_len=255, top_k=1, ban_eos=True)
        i1 = pool.submit(ps2[1], max_len=30, temp=0.7, top_k=5, ban_eos=True)
        with pytest.raises(ValueError, match="capacity"):
            pool.submit(ps2[1], max_len=256)
        while pool.pending():
            pool.step()
        assert pool.ses is ses and ses.g_net is graphs[0] and ses.g_steps is graphs[1], "the session was recaptured"
        r0, r1 = pool.result(i0), pool.result(i1)
    assert r0.shape == (255, 8) and (r0[:200] == ps2[0]).all() and r1.shape == (30, 8) and (r1[:2] == ps2[1]).all()
    assert m._sessions.idle == [ses]
