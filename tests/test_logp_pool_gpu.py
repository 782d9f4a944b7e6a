"""Event log-likelihoods end to end on the MI355X, production sessions with captured graphs, on the tiny 4-layer model:

  steps      a logprobs session stepped token by token: after every token step logp_rows[:, i] is within the derived bound B
             (tests/ref_logp.py) of logp64 of the session's OWN logits buffer and the id it drew -- bf16 and fp32, seeded and not;
  oracle     graph-mode pool, fp32: logprobs(rid) against the oracle's float64 teacher-forced ll, per token twice the gate
             test_model_gpu.py holds the device's lse to (rtol 1e-4, atol 1e-4): logp is a logit minus an lse;
  ids        a pool with the option returns the ids of the same pool without it, bit for bit: plain, seeded, prefix-slot and fp8;
  seeded     a request alone, and the same request in another row among neighbours: ids AND log-likelihoods bit-equal;
  score      MIDIModel.score on the golden training batch: the golden loss within 1e-4 (fp32)."""
import numpy as np
import pytest
import torch

import midi_model_amd as mm

import fork_common as fc
import logp_common as lc
import ragged_common as rc
import ref_logp as rl

pytestmark = pytest.mark.gpu

CAP = 256


@pytest.fixture(scope="module")
def tok():
    return mm.MIDITokenizerV2()


@pytest.fixture(scope="module")
def tiny(orc, tok):
    shp = orc.Shape(n_layer=4, n_head=4, n_embd=256, n_inner=512, vocab=tok.vocab_size)
    sd = orc.make_state_dict(shp, seed=0)
    made = {}

    def model(dtype):
        if dtype not in made:
            m = mm.MIDIModel(mm.MIDIModelConfig.get_config("v2", True, 4, 4, 256, 512))
            m.load_state_dict(sd, strict=True)
            made[dtype] = m.to("cuda", dtype).eval()
        return made[dtype]

    return shp, sd, model


@pytest.mark.parametrize("seeded", (False, True), ids=["noise", "seeded"])
@pytest.mark.parametrize("dtype", (torch.bfloat16, torch.float32), ids=["bf16", "fp32"])
def test_token_steps_against_the_sessions_own_logits(orc, tok, tiny, dtype, seeded):
    from midi_model_amd.decode import DecodeSession
    model = tiny[2](dtype)
    B, V, T = 3, tok.vocab_size, tok.max_token_seq
    ps = rc.prompts(orc, tok, (4, 9, 2), seed0=720)
    worst = 0.0
    with torch.inference_mode():
        ses = DecodeSession(model, B, CAP, 1.0, 0.98, 1, ragged=True, row_params=True, seeded=seeded, logprobs=True)
        assert ses.g_net is not None and ses.g_steps is not None and ses.logp_rows.shape == (B, T)
        ses.reset()
        ses.begin(None if seeded else torch.Generator(device="cuda").manual_seed(7))
        first = model._grammar()[0].cpu()[None].repeat(B, 1).contiguous()
        ses.admit([2, 0, 1], torch.cat([torch.as_tensor(p) for p in ps]), [len(p) for p in ps], [CAP - 1] * B, [0.8, 1.0, 1.5],
                  [0.9, 0.98, 1.0], [5, 20, 64], first, torch.zeros((B, V), dtype=torch.uint8), seeds=[5, 6, 7] if seeded else None)
        for _ in range(3):
            ses.draw_noise()
            ses.logp_rows.fill_(777.0)
            for i in range(T):
                ses.tok_step(i)
                z, ids, got = ses.logits.cpu(), ses.seq[:, i].cpu(), ses.logp_rows.cpu()
                assert bool((got[:, i + 1:] == 777.0).all()), "a token step wrote a column that is not its own"
                frac = (got[:, i].double() - rl.logp64(z, ids, V)).abs() / rl.bound(z, ids, V)
                worst = max(worst, float(frac.max()))
                assert bool((frac < 1).all()), (i, frac.tolist())
            ses.consumed(T)
            ses.net_step()
        ses.end()
    print(f"token steps ({dtype}, seeded={seeded}): worst {worst:.3f} of the bound")


@pytest.mark.parametrize("seeded", (False, True), ids=["noise", "seeded"])
def test_pool_logprobs_against_the_oracle_fp32(orc, tok, tiny, seeded):
    shp, sd, model = tiny
    m = model(torch.float32)
    kw = dict(seeded=True) if seeded else dict(generator=torch.Generator(device="cuda").manual_seed(11))
    worst = lc.pool_against_oracle(m, orc, tok, sd, shp, 2e-4, rel=2e-4, capacity=CAP, **kw)
    print(f"pool against the oracle (seeded={seeded}): worst {worst:.3f} of twice the lse gate")


def _requests(pool, orc, tok, seeded, **sub):
    p, q = rc.prompts(orc, tok, (7, 4), seed0=560)
    s = (lambda *v: dict(seed=list(v) if len(v) > 1 else v[0])) if seeded else (lambda *v: {})
    a, b = pool.submit(p, max_len=14, n=2, **s(1, 2), **sub, **fc.KW)
    c = pool.submit(q, max_len=9, **s(4), **fc.KW)
    for _ in range(3):
        pool.step()
    kid, = pool.fork(a, **s(9))
    fc.drain(pool)
    return [a, b, c, kid]


@pytest.mark.parametrize("form", ("plain", "seeded", "slots", "fp8"))
def test_ids_are_those_of_the_pool_without_the_option(orc, tok, tiny, form):
    m = tiny[2](torch.bfloat16)
    seeded = form != "plain"
    kw = {"slots": dict(prefix_slots=2, prefix_capacity=16), "fp8": dict(kv_dtype="fp8")}.get(form, {})
    sub = dict(share_prefix=True) if form == "slots" else {}
    out = []
    for opt in ({}, dict(logprobs=True)):
        gen = {} if seeded else dict(generator=torch.Generator(device="cuda").manual_seed(5))
        with m.decode_pool(5, CAP, seeded=seeded, **gen, **kw, **opt) as pool:
            ids = _requests(pool, orc, tok, seeded, **sub)
            out.append([pool.result(i) for i in ids])
            assert pool.ses.logprobs == bool(opt) and pool.ses.g_steps is not None
            if opt:
                for i in ids:
                    lp = pool.logprobs(i)
                    assert lp.shape == (len(pool.result(i)) - len(pool.requests[i].prompt),) and np.isfinite(lp).all() and (lp < 0).all()
    for x, y in zip(*out):
        assert fc.same(x, y), np.argwhere(x != y)[:4]


def test_seeded_request_alone_and_among_neighbours(orc, tok, tiny):
    """equal launch shapes: the same pool size, the request admitted alone both times -- into row 0 of an empty pool, and into row 2
    of a pool whose rows 0 and 1 run other requests"""
    m = tiny[2](torch.bfloat16)
    x, a, b = rc.prompts(orc, tok, (6, 9, 3), seed0=740)
    got = []
    for among in (False, True):
        with m.decode_pool(4, CAP, seeded=True, logprobs=True) as pool:
            if among:
                pool.submit(a, max_len=40, seed=21, **fc.KW)
                pool.submit(b, max_len=40, seed=22, temp=0.7, top_k=3, ban_eos=True)
                pool.step()
            rid = pool.submit(x, max_len=16, seed=77, **fc.KW)
            pool.step()
            assert pool.requests[rid].row == (2 if among else 0)
            while not pool.requests[rid].done:
                pool.step()
            got.append((pool.result(rid), pool.logprobs(rid)))
    assert fc.same(got[0][0], got[1][0])
    assert got[0][1].shape == (10,) and (got[0][1].view(np.int32) == got[1][1].view(np.int32)).all(), (got[0][1], got[1][1])


def test_score_gives_the_golden_loss(orc, tok, golden):
    shp = orc.Shape(n_layer=4, n_head=4, n_embd=256, n_inner=512, vocab=tok.vocab_size)
    sd = orc.make_state_dict(shp, seed=1)
    batch = orc.synthetic_events(tok, 2, 17, seed=2)
    batch[1, 14:] = tok.pad_id   # (the batch of tiny_train.npz: test_model_gpu.py)
    g = golden("tiny_train.npz")
    m = mm.MIDIModel(mm.MIDIModelConfig.get_config("v2", True, 4, 4, 256, 512))
    m.load_state_dict(sd, strict=True)
    m = m.to("cuda", torch.float32)
    s = m.score(batch.cuda())
    assert s.shape == (2, 16) and s.dtype == torch.float32 and s.is_cuda
    n = int((batch[:, 1:] != tok.pad_id).sum())
    assert abs(float(-s.double().sum() / n) - float(g["loss"])) < 1e-4
    assert bool((s[1, 13:] == 0).all()) and bool((s[1, :13] < 0).all()) and bool((s[0] < 0).all())
    cut = m.score(batch.cuda(), lengths=[9, 14])
    assert bool((cut[0, 8:] == 0).all()) and torch.equal(cut[0, :8], s[0, :8]) and torch.equal(cut[1], s[1])
