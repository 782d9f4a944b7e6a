"""Lookahead decoding in the decode pool, end to end on the MI355X: production sessions with captured graphs, bf16, the tiny 4-layer
model of test_lora_pool_gpu.py (I = 1024, so that both stacks run the fused folded form), R = 2 and 3 requests of k + 1 = 4 rows,
prompts of 5 to 20 events, max_len at most 40.

The promise under test (pool.py, "LOOKAHEAD"): a request's ids and log-likelihoods do not depend on what the drafts were.  Five runs of
the same requests (tests/lookahead_common.py) -- the proposer returning nothing (recorded), the recorded continuation, wrong events,
right for two events then wrong, the built-in n-gram proposer -- must give bit-equal ``result()`` and ``logprobs()``.  The set holds a
request that ends on EOS before its max_len (seed lookahead_common.EOS_SEED, asserted), one that reaches max_len in the middle of a
run of k + 1, an ``n=2`` sibling submit and (R = 3) a ``hold=True`` request forked afterwards with a larger max_len, which must equal
the uninterrupted request in the same pool shape.

Step counts asserted with the oracle proposer: a request admitted in step 1 that generates E events takes exactly
1 + ceil((E - 1) / (k + 1)) ``step()`` calls -- the admitting step samples one event, since nothing was drafted before the prefill,
and every later step k + 1 -- and a wave of requests takes the largest of those (``lookahead_common.steps_of``)."""
import numpy as np
import pytest
import torch

import midi_model_amd as mm

import fork_common as fc
import lookahead_common as lk
import ragged_common as rc

pytestmark = pytest.mark.gpu

CAP, K = 256, 3


@pytest.fixture(scope="module")
def tok():
    return mm.MIDITokenizerV2()


@pytest.fixture(scope="module")
def model(orc, tok):
    shp = orc.Shape(n_layer=4, n_head=4, n_embd=256, n_inner=1024, vocab=tok.vocab_size)
    sd = {k: v.to(torch.bfloat16).float() for k, v in orc.make_state_dict(shp, seed=0).items()}
    m = mm.MIDIModel(mm.MIDIModelConfig.get_config("v2", True, 4, 4, 256, 1024))
    m.load_state_dict(sd, strict=True)
    return m.to("cuda", torch.bfloat16).eval()


@pytest.mark.parametrize("rows", [2, 3])
def test_ids_and_logprobs_do_not_depend_on_the_drafts(orc, tok, model, rows):
    gen = lk.drafts_do_not_matter(model, orc, tok, CAP, rows=rows, k=K)
    ses = model._sessions.idle[-1]
    assert ses.lookahead == K and ses.B == rows * (K + 1) and ses.kv1.B == rows and ses.g_net is not None and ses.g_steps is not None
    assert ses.fold1 is not None, "the fused folded form"
    print(f"rows {rows}: generated events per request {gen}")


def test_a_held_request_forked_later_equals_an_uninterrupted_one(orc, tok, model):
    lk.held_then_forked_equals_uninterrupted(model, orc, tok, CAP, rows=3, k=K)


def test_one_request_alone_takes_the_stated_number_of_steps(orc, tok, model):
    """one request, every guess right: 1 + ceil((E - 1) / (k + 1)) steps for E = 1 .. 10 generated events; no guess: E steps; the
    ids are the same; nothing is recaptured between the runs (one pooled session serves them all)"""
    p = rc.prompts(orc, tok, (7,), seed0=940)[0]
    kw = dict(seed=5, ban_eos=True, **lk.KW)
    with model.decode_pool(2, CAP, seeded=True, lookahead=K) as pool:
        pool.proposer = lk._none
        rid = pool.submit(p, max_len=7 + 10, **kw)
        fc.drain(pool)
        rec, ses, graphs = pool.result(rid), pool.ses, (pool.ses.g_net, pool.ses.g_steps)
        assert pool.steps == 10
    for E in range(1, 11):
        with model.decode_pool(2, CAP, seeded=True, lookahead=K) as pool:
            pool.proposer = lk.oracle_of([rec], tok.vocab_size)
            rid = pool.submit(p, max_len=7 + E, **kw)
            fc.drain(pool)
            assert pool.ses is ses and (ses.g_net, ses.g_steps) == graphs
            assert fc.same(pool.result(rid), rec[:7 + E]), E
            assert pool.steps == lk.steps_of(E, K) == 1 + -(-(E - 1) // (K + 1)), (E, pool.steps)


def test_generate_pool_takes_the_option(orc, tok, model):
    ps = rc.prompts(orc, tok, (6, 11, 8), seed0=950)
    reqs = [dict(prompt=p, max_len=len(p) + 9, seed=60 + i, ban_eos=True, **lk.KW) for i, p in enumerate(ps)]
    a = model.generate_pool(reqs, rows=3, capacity=CAP, lookahead=K)
    with model.decode_pool(3, CAP, seeded=True, lookahead=K) as pool:
        pool.proposer = lk._none
        ids = [pool.submit(**r) for r in reqs]
        fc.drain(pool)
        b = [pool.result(i) for i in ids]
    assert all(fc.same(x, y) and len(x) == len(p) + 9 for x, y, p in zip(a, b, ps))
    assert isinstance(a[0], np.ndarray)
