"""Forking inside the decode pool on the MI355X, production session: bf16 tv2o-medium with random weights, captured graphs, folded
norms, fused sampler; pools of 4 rows, capacity 256, prompts of 5 to 9 events, at most 30 events per request.  The four id-equality
properties of test_fork_host.py (tests/fork_common.py) with mh_kv_fork_rows doing the copies -- no tolerance: the copy is bit-exact
and the decode kernels treat rows independently -- and, after runs that fork, hold and drop, the same session and the same graph
objects: nothing is captured again."""
import pytest
import torch

import midi_model_amd as mm

import fork_common as fc
import ragged_common as rc

pytestmark = pytest.mark.gpu

CAP = 256


@pytest.fixture(scope="module")
def tok():
    return mm.MIDITokenizerV2()


@pytest.fixture(scope="module")
def medium_bf16(orc, tok):
    shp = orc.Shape(vocab=tok.vocab_size)
    sd = orc.make_state_dict(shp, seed=0)
    m = mm.MIDIModel(mm.MIDIModelConfig.from_name("tv2o-medium"))
    m.load_state_dict(sd, strict=True)
    return m.to("cuda", torch.bfloat16).eval()


@pytest.fixture(scope="module")
def seeded_session(orc, tok, medium_bf16):
    """the pooled seeded session of 4 rows and its graphs, made by one request that runs two events"""
    m = medium_bf16
    m._sessions.idle.clear()
    with m.decode_pool(fc.ROWS, CAP, seeded=True) as pool:
        pool.submit(rc.prompts(orc, tok, (5,), seed0=590)[0], max_len=7, seed=1)
        fc.drain(pool)
        ses = pool.ses
    assert ses.use_graphs and ses.g_net is not None and ses.g_steps is not None, "captured graphs are the production form"
    assert ses.seeded and ses.row_params and ses.fold1 is not None and ses.fused_sampler and ses.B == fc.ROWS and ses.cap == CAP
    return ses, ses.g_net, ses.g_steps


def _same_session(m, ses, got):
    s, g_net, g_steps = ses
    assert got is s and s.g_net is g_net and s.g_steps is g_steps and s.g_noise is None, "the session was replaced or recaptured"
    assert [x for x in m._sessions.idle if x.seeded] == [s], "one pooled session serves every seeded pool"


def test_a_child_repeats_its_parent(orc, tok, medium_bf16, seeded_session):
    _same_session(medium_bf16, seeded_session, fc.child_repeats_parent(medium_bf16, orc, tok, CAP))


def test_siblings_equal_lone_requests(orc, tok, medium_bf16, seeded_session):
    _same_session(medium_bf16, seeded_session, fc.siblings_equal_lone_requests(medium_bf16, orc, tok, CAP))


@pytest.mark.parametrize("alone", (False, True))
def test_a_held_request_forked_later_equals_an_uninterrupted_one(orc, tok, medium_bf16, seeded_session, alone):
    ses = fc.held_then_forked_equals_uninterrupted(medium_bf16, orc, tok, CAP, 5, alone)
    _same_session(medium_bf16, seeded_session, ses)
    assert ses.held_hidden is not None and ses.held_hidden.shape == ses.hidden.shape and ses.held_hidden.dtype == torch.bfloat16


def test_a_greedy_child_in_an_unseeded_pool(orc, tok, medium_bf16):
    m = medium_bf16
    ses = fc.greedy_child_in_an_unseeded_pool(m, orc, tok, CAP)
    assert ses.use_graphs and not ses.seeded and ses.g_noise is not None and ses.row_params
    graphs = (ses.g_net, ses.g_steps, ses.g_noise)
    assert fc.greedy_child_in_an_unseeded_pool(m, orc, tok, CAP) is ses and (ses.g_net, ses.g_steps, ses.g_noise) == graphs
