"""Prefix slots inside the decode pool on the MI355X, production session (captured graphs, folded norms, fused sampler): pools of 8
rows, prompts of 5, 256 and 300 events (one ragged chunk of the prefix kernel, one full chunk, two), at most 12 events generated per
request.  fp32 tv2o-medium: a greedy sharing group follows the CPU oracle id for id, by the acceptance rule of
test_shared_prompt_gpu.py.  bf16 tv2o-medium, seeded pools: the id-equality properties of tests/poolshare_common.py with the two slot
kernels in the net graph -- no tolerance: per row the kernels are bit-equal whatever else shares a slot or a query tile
(test_poolshare_kernels_gpu.py) -- and, after runs that admit, fork, hold, drop and free slots, the same session and the same graph
objects: nothing is captured again."""
import pytest
import torch

import poolshare_common as pc
from test_shared_prompt_gpu import PROMPT_SEED, _oracle_argmax_check, medium, medium_fp32, tok  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

ROWS, CAP = 8, 512
SLOTS = dict(prefix_slots=2, prefix_capacity=300)
LENGTHS = (5, 256, 300)


@pytest.fixture(scope="module")
def medium_bf16(medium):
    import copy
    return copy.deepcopy(medium[2]).to("cuda", torch.bfloat16).eval()


@pytest.fixture(scope="module")
def slots_session(orc, tok, medium_bf16):
    """the pooled seeded session of 8 rows with 2 prefix slots of 512 events, and its graphs, made by one sharing request"""
    import ragged_common as rc
    m = medium_bf16
    m._sessions.idle.clear()
    with m.decode_pool(ROWS, CAP, seeded=True, **SLOTS) as pool:
        pool.submit(rc.prompts(orc, tok, (5,), seed0=590)[0], max_len=7, seed=1, share_prefix=True)
        pc.drain(pool)
        ses = pool.ses
    assert ses.use_graphs and ses.g_net is not None and ses.g_steps is not None, "captured graphs are the production form"
    assert ses.seeded and ses.row_params and ses.fold1 is not None and ses.fused_sampler and ses.B == ROWS and ses.cap == CAP
    assert ses.prefix_slots == 2 and ses.prefix_capacity == 512 and ses.kvs.k.shape[1:] == (2, 16, 512, 64)
    return ses, ses.g_net, ses.g_steps


def _same_session(m, ses, got):
    s, g_net, g_steps = ses
    assert got is s and s.g_net is g_net and s.g_steps is g_steps and s.g_noise is None, "the session was replaced or recaptured"
    assert [x for x in m._sessions.idle if x.kvs is not None] == [s], "one pooled session serves every pool with these slots"


@pytest.mark.parametrize("P", LENGTHS)
def test_a_greedy_sharing_group_follows_the_oracle_fp32(orc, tok, medium_fp32, P):
    """fp32 tv2o-medium, an unseeded pool of 8 rows with slots: submit(n=3, share_prefix=True, top_k=1, ban_eos=True) behind a prompt
    of P events, 12 events generated.  The rule of test_generate_share_prompt_fp32_follows_the_oracle_id_for_id: teacher-forced
    oracle, margin 1e-3, every checked position equal, checked share > 0.97."""
    import numpy as np
    shp, sd, m = medium_fp32
    prompt = orc.synthetic_events(tok, 1, P, seed=PROMPT_SEED)[0].numpy()
    with m.decode_pool(ROWS, CAP, generator=torch.Generator(device="cuda").manual_seed(3), **SLOTS) as pool:
        ids = pool.submit(prompt, max_len=P + 12, top_k=1, ban_eos=True, n=3, share_prefix=True)
        pool.step()
        ses = pool.ses
        assert ses.slot_refs == [3, 0] and ses.slot_len.tolist() == [P, 0] and ses.row_slot.tolist() == [0, 0, 0] + [-1] * 5
        pc.drain(pool)
        out = np.stack([pool.result(i) for i in ids])
    assert out.shape == (3, P + 12, 8) and (out[:, :P] == prompt[None]).all() and (out[0] == out[1]).all() and (out[0] == out[2]).all()
    checked, total = _oracle_argmax_check(orc, tok, sd, shp, out, P)
    print(f"sharing group behind {P} events: {checked}/{total} sampling positions checked against the oracle's arg-max, all equal")
    assert checked > 0.97 * total, (checked, total)


@pytest.mark.parametrize("P", LENGTHS)
def test_ids_do_not_depend_on_the_group_or_the_other_slots(orc, tok, medium_bf16, slots_session, P):
    _same_session(medium_bf16, slots_session, pc.ids_do_not_depend_on_the_group(medium_bf16, orc, tok, ROWS, CAP, SLOTS, P))


def test_rows_that_share_nothing_equal_a_pool_without_slots(orc, tok, medium_bf16, slots_session):
    ses, plain = pc.rows_that_share_nothing(medium_bf16, orc, tok, ROWS, CAP, SLOTS, (5, 256, 300))
    _same_session(medium_bf16, slots_session, ses)
    assert plain.use_graphs and plain.kvs is None and plain.key != ses.key


@pytest.mark.parametrize("P", LENGTHS)
def test_a_child_of_a_sharing_parent_repeats_it(orc, tok, medium_bf16, slots_session, P):
    _same_session(medium_bf16, slots_session, pc.child_repeats_parent(medium_bf16, orc, tok, ROWS, CAP, SLOTS, P))


@pytest.mark.parametrize("P", LENGTHS)
def test_a_held_sharing_request_forked_later_equals_an_uninterrupted_one(orc, tok, medium_bf16, slots_session, P):
    ses = pc.held_then_forked_equals_uninterrupted(medium_bf16, orc, tok, ROWS, CAP, SLOTS, P)
    _same_session(medium_bf16, slots_session, ses)
    assert ses.held_hidden is not None and ses.held_hidden.dtype == torch.bfloat16
