"""The PRODUCTION decode path at 65 to 256 rows against the oracle on the MI355X: bf16 tv2o-medium through ``DecodeSession`` as
``generate()`` drives it -- captured graphs, folded norms, the 5-launch layer on mh_gemm_skinny_wide, the fused sampler -- by the
criterion of test_decode_gpu.test_production_decode_session_matches_oracle, unchanged (that function is what runs here: hidden and
logits within DRIFT = 1.5 x the reference's own bf16 drift of tests/golden/medium_long_S2048.npz, greedy ids equal to the oracle's
masked arg-max wherever its top-2 margin exceeds twice that bound, every id inside the grammar mask, more than 0.4 of the followed
positions with a safe margin; it also asserts the folds, the three graphs and the fused sampler).  The oracle follows 12 of the rows:
both ends of every 64-row group the kernel walks, and rows inside them.  The oracle alone, continuing these prompts greedily, has a
safe margin at 196 / 288 (80 rows) and 130 / 192 (256 rows) of the followed positions: 0.68, against the 0.4 asked for.

And two equalities: generate_ragged over 80 prompts of equal length returns the ids of generate(batch_size=80) for the same seeded
generator, and a ragged and a plain session of 80 rows decode the same ids from the same state -- the projections are row-independent
within one launch geometry and the per-row attention is bit-equal per row."""
import numpy as np
import pytest
import torch

import test_decode_gpu as D
from test_decode_gpu import medium_bf16, tok  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,P,n_events,cap,rows", [(80, 17, 3, 256, (0, 15, 16, 31, 47, 48, 63, 64, 65, 70, 78, 79)),
                                                      (256, 9, 2, 256, (0, 63, 64, 65, 127, 128, 129, 191, 192, 200, 254, 255))],
                         ids=["b80", "b256"])
def test_production_decode_session_of_65_to_256_rows_matches_oracle(orc, tok, medium_bf16, golden, B, P, n_events, cap, rows):
    """(the called function asserts, before anything else, that the session it builds has fold1, lm_fold, the net / steps / noise
    graphs and the fused sampler: at these row counts that is the feature)"""
    D.test_production_decode_session_matches_oracle(orc, tok, medium_bf16, golden, B, P, n_events, cap, rows)


def test_generate_ragged_of_equal_lengths_is_generate_at_80_rows(orc, tok, medium_bf16):
    """generate_ragged over 80 prompts of 5 events against generate(batch_size=80), max_len 12, generators seeded alike (top_k 20):
    the ids are equal and the generators end in the same state.  Prompts of one length are prefilled by the uniform forward in
    both calls (DecodeSession.prefill_ragged), the projections of the decode steps are row-independent within one launch geometry
    and the per-row attention is bit-equal to the uniform one per row.  Through the packed prefill, which rotates the
    rounded q|k|v product in a launch of its own, the states differed by bf16 roundings (hidden 7.8e-2, K 3.9e-2) and 72 of the 80
    rows parted -- as 62 of 64 did at batch 64 on the narrow kernel."""
    model = medium_bf16[2]
    B, P, L = 80, 5, 12
    prompt = orc.synthetic_events(tok, B, P, seed=33).numpy()
    g0, g1 = (torch.Generator(device="cuda").manual_seed(7) for _ in range(2))
    ref = model.generate(prompt, batch_size=B, max_len=L, ban_eos=True, generator=g0)
    out = model.generate_ragged([prompt[b] for b in range(B)], max_len=L, ban_eos=True, generator=g1)
    plain = [s for s in model._sessions.idle if s.B == B and not s.ragged]
    ragged = [s for s in model._sessions.idle if s.B == B and s.ragged]
    assert plain and ragged and all(s.wide and s.fold1 is not None and s.g_steps is not None for s in plain + ragged)
    differ = [b for b in range(B) if len(out[b]) != ref.shape[1] or not np.array_equal(out[b], ref[b])]
    print(f"generate_ragged vs generate at {B} rows: {len(differ)} rows differ")
    assert not differ, f"{len(differ)} of {B} rows differ, first {differ[:8]}"
    assert torch.equal(g0.get_state(), g1.get_state())


def test_ragged_and_plain_sessions_of_80_rows_decode_the_same_ids_from_the_same_state(orc, tok, medium_bf16):
    """What the equality rests on, without the prefill: a plain and a ragged session of 80 rows, the ragged one given the plain
    one's state after its prefill (hidden, K/V rows, positions), generators seeded alike, 6 events through the captured graphs
    (top_k 20: the sampler's draws included).  The projections are row-independent within one launch geometry -- both sessions run
    mh_gemm_skinny_wide on 80 rows -- and the per-row attention is bit-equal to the uniform one per row: every id equal."""
    from midi_model_amd.decode import DecodeSession
    model = medium_bf16[2]
    B, P, n_events = 80, 5, 6
    prompt = orc.synthetic_events(tok, B, P, seed=33).cuda()
    with torch.inference_mode():
        a = DecodeSession(model, B, 256, 1.0, 0.98, 20)
        r = DecodeSession(model, B, 256, 1.0, 0.98, 20, ragged=True)
        for ses in (a, r):
            assert ses.wide and ses.fold1 is not None and ses.g_steps is not None and ses.g_net is not None
            ses.first_mask.copy_(model._grammar()[0])
            ses.ban.zero_()
            ses.reset()
        a.prefill(prompt)
        r.hidden.copy_(a.hidden)
        r.kv1.k.copy_(a.kv1.k), r.kv1.v.copy_(a.kv1.v)
        r.pos.fill_(P)
        r.set_limit(P + n_events + 1)
        a.begin(torch.Generator(device="cuda").manual_seed(7))
        r.begin(torch.Generator(device="cuda").manual_seed(7))
        for i in range(n_events):
            ea, _ = a.sample_event(then_net=True)
            er, _ = r.sample_event(then_net=True)
            assert np.array_equal(ea, er), (i, np.flatnonzero((ea != er).any(-1))[:8].tolist())
            assert r.pos.tolist() == [P + i + 1] * B and int(a.pos.item()) == P + i + 1
        torch.cuda.synchronize()
        assert torch.equal(a.hidden, r.hidden)
        a.end(), r.end()
