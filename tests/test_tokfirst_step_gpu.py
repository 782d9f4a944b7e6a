"""The training step on the device with the first token-level block per vocabulary entry (TrainMIDIModel.tok_table_first,
engine.tok_first_forward / tok_first_backward) against the same step with every block dense: bit-equal loss, and gradients no
further from the fp32 oracle's than 1.5 x the dense bf16 step's own distance -- the factor the parity tests grant over the
reference's bf16 drift."""
import random

import pytest
import torch

import midi_model_amd as mm
from midi_model_amd import ops, tokfirst
from midi_model_amd.train import TrainMIDIModel

pytestmark = pytest.mark.gpu

# (n_layer, events per sequence + 1, sample_seq): the tiny configuration of tests/test_model_gpu.py (one token-level block), the
# same with train.py's sampling of positions, and the tiny widths at 12 layers -- three token-level blocks, so that the call
# counter can tell the first from the other two
CASES = {"tiny": (4, 17, False), "tiny_sample_seq": (4, 17, True), "three_token_blocks": (12, 17, False)}


def oracle_grads(orc, shp, sd, batch, sel):
    sdg = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    if sel is None:
        loss, _ = orc.training_loss(sdg, shp, batch)
    else:  # train.py:172-175 on the oracle's pieces: the token-level net sees the selected positions only
        x, y = batch[:, :-1], batch[:, 1:]
        hidden = orc.midi_forward(sdg, shp, x)[:, sel].reshape(-1, shp.n_embd)
        y = y[:, sel].reshape(-1, y.shape[-1])
        logits = orc.midi_forward_token(sdg, shp, hidden, y[:, :-1])
        loss = torch.nn.functional.cross_entropy(logits.reshape(-1, shp.vocab), y.reshape(-1), reduction="mean", ignore_index=0)
    loss.backward()
    return {k: v.grad for k, v in sdg.items()}


@pytest.mark.parametrize("case", list(CASES))
def test_step_with_the_table_form_against_the_dense_step(orc, case, monkeypatch):
    n_layer, length, sample = CASES[case]
    tok = mm.MIDITokenizerV2()
    cfg = mm.MIDIModelConfig.get_config("v2", True, n_layer, 4, 256, 512)
    shp = orc.Shape(n_layer=n_layer, n_head=4, n_embd=256, n_inner=512, vocab=tok.vocab_size)
    sd = orc.make_state_dict(shp, seed=1)
    batch = orc.synthetic_events(tok, 2, length, seed=2)
    batch[1, 14:] = tok.pad_id
    batch[0, 3, 2] = tok.pad_id                              # a pad in mid-sequence
    S = length - 1
    sel = None
    if sample:
        random.seed(5)
        idx = [-1] + random.sample(list(range(S - 2)), min(127, (S - 2) // 2))
        sel = torch.tensor([i % S for i in idx])
    ref = oracle_grads(orc, shp, sd, batch, sel)

    counts = {}
    for mod, name in ((tokfirst, "tokattn_fwd_rows"), (tokfirst, "tokattn_bwd_rows"), (ops, "tokattn_fwd"), (ops, "tokattn_bwd")):
        real = getattr(mod, name)
        monkeypatch.setattr(mod, name, lambda *a, _n=name, _f=real, **k: (counts.__setitem__(_n, counts.get(_n, 0) + 1), _f(*a, **k))[1])
    outs = {}
    for table in (False, True):
        m = TrainMIDIModel(cfg, accumulate_grad_batches=1, sample_seq=sample)
        m.load_state_dict(sd, strict=True)
        m = m.to("cuda", torch.bfloat16)
        m.tok_table_first = table
        counts.clear()
        random.seed(5)
        loss = m.fit_step(batch)
        torch.cuda.synchronize()
        nb = n_layer // 4
        want = {"tokattn_fwd_rows": 1, "tokattn_bwd_rows": 1, "tokattn_fwd": nb - 1, "tokattn_bwd": nb - 1} if table else \
            {"tokattn_fwd": nb, "tokattn_bwd": nb}
        assert {k: v for k, v in counts.items() if v} == {k: v for k, v in want.items() if v}, (table, counts)
        outs[table] = (loss.float().cpu().clone(), {k: p.grad.float().cpu().clone() for k, p in m.named_parameters()})
        del m
    assert torch.equal(outs[False][0], outs[True][0]), (outs[False][0], outs[True][0])
    worst = 0.0
    for k, r in ref.items():
        rn = r.norm().item()
        d_off = (outs[False][1][k] - r).norm().item() / rn
        d_on = (outs[True][1][k] - r).norm().item() / rn
        worst = max(worst, d_on / d_off)
        print(f"{case} {k}: rel L2 to the fp32 oracle  dense {d_off:.5f}  table {d_on:.5f}  ratio {d_on / d_off:.3f}")
    print(f"{case}: worst ratio {worst:.3f}")
    for k, r in ref.items():
        rn = r.norm().item()
        d_off = (outs[False][1][k] - r).norm().item() / rn
        d_on = (outs[True][1][k] - r).norm().item() / rn
        assert d_on <= 1.5 * d_off, (k, d_on, d_off)
    assert float(outs[True][1]["net_token.embed_tokens.weight"][tok.pad_id].abs().max()) == 0
