"""training_step / validation_step / fit_step on a data.PackedBatch on the MI355X, tiny config of test_model_gpu.py, four windows
of 17, 5, 2 and 12 events: against the CPU oracle's autograd on the PADDED batch of the same windows (fp32, the tolerances of
test_tiny_fp32_fused_step_and_optimizer), against the padded bf16 step (bf16), and run to run."""
import numpy as np
import pytest
import torch

import midi_model_amd as mm
from midi_model_amd.data import PackedBatch, TokenCorpus, WindowSampler
from midi_model_amd.train import TrainMIDIModel

pytestmark = pytest.mark.gpu

LENS = [17, 5, 2, 12]
H = 4


def tiny_config():
    return mm.MIDIModelConfig.get_config("v2", True, 4, H, 256, 512)


@pytest.fixture(scope="module")
def tok():
    return mm.MIDITokenizerV2()


@pytest.fixture(scope="module")
def case(orc, tok):
    """weights, the padded batch, and the oracle's loss and gradients on it (computed once)"""
    shp = orc.Shape(n_layer=4, n_head=H, n_embd=256, n_inner=512, vocab=tok.vocab_size)
    sd = orc.make_state_dict(shp, seed=1)
    batch = orc.synthetic_events(tok, len(LENS), max(LENS), seed=2)
    for i, n in enumerate(LENS):
        batch[i, n:] = tok.pad_id
    sdg = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    loss, _ = orc.training_loss(sdg, shp, batch)
    loss.backward()
    return sd, batch, loss.item(), {k: v.grad for k, v in sdg.items()}


def build(sd, dtype, **kw):
    m = TrainMIDIModel(tiny_config(), accumulate_grad_batches=1, **kw)
    m.load_state_dict(sd, strict=True)
    return m.to("cuda", dtype)


def packed(batch, tok):
    return PackedBatch.from_padded(batch.cuda(), LENS, tok.pad_id)


def test_fp32_packed_step_against_the_oracle_on_the_padded_batch(case, tok):
    sd, batch, loss_ref, grads_ref = case
    model = build(sd, torch.float32)
    pb = packed(batch, tok)
    assert pb.x.shape[0] == 64 and pb.lengths == (16, 4, 1, 11, 32) and pb.tail == 32
    loss = model.training_step(pb)
    print(f"fp32 packed loss {loss.item():.7f}, oracle (padded) {loss_ref:.7f}")
    assert abs(loss.item() - loss_ref) < 1e-4
    named = dict(model.named_parameters())
    names = sorted(grads_ref)
    norms = np.array([named[n].grad.norm().item() for n in names])
    np.testing.assert_allclose(norms, np.array([grads_ref[n].norm().item() for n in names]), rtol=2e-3, atol=1e-7)
    for n in names:
        gr, ref = named[n].grad.cpu(), grads_ref[n]
        got, want = (gr.numpy(), ref.numpy()) if gr.dim() == 1 else (gr[:64:3, ::5].numpy(), ref[:64:3, ::5].numpy())
        np.testing.assert_allclose(got, want, rtol=5e-3, atol=1e-6, err_msg=n)
    vloss, acc = model.validation_step(pb)
    vloss_p, acc_p = model.validation_step(batch)
    assert abs(vloss.item() - loss_ref) < 1e-4 and abs(vloss.item() - vloss_p.item()) < 1e-4
    assert abs(acc.item() - acc_p.item()) < 1e-6


def test_bf16_packed_step_is_as_close_to_the_oracle_as_the_padded_step(case, tok):
    """the rule of test_two_times_hidden_step_at_S4096: the packed loss lies within 1.5 x the padded bf16 step's own distance to
    the fp32 oracle loss; two packed runs are bit-identical (loss and every gradient)"""
    sd, batch, loss_ref, _ = case
    lp = build(sd, torch.bfloat16).training_step(batch).item()
    runs = []
    for _ in range(2):
        m = build(sd, torch.bfloat16)
        loss = m.training_step(packed(batch, tok))
        runs.append((loss.clone(), {k: p.grad.clone() for k, p in m.named_parameters()}))
    lq = runs[0][0].item()
    print(f"bf16 distances to the fp32 oracle loss {loss_ref:.6f}: padded {abs(lp - loss_ref):.3e}, packed {abs(lq - loss_ref):.3e}")
    assert abs(lq - loss_ref) <= 1.5 * abs(lp - loss_ref)
    assert torch.equal(runs[0][0], runs[1][0])
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k
        assert torch.isfinite(runs[0][1][k].float()).all(), k


def test_sampler_packed_fit_step_runs_and_repeats(case, tok):
    sd = case[0]
    rng = np.random.default_rng(5)
    pieces = [rng.integers(1, tok.vocab_size, size=(n, 8)).astype(np.int16) for n in (40, 3, 25, 90, 2)]
    losses = []
    for _ in range(2):
        model = build(sd, torch.bfloat16, lr=1e-3, warmup=0)
        sampler = WindowSampler(TokenCorpus(pieces, device="cuda"), max_len=32, rand_start=True, seed=3)
        idx = next(sampler.fill(iter([3, 0, 1, 2, 4]), 128))
        pb = sampler.packed_batch(idx, tok.pad_id)
        assert pb.x.is_cuda and pb.x.shape[0] % 64 == 0 and pb.real_rows <= 128
        losses.append(model.fit_step(pb).clone())
        assert model.global_step == 1 and torch.isfinite(losses[-1]).all()
    assert torch.equal(losses[0], losses[1])
