"""Host logic of ``TrainMIDIModel(precision="bf16-mixed")`` on CPU: fp32 master weights, fp32 moments and an fp32 gradient
accumulator behind the bf16 parameters (midi_model_amd/mixed.py), driven through the CPU stand-ins (tests/emu_ops.py +
tests/emu_mixed.py).  The same checks run on the HIP kernels in test_mixed_precision_gpu.py, which imports the helpers here."""
import os
import socket
import sys

import numpy as np
import pytest
import torch

import midi_model_amd as mm
from midi_model_amd.train import TrainMIDIModel, lr_lambda

import emu_mixed

NO_DECAY = ("bias", "norm")


def tiny_config():
    return mm.MIDIModelConfig.get_config("v2", True, 4, 4, 256, 512)


def tiny_weights(orc, tok, seed=1):
    shp = orc.Shape(n_layer=4, n_head=4, n_embd=256, n_inner=512, vocab=tok.vocab_size)
    return shp, orc.make_state_dict(shp, seed=seed)


def mixed_model(sd, device="cpu", **kw):
    """a bf16 model on `device` in bf16-mixed whose MASTER holds the fp32 tensors of `sd` bit for bit"""
    m = TrainMIDIModel(tiny_config(), precision="bf16-mixed", **kw).to(device, torch.bfloat16)
    m.configure_optimizers()
    m.load_state_dict(sd)
    return m


@pytest.fixture(scope="module")
def tok():
    return mm.MIDITokenizerV2()


# ------------------------------------------------------------------------------------------ helpers shared with the GPU file
def replay_against_torch(model, batches, nacc):
    """Run len(batches) / nacc optimiser steps of `model` (bf16-mixed), capturing the fp32 accumulator before every update;
    then feed the captured gradients, the same clip rule (clip_grad_norm_(1.0)) and the same learning rates (LambdaLR over
    lr_lambda) to the real torch.optim.AdamW on fp32 parameters started from the same master, in the reference's two groups.
    Asserts the working copy is the bf16 rounding of the master after every step; returns (master, torch's parameters) flat."""
    mx = model._mixed
    start = mx.master.detach().cpu().clone()
    captured = []
    for i, b in enumerate(batches):
        model.training_step(b)
        if (i + 1) % nacc == 0:
            captured.append(mx.g32.detach().cpu().clone())
            model.optimizer_step()
            assert torch.equal(model._flat, mx.master.to(torch.bfloat16)), f"working copy != bf16(master) after step {len(captured)}"
    assert model.global_step == len(captured) and model._micro == 0
    names = list(model._offsets)
    params = {}
    for n in names:
        off, cnt, _ = model._offsets[n]
        params[n] = start[off:off + cnt].clone().requires_grad_(True)
    opt = torch.optim.AdamW([{"params": [params[n] for n in names if not any(nd in n for nd in NO_DECAY)], "weight_decay": model.weight_decay},
                             {"params": [params[n] for n in names if any(nd in n for nd in NO_DECAY)], "weight_decay": 0.0}],
                            lr=model.lr, betas=model.betas, eps=model.eps)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: lr_lambda(s, model.warmup, model.max_step))
    for g in captured:
        for n in names:
            off, cnt, _ = model._offsets[n]
            params[n].grad = g[off:off + cnt].clone()
        torch.nn.utils.clip_grad_norm_(list(params.values()), model.gradient_clip_val)
        opt.step()
        sched.step()
    want = torch.cat([params[n].detach() for n in names])
    return mx.master.detach().cpu(), want


def window_gradients(mixed, plain, batches):
    """g32 of `mixed` after one window over `batches`, and the fp32 sum of the micro-batch gradients `plain` (bf16-true, same
    weights, same accumulate_grad_batches) computes one at a time with zero_grad between"""
    plain._flat.copy_(mixed._flat)
    plain.weights_written()
    want = None
    for b in batches:
        plain.zero_grad()
        plain.training_step(b)
        g = plain.grad_buffer().float().clone()
        want = g if want is None else want + g
    plain.zero_grad()
    for b in batches:
        mixed.training_step(b)
    return mixed._mixed.g32.clone(), want


# ------------------------------------------------------------------------------------------------------------ tests
def test_precision_keyword_names_and_refusals(orc, tok):
    _, sd = tiny_weights(orc, tok)
    for name in (None, "bf16-true", "bf16", "32-true", "32"):
        assert TrainMIDIModel(tiny_config(), precision=name).precision is None      # today's behaviour under every such name
    for bad in ("16-mixed", "16-true", "64-true", "fp8"):
        with pytest.raises(ValueError, match="bf16-mixed"):
            TrainMIDIModel(tiny_config(), precision=bad)
    with emu_mixed.install():
        m = TrainMIDIModel(tiny_config(), precision="bf16-mixed")                    # fp32 model: refused when the optimiser is built
        with pytest.raises(TypeError, match="bfloat16"):
            m.configure_optimizers()
        m = m.to(torch.bfloat16)
        with pytest.raises(NotImplementedError, match="LoRA"):
            m.add_adapter(r=4)
        m.configure_optimizers()
        with pytest.raises(RuntimeError, match="master"):
            m.float()
        with pytest.raises(RuntimeError, match="master"):
            m.to(torch.float32)
        with pytest.raises(RuntimeError, match="bf16-mixed"):
            TrainMIDIModel(tiny_config()).master_state_dict()


@pytest.mark.parametrize("nacc", [1, 2, 3])
def test_window_folds_overwrite_then_add(orc, tok, nacc):
    """the first micro-batch of a window overwrites the fp32 accumulator, later ones add, and the window's sum is the fp32 sum
    of the bf16 micro-batch gradients -- bit for bit on the (order-deterministic) CPU stand-ins -- for two windows in a row"""
    _, sd = tiny_weights(orc, tok)
    kw = dict(lr=1e-2, warmup=0, max_step=10, accumulate_grad_batches=nacc)
    with emu_mixed.install():
        m = mixed_model(sd, **kw)
        plain = TrainMIDIModel(tiny_config(), **kw).to(torch.bfloat16)
        for w in range(2):
            batches = [orc.synthetic_events(tok, 2, 9, seed=500 + 10 * w + i) for i in range(nacc)]
            m._mixed.g32.fill_(123.0)     # whatever the last window left must not leak into this one
            got, want = window_gradients(m, plain, batches)
            assert m._micro == nacc and torch.equal(got, want), (w, (got - want).abs().max().item())
            before = m._mixed.master.clone()
            m.optimizer_step()
            assert m._micro == 0 and m.global_step == w + 1 and not torch.equal(before, m._mixed.master)
            assert torch.equal(m._flat, m._mixed.master.to(torch.bfloat16))


def test_replay_against_torch_adamw_cpu(orc, tok):
    """six optimiser steps (accumulate 2, lr 1e-3, warm-up 2): the master follows the real torch.optim.AdamW fed the captured
    fp32 gradients within rtol 1e-5 / atol 1e-6 (six times the one-step bound: the errors compound through m and v)"""
    _, sd = tiny_weights(orc, tok)
    batches = [orc.synthetic_events(tok, 2, 9, seed=600 + i) for i in range(12)]
    with emu_mixed.install():
        m = mixed_model(sd, lr=1e-3, warmup=2, max_step=10, accumulate_grad_batches=2)
        got, want = replay_against_torch(m, batches, 2)
    assert not torch.equal(got, torch.cat([sd[n].reshape(-1) for n in m._offsets]))
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-5, atol=1e-6)


def test_fp32_checkpoint_in_and_out_cpu(orc, tok, tmp_path):
    """fp32 tensors with low mantissa bits set go into the master untouched; training_state() -> load_training_state into a
    fresh mixed model is bit-equal in master, m, v, step, phase and (inside a window) the fp32 accumulator; the written
    optimiser / scheduler dictionaries load into the real torch objects"""
    _, sd = tiny_weights(orc, tok)
    sd = {k: (v * (1.0 + 2.0 ** -20)).float() for k, v in sd.items()}              # bits a bf16 round trip would drop
    assert any(not torch.equal(v, v.to(torch.bfloat16).float()) for v in sd.values())
    kw = dict(lr=1e-2, warmup=2, max_step=10, accumulate_grad_batches=2)
    batches = [orc.synthetic_events(tok, 2, 9, seed=700 + i) for i in range(4)]
    with emu_mixed.install():
        a = TrainMIDIModel(tiny_config(), precision="bf16-mixed", **kw).to(torch.bfloat16)
        a.load_training_state({"state_dict": sd, "optimizer_states": [{"state": {}, "param_groups": [{"params": list(range(len(sd)))}]}],
                               "global_step": 0})
        msd = a.master_state_dict()
        assert all(msd[k].dtype == torch.float32 and torch.equal(msd[k], sd[k]) for k in sd)
        assert all(t.dtype == torch.bfloat16 for t in a.state_dict().values())
        assert torch.equal(a._flat, a._mixed.master.to(torch.bfloat16))
        for b in batches[:3]:                                                        # one step + one micro-batch into the next window
            a.fit_step(b)
        path = str(tmp_path / "mixed.ckpt")
        a.save_training_state(path)
        state = torch.load(path, map_location="cpu", weights_only=True)
        assert all(t.dtype == torch.float32 for t in state["state_dict"].values()) and state["mh_grad"].dtype == torch.float32
        b_ = TrainMIDIModel(tiny_config(), precision="bf16-mixed", **kw).to(torch.bfloat16)
        b_.load_training_state(path)
        assert b_.global_step == a.global_step == 1 and b_._micro == a._micro == 1
        for k in ("master", "m", "v", "g32"):
            assert torch.equal(getattr(b_._mixed, k), getattr(a._mixed, k)), k
        assert torch.equal(b_._flat, a._flat)
        la, lb = a.fit_step(batches[3]), b_.fit_step(batches[3])
        assert torch.equal(la, lb) and torch.equal(a._mixed.master, b_._mixed.master) and b_.global_step == 2
        state = b_.training_state()
    load_into_torch_objects(b_, state)


def load_into_torch_objects(model, state):
    """what training_state() writes in bf16-mixed loads into the real torch.optim.AdamW (fp32 parameters, the reference's two
    groups) and LambdaLR, as tests/test_host_logic.py checks for the native layout"""
    named = [(k, state["state_dict"][k].clone().requires_grad_(True)) for k, _ in model.named_parameters()]
    assert all(p.dtype == torch.float32 for _, p in named)
    opt = torch.optim.AdamW([{"params": [p for n, p in named if not any(nd in n for nd in NO_DECAY)], "weight_decay": 0.01},
                             {"params": [p for n, p in named if any(nd in n for nd in NO_DECAY)], "weight_decay": 0.0}],
                            lr=model.lr, betas=(0.9, 0.99), eps=1e-8)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s_: lr_lambda(s_, model.warmup, model.max_step))
    opt.load_state_dict(state["optimizer_states"][0])
    sched.load_state_dict(state["lr_schedulers"][0])
    assert sched.last_epoch == model.global_step and abs(sched.get_last_lr()[0] - model.current_lr()) < 1e-12
    st = opt.state_dict()["state"]
    order = model._optimizer_param_order([n for n, _ in named])
    for i, n in enumerate(order):
        off, cnt, _ = model._offsets[n]
        assert st[i]["exp_avg"].dtype == torch.float32 and st[i]["exp_avg_sq"].dtype == torch.float32
        assert torch.equal(st[i]["exp_avg"].reshape(-1), model._mixed.m[off:off + cnt].cpu()), n
        assert torch.equal(st[i]["exp_avg_sq"].reshape(-1), model._mixed.v[off:off + cnt].cpu()), n
        assert int(st[i]["step"]) == model.global_step


# --------------------------------------------------------------------------------------------- two ranks over gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import torch.distributed as dist
    from conftest import load_oracle
    import emu_mixed as em
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    orc = load_oracle()
    tok = mm.MIDITokenizerV2()
    shp = orc.Shape(n_layer=4, n_head=4, n_embd=256, n_inner=512, vocab=tok.vocab_size)
    sd = orc.make_state_dict(shp, seed=1)
    with em.install():
        model = TrainMIDIModel(tiny_config(), lr=1e-2, warmup=0, accumulate_grad_batches=1, bucket_mb=1,
                               precision="bf16-mixed").to(torch.bfloat16)
        model.configure_optimizers()
        if rank == 0:
            model.load_state_dict(sd)
        model.broadcast_parameters(0)          # the MASTER travels; rank 1 started from different random weights
        start = model._mixed.master.clone()
        assert torch.equal(model._flat, start.to(torch.bfloat16))
        model.training_step(orc.synthetic_events(tok, 2, 9, seed=800 + rank))
        red = model._reducer
        assert red is not None and red.flat is model._mixed.g32
        n_buckets = len(red.launched)
        red.profile = True
        model.optimizer_step()
        (_, _, nbytes, nlaunch), = red.stats
        assert nbytes == 4 * model._flat.numel() and n_buckets <= nlaunch <= n_buckets + 1
        np.savez(os.path.join(out_dir, f"mixed_rank{rank}.npz"), start=start.numpy(), master=model._mixed.master.numpy(),
                 flat=model._flat.float().numpy(), g32=model._mixed.g32.numpy(), n_buckets=n_buckets)
        if rank == 0:
            # ONE rank accumulating the two batches in a window, computed here: the same process, thread count and CPU kernels
            # as the two-rank step (the bf16 matrix products of the CPU stand-ins depend on them), its exchange switched off
            one = mixed_model(sd, lr=1e-2, warmup=0, accumulate_grad_batches=2)
            one._reducer_for_step = lambda: None
            assert torch.equal(one._mixed.master, start)                              # fp32 bits of rank 0's weights
            for r in range(world):
                one.training_step(orc.synthetic_events(tok, 2, 9, seed=800 + r))
            g_one = one._mixed.g32.clone()
            one.optimizer_step()
            np.savez(os.path.join(out_dir, "mixed_one.npz"), g32=g_one.numpy(), master=one._mixed.master.numpy())
    dist.destroy_process_group()


def test_two_gloo_ranks_equal_one_rank_accumulating(tmp_path, orc, tok):
    """two ranks with one batch each end on the master one rank reaches by accumulating the two batches in a window (the mean
    of the two gradients either way), within the bound the native world-2 test holds its averaged gradient to; the parameter
    broadcast carried the fp32 master, and the exchange moved 4 bytes per parameter in several buckets"""
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = np.load(tmp_path / "mixed_rank0.npz"), np.load(tmp_path / "mixed_rank1.npz")
    one = np.load(tmp_path / "mixed_one.npz")
    np.testing.assert_array_equal(r0["start"], r1["start"])
    np.testing.assert_array_equal(r0["g32"], r1["g32"])
    np.testing.assert_array_equal(r0["master"], r1["master"])
    np.testing.assert_array_equal(r0["flat"], r1["flat"])
    assert int(r0["n_buckets"]) >= 3 and not np.array_equal(r0["master"], r0["start"])
    np.testing.assert_allclose(r0["g32"], one["g32"], rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(r0["master"], one["master"], rtol=1e-4, atol=1e-7)
