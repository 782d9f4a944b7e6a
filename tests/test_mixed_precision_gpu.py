"""``TrainMIDIModel(precision="bf16-mixed")`` on the device: the two new kernels (mh_adamw_master, mh_grad_fold_f32) against
torch, and the mixed-precision step at model level -- replay against the real torch.optim.AdamW, the fp32 window gradient, the
trajectory against the reference's own low-precision runs (tests/golden/tiny_mixed.npz, tests/gen_golden_mixed.py), fp32
checkpoints in and out, the bucketed exchange over the fp32 accumulator through both RCCL routes, and the refusals."""
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch

import midi_model_amd as mm
from midi_model_amd import mixed
from midi_model_amd.train import TrainMIDIModel

from test_mixed_precision_host import (load_into_torch_objects, mixed_model, replay_against_torch, tiny_config, tiny_weights,
                                       window_gradients)

pytestmark = pytest.mark.gpu

DRIFT = 1.5   # allowed multiple of the reference's own low-precision deviation (tests/test_parity_long_gpu.py)


@pytest.fixture(scope="module")
def tok():
    return mm.MIDITokenizerV2()


def rnd(n, seed, scale):
    return scale * torch.randn(n, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("case", ["n8", "tail", "offset_slice"])
@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("wd", [0.01, 0.0])
def test_adamw_master_against_torch_adamw(wd, clip, case):
    """mh_adamw_master against torch.optim.AdamW on CPU fp32 tensors: lr 3e-3, betas (0.9, 0.99), eps 1e-8, the third step's
    bias corrections on pre-seeded moments (seeded as test_clip_and_adamw seeds them), with and without a clip coefficient.
    p32, m, v within rtol 1e-6 / atol 1e-7 -- at most eight rounded fp32 operations per element at a relative 6e-8 each, the
    bound tests/test_emu_vs_oracle.py holds the fp32 AdamW restatement to -- and p_lo bit-equal to the bf16 rounding of the
    kernel's own p32.  Lengths: 100003 * 8; one that is not a multiple of 4 (scalar tail); a slice 96 bytes into a larger
    buffer whose neighbours must stay untouched."""
    n = {"n8": 100003 * 8, "tail": 100003 * 8 + 3, "offset_slice": 100003 * 8}[case]
    lo, pad = (24, 64) if case == "offset_slice" else (0, 0)
    p, g = rnd(n, 28, 0.02), rnd(n, 29, 0.01)
    m, v = rnd(n, 30, 0.001), rnd(n, 31, 0.001).abs()
    lr, b1, b2, eps = 3e-3, 0.9, 0.99, 1e-8
    coef = None
    if clip:
        from midi_model_amd import ops
        ss, part, coef, norm = (torch.zeros(1, device="cuda"), torch.empty(1024, device="cuda"), torch.empty(1, device="cuda"),
                                torch.empty(1, device="cuda"))
        ops.sumsq(g.cuda(), part, ss, False)
        ops.clip_coef(ss, 1.0, coef, norm)
        assert abs(norm.item() - g.norm().item()) < 1e-5 * g.norm().item() and 0 < coef.item() < 1
    # torch: one parameter whose state says two steps were taken
    pt = p.clone().requires_grad_(True)
    opt = torch.optim.AdamW([pt], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    opt.state[pt] = {"step": torch.tensor(2.0), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    pt.grad = g * coef.cpu() if clip else g.clone()
    opt.step()
    # device: the operands as slices [lo, lo + n) of buffers pre-filled with a sentinel
    def buf(t, dtype=torch.float32):
        b = torch.full((n + pad,), 7.0, dtype=dtype, device="cuda")
        b[lo:lo + n] = t.to(dtype).cuda()
        return b
    P, G, M, V, PL = buf(p), buf(g), buf(m), buf(v), buf(torch.zeros(n), torch.bfloat16)
    mixed.adamw_master(P[lo:lo + n], PL[lo:lo + n], G[lo:lo + n], M[lo:lo + n], V[lo:lo + n], lr, b1, b2, eps, wd,
                       1 - b1 ** 3, 1 - b2 ** 3, coef)
    torch.cuda.synchronize()
    st = opt.state[pt]
    for what, got, want in (("p32", P, pt.detach()), ("m", M, st["exp_avg"]), ("v", V, st["exp_avg_sq"])):
        got = got.cpu()
        err = (got[lo:lo + n] - want).abs()
        print(f"adamw_master {what} wd={wd} clip={clip} {case}: max abs err {err.max().item():.3e}, max err/bound "
              f"{(err / (1e-7 + 1e-6 * want.abs())).max().item():.3f}")
        np.testing.assert_allclose(got[lo:lo + n].numpy(), want.numpy(), rtol=1e-6, atol=1e-7, err_msg=what)
        assert (got[:lo] == 7.0).all() and (got[lo + n:] == 7.0).all(), f"{what}: wrote outside its range"
    assert torch.equal(PL[lo:lo + n], P[lo:lo + n].to(torch.bfloat16)), "p_lo is not the bf16 rounding of the kernel's own p32"
    assert (PL[:lo] == 7.0).all() and (PL[lo + n:] == 7.0).all()
    assert torch.equal(G[lo:lo + n].cpu(), g), "the gradient accumulator is read-only"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_grad_fold_f32_is_exact(dtype):
    """dst = float(src) and dst += float(src): one exact conversion and one IEEE add, so bit-equal to torch; a length with a
    scalar tail, both source dtypes, a range inside a larger buffer"""
    n, lo = 100003 * 8 + 5, 16
    src = rnd(n, 40, 0.01).to(dtype).cuda()
    dst = torch.full((n + 40,), 3.0, device="cuda")
    base = rnd(n, 41, 0.01).cuda()
    dst[lo:lo + n] = base
    mixed.grad_fold(src, dst[lo:lo + n], True)
    assert torch.equal(dst[lo:lo + n], base + src.float())
    assert (dst[:lo] == 3.0).all() and (dst[lo + n:] == 3.0).all()
    mixed.grad_fold(src, dst[lo:lo + n], False)
    assert torch.equal(dst[lo:lo + n], src.float())
    assert (dst[:lo] == 3.0).all() and (dst[lo + n:] == 3.0).all()


# ------------------------------------------------------------------------------------------------------ model level
def test_replay_against_torch_adamw(orc, tok):
    """six optimiser steps with accumulate_grad_batches=2, lr 1e-3, warm-up 2; the fp32 accumulator captured before each update
    goes, with the same clip rule and learning rates, to the real torch.optim.AdamW on fp32 parameters started from the same
    master in the reference's two groups.  Master after six steps within rtol 1e-5 / atol 1e-6 (six times the one-step bound:
    errors compound through m and v); the bf16 parameters are bit-equal to master.to(bf16) after every step."""
    _, sd = tiny_weights(orc, tok)
    batches = [orc.synthetic_events(tok, 2, 33, seed=600 + i).cuda() for i in range(12)]
    m = mixed_model(sd, "cuda", lr=1e-3, warmup=2, max_step=10, accumulate_grad_batches=2)
    got, want = replay_against_torch(m, batches, 2)
    err = (got - want).abs()
    print(f"replay: max abs err {err.max().item():.3e}, max err/bound {(err / (1e-6 + 1e-5 * want.abs())).max().item():.3f}")
    assert m.last_grad_norm.item() > 0 and abs(m.current_lr() - 1e-3 * 4 / 8) < 1e-12
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-5, atol=1e-6)


def test_window_gradient_is_the_fp32_sum(orc, tok):
    """g32 after a window of two micro-batches = the fp32 sum of the two bf16 micro-batch gradients computed one at a time in
    bf16-true from the same weights: bit-equal outside the embedding tables; inside them the allowance the forced-exchange test
    of tests/test_ddp_gpu.py grants the unspecified order of the embedding backward's sums (at most 8 elements, one bf16 step)"""
    _, sd = tiny_weights(orc, tok)
    kw = dict(lr=1e-2, warmup=0, accumulate_grad_batches=2)
    m = mixed_model(sd, "cuda", **kw)
    plain = TrainMIDIModel(tiny_config(), **kw).to("cuda", torch.bfloat16)
    batches = [orc.synthetic_events(tok, 2, 33, seed=500 + i).cuda() for i in range(2)]
    m._mixed.g32.fill_(123.0)
    got, want = window_gradients(m, plain, batches)
    diff = got != want
    inside = torch.zeros_like(diff)
    for n in ("net.embed_tokens.weight", "net_token.embed_tokens.weight"):
        off, cnt, _ = m._offsets[n]
        inside[off:off + cnt] = True
    n_diff, n_outside = int(diff.sum()), int((diff & ~inside).sum())
    rel = ((got - want).abs() / want.abs().clamp_min(1e-30))[diff]
    print(f"window gradient: {n_diff} differing elements, {n_outside} outside the embedding tables")
    assert want.abs().max() > 0 and n_outside == 0 and n_diff <= 8 and (n_diff == 0 or float(rel.max()) <= 2.0 ** -6)


def test_trajectory_against_the_reference(orc, tok, golden):
    """The reference's recipe for six optimiser steps (accumulate 2) run three ways by tests/gen_golden_mixed.py: fp32, bf16-true
    (``.bfloat16()``) and fp32 parameters under ``torch.autocast("cpu", torch.bfloat16)``.  The device run in bf16-mixed starts
    from the same fp32 weights loaded into the master directly.  At every step the micro-batch loss must stay within 1.5x the
    LARGER of the reference's two low-precision deviations from its fp32 run at that step (the factor of
    tests/test_parity_long_gpu.py; our forward is the bf16-true one, our optimiser the fp32 one).  The final parameter norms are
    held to the same factor on the worst and on the rms relative deviation over the 140 tensors, not tensor by tensor: a single
    tensor's norm deviation is a signed sum that in the reference's own runs cancels down to the fp32 resolution of the norm
    itself for some tensors (3e-6 of 5.18 in one of them), which bounds nothing.  The measured ratios are printed."""
    g = golden("tiny_mixed.npz")
    shp, sd = tiny_weights(orc, tok, int(g["weight_seed"]))
    nacc, steps = int(g["nacc"]), int(g["steps"])
    batches = [orc.synthetic_events(tok, int(g["batch"]), int(g["events"]), seed=int(g["batch_seed0"]) + i) for i in range(steps * nacc)]
    m = mixed_model(sd, "cuda", lr=float(g["lr"]), warmup=int(g["warmup"]), max_step=int(g["max_step"]),
                    weight_decay=float(g["weight_decay"]), accumulate_grad_batches=nacc)
    losses = np.array([m.fit_step(b.cuda()).item() for b in batches])
    assert m.global_step == steps
    ref = g["losses_fp32"]
    allow = np.maximum(np.abs(g["losses_bf16"] - ref), np.abs(g["losses_autocast"] - ref))
    ratio = np.abs(losses - ref) / allow
    print("loss deviation / larger reference deviation per micro-batch:", np.round(ratio, 3).tolist())
    msd = m.master_state_dict()
    names = [str(n) for n in g["param_names"]]
    norms = np.array([msd[n].double().norm().item() for n in names])
    nref = g["param_norms_fp32"]
    rel = lambda x: np.abs(x - nref) / nref                       # per-tensor relative deviation of the norm from the fp32 run's
    ours, ref_lo = rel(norms), (rel(g["param_norms_bf16"]), rel(g["param_norms_autocast"]))
    per_tensor = ours / np.maximum(np.maximum(*ref_lo), 1e-300)
    worst = int(np.argmax(per_tensor))
    stats = {"max": np.max, "rms": lambda x: float(np.sqrt(np.mean(x ** 2)))}
    for what, f in stats.items():
        print(f"parameter norms, {what} relative deviation over the {len(names)} tensors: ours {f(ours):.3e}, reference bf16-true "
              f"{f(ref_lo[0]):.3e}, reference autocast {f(ref_lo[1]):.3e}")
    print(f"  (per tensor, for information: largest ours / larger reference deviation {per_tensor.max():.3f} at {names[worst]})")
    assert (np.abs(losses - ref) <= DRIFT * allow).all(), ratio.tolist()
    for what, f in stats.items():
        assert f(ours) <= DRIFT * max(f(ref_lo[0]), f(ref_lo[1])), what


def test_fp32_checkpoint_in_and_out(orc, tok, tmp_path):
    """an fp32 checkpoint with low mantissa bits set lands in the master bit for bit; training_state() -> load_training_state
    into a fresh mixed model is bit-equal in master, m, v, step, phase and -- inside a window -- g32; the written optimiser and
    scheduler dictionaries load into the real torch.optim.AdamW (fp32 parameters) and LambdaLR"""
    _, sd = tiny_weights(orc, tok)
    sd = {k: (v * (1.0 + 2.0 ** -20)).float() for k, v in sd.items()}
    assert any(not torch.equal(v, v.to(torch.bfloat16).float()) for v in sd.values())
    kw = dict(lr=1e-2, warmup=2, max_step=10, accumulate_grad_batches=2)
    batches = [orc.synthetic_events(tok, 2, 33, seed=700 + i).cuda() for i in range(4)]
    a = TrainMIDIModel(tiny_config(), precision="bf16-mixed", **kw).to("cuda", torch.bfloat16)
    a.load_training_state({"state_dict": sd, "optimizer_states": [{"state": {}, "param_groups": [{"params": list(range(len(sd)))}]}],
                           "global_step": 0})
    msd = a.master_state_dict()
    assert all(msd[k].dtype == torch.float32 and torch.equal(msd[k].cpu(), sd[k]) for k in sd)
    assert all(t.dtype == torch.bfloat16 for t in a.state_dict().values())
    assert torch.equal(a._flat, a._mixed.master.to(torch.bfloat16))
    for b in batches[:3]:
        a.fit_step(b)
    path = str(tmp_path / "mixed.ckpt")
    a.save_training_state(path)
    state = torch.load(path, map_location="cpu", weights_only=True)
    assert all(t.dtype == torch.float32 for t in state["state_dict"].values()) and state["mh_grad"].dtype == torch.float32
    b_ = TrainMIDIModel(tiny_config(), precision="bf16-mixed", **kw).to("cuda", torch.bfloat16)
    b_.load_training_state(path)
    assert b_.global_step == a.global_step == 1 and b_._micro == a._micro == 1
    for k in ("master", "m", "v", "g32"):
        assert torch.equal(getattr(b_._mixed, k), getattr(a._mixed, k)), k
    assert torch.equal(b_._flat, a._flat)
    # a bf16 checkpoint upcasts
    c = TrainMIDIModel(tiny_config(), precision="bf16-mixed", **kw).to("cuda", torch.bfloat16)
    lo_sd = {k: v.to(torch.bfloat16) for k, v in sd.items()}
    c.load_training_state({"state_dict": lo_sd, "optimizer_states": [{"state": {}, "param_groups": [{"params": list(range(len(sd)))}]}]})
    assert all(torch.equal(t.cpu(), lo_sd[k].float()) for k, t in c.master_state_dict().items())
    load_into_torch_objects(b_, b_.training_state())


def test_refusals(orc, tok):
    for bad in ("16-mixed", "16-true", "64-true"):
        with pytest.raises(ValueError, match="bf16-mixed"):
            TrainMIDIModel(tiny_config(), precision=bad)
    m = TrainMIDIModel(tiny_config(), precision="bf16-mixed").to("cuda")              # an fp32 model
    with pytest.raises(TypeError, match="bfloat16"):
        m.configure_optimizers()
    m = m.to(torch.bfloat16)
    with pytest.raises(NotImplementedError, match="LoRA"):
        m.add_adapter(r=4)
    m.configure_optimizers()
    with pytest.raises(RuntimeError, match="master"):
        m.float()
    b = orc.synthetic_events(tok, 2, 33, seed=3).cuda()                                # and the model still trains
    m.accumulate_grad_batches = 1
    assert math.isfinite(m.fit_step(b).item()) and m.global_step == 1


# ------------------------------------------------------------------------------------------------------ exchange
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker_world1(rank, port, out_dir, backend):
    """tests/test_ddp_gpu.py::_worker_world1 in bf16-mixed: the real RCCL backends at world size 1 forced through the reducer's
    bucketed path inside the benchmarked step (tv2o-medium, 16 x 2048 events), over the fp32 accumulator"""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1")
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import torch.distributed as dist
    from midi_model_amd.comm import MHComm
    from midi_model_amd.data import synthetic_events
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1)
    dev = torch.device("cuda", 0)
    cfg = mm.MIDIModelConfig.from_name("tv2o-medium")
    torch.manual_seed(0)
    model = TrainMIDIModel(cfg, lr=2e-4, warmup=0, accumulate_grad_batches=1, precision="bf16-mixed").to(dev, torch.bfloat16)
    model.configure_optimizers()
    mx = model._mixed
    start = mx.master.detach().clone()
    batch = synthetic_events(model.tokenizer, 16, 2049, seed=5, device="cuda")
    loss_plain = model.fit_step(batch).item()                      # the plain single-GPU mixed step (no exchange)
    master_plain = mx.master.detach().clone()
    mx.master.copy_(start)                                         # the same step from the same state, exchange forced
    mx.derive_working_copy()
    model.weights_written()
    mx.m.zero_()
    mx.v.zero_()
    model.global_step = 0
    model.force_reduce = True
    if backend == "mh":
        model.use_comm(MHComm.from_process_group(0))
    model.broadcast_parameters(0)
    assert torch.equal(mx.master, start) and torch.equal(model._flat, start.to(torch.bfloat16))
    red = model._reducer_for_step()
    assert red is not None and red.force and red.flat is mx.g32 and (red.comm is not None) == (backend == "mh")
    red.profile = True
    loss_x = model.fit_step(batch).item()
    torch.cuda.synchronize()
    (ev0, ev1, nbytes, nlaunch), = red.stats
    diff = mx.master != master_plain
    inside = torch.zeros_like(diff)
    for n in ("net.embed_tokens.weight", "net_token.embed_tokens.weight"):
        off, cnt, _ = model._offsets[n]
        inside[off:off + cnt] = True
    n_diff, n_outside = int(diff.sum()), int((diff & ~inside).sum())
    rel = ((mx.master - master_plain).abs() / master_plain.abs().clamp_min(1e-30))[diff]
    same = bool(n_outside == 0 and n_diff <= 8 and (n_diff == 0 or float(rel.max()) <= 2.0 ** -6))
    np.savez(os.path.join(out_dir, f"mixed_world1_{backend}.npz"), loss_plain=loss_plain, loss_x=loss_x, same=same, nbytes=nbytes,
             n_diff=n_diff, nlaunch=nlaunch, n_params=model._flat.numel(), moved=bool((master_plain != start).any()),
             lo_ok=bool(torch.equal(model._flat, mx.master.to(torch.bfloat16))), exposed_ms=ev0.elapsed_time(ev1))
    if model.comm is not None:
        model.comm.close()
    dist.destroy_process_group()


@pytest.mark.parametrize("backend", ["torch", "mh"])
def test_rccl_world1_bucketed_exchange_over_the_fp32_accumulator(tmp_path, backend):
    """both exchange routes (torch.distributed's RCCL; mh_comm_allreduce with the fp32 dtype and mean=1) carry the fp32
    accumulator in buckets behind the backward of a real 16 x 2048 step: the coverage check of finish() holds on the fp32
    buffer, 4 bytes per parameter go out per optimiser step, and with one rank the master ends where the plain mixed step ends
    (under the forced-exchange test's own allowance for the embedding gradient's summation order)"""
    import torch.multiprocessing as mp
    mp.spawn(_worker_world1, args=(_free_port(), str(tmp_path), backend), nprocs=1, join=True)
    r = np.load(tmp_path / f"mixed_world1_{backend}.npz")
    assert int(r["nbytes"]) == 4 * int(r["n_params"]) == 2 * 467_685_376
    assert 14 <= int(r["nlaunch"]) <= 20, int(r["nlaunch"])         # (a bucket closes on a layer boundary: as many as in bf16)
    assert float(r["loss_plain"]) == float(r["loss_x"])
    assert bool(r["moved"]) and bool(r["lo_ok"])
    assert bool(r["same"]), int(r["n_diff"])
    assert float(r["exposed_ms"]) >= 0.0
