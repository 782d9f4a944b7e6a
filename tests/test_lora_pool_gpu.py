"""A LoRA adapter per request in the decode pool, end to end on the MI355X: production sessions with captured graphs, bf16, G = 4 slots
of rank 64, adapters of rank 8 and 64 saved in peft's layout with B drawn as randn * 0.05.

The model is the tiny 4-layer one of test_logp_pool_gpu.py with I = 1024 instead of 512: that model's token-level stack has I = 512 / 4
= 128, a contraction no skinny entry point serves, so its sessions run the unfused decode form, which takes no adapters by
construction (``ValueError``).  With I = 1024 the token-level I is 256 and both stacks run the fused folded form.

  ids         seeded: a LoRA pool whose requests name no adapter, and a request whose adapter has B = 0, return the plain pool's ids;
  neighbours  seeded: an adapted request alone, and among neighbours on other adapters and on none: ids and logprobs bit-equal;
  accuracy    e_lora = RMS over >= 60 generated events of logprobs(rid) minus the oracle's teacher-forced ll on fp32 W + s B A, against
              e_merged, the same for a plain bf16 pool on a model loaded with those merged weights: e_lora <= 1.5 e_merged (the RMS
              of 60 samples spreads by 1 / sqrt(120) = 9 %, the ratio of two by 13 %: 1.5 is beyond three of those), and the adapter
              matters: the oracle's ll on the base weights differs from that on the merged ones by >= 10 e_merged in RMS;
  fork        a child of an adapted request on its parent's seed repeats the parent;
  reload      unload_adapter then load_adapter of another adapter into the freed slot while other rows run: their ids are those of
              an undisturbed run, and the new adapter's request meets the accuracy bound."""
import json
import os

import numpy as np
import pytest
import torch

import midi_model_amd as mm

import fork_common as fc
import logp_common as lc
import ragged_common as rc

pytestmark = pytest.mark.gpu

CAP = 256
G, R = 4, 64
TARGETS = {"self_attn.q_proj": (0, 0), "self_attn.k_proj": (0, 0), "self_attn.v_proj": (0, 0), "self_attn.o_proj": (0, 0),
           "mlp.gate_proj": (1, 0), "mlp.up_proj": (1, 0), "mlp.down_proj": (0, 1)}   # (out is I, in is I)


@pytest.fixture(scope="module")
def tok():
    return mm.MIDITokenizerV2()


def make_model(sd):
    m = mm.MIDIModel(mm.MIDIModelConfig.get_config("v2", True, 4, 4, 256, 1024))
    m.load_state_dict(sd, strict=True)
    return m.to("cuda", torch.bfloat16).eval()


@pytest.fixture(scope="module")
def world(orc, tok, tmp_path_factory):
    """-> (shape, base state dict, base model, {name: (directory, merged fp32 state dict)})"""
    shp = orc.Shape(n_layer=4, n_head=4, n_embd=256, n_inner=1024, vocab=tok.vocab_size)
    sd = {k: v.to(torch.bfloat16).float() for k, v in orc.make_state_dict(shp, seed=0).items()}   # (what the bf16 model holds)
    from safetensors.torch import save_file
    root = tmp_path_factory.mktemp("adapters")
    ads = {}
    for name, r, alpha, bscale, seed in (("r8", 8, 16.0, 0.05, 1), ("r64", 64, 128.0, 0.05, 2), ("zero", 64, 128.0, 0.0, 3), ("late", 64, 128.0, 0.05, 4)):
        g = torch.Generator().manual_seed(seed)
        tensors, merged = {}, dict(sd)
        for stack, n_layer, inner in (("net", 4, 1024), ("net_token", 1, 256)):
            for li in range(n_layer):
                for t, (oi, ii) in TARGETS.items():
                    o, i = (inner if oi else 256), (inner if ii else 256)
                    A = ((torch.rand((r, i), generator=g) * 2 - 1) * i ** -0.5).to(torch.bfloat16)
                    B = (torch.randn((o, r), generator=g) * bscale).to(torch.bfloat16)
                    key = f"{stack}.layers.{li}.{t}"
                    tensors[f"base_model.model.{key}.lora_A.weight"], tensors[f"base_model.model.{key}.lora_B.weight"] = A, B
                    merged[key + ".weight"] = sd[key + ".weight"] + (alpha / r) * (B.float() @ A.float())
        d = str(root / name)
        os.makedirs(d)
        save_file(tensors, os.path.join(d, "adapter_model.safetensors"))
        with open(os.path.join(d, "adapter_config.json"), "w") as f:
            json.dump({"peft_type": "LORA", "r": r, "lora_alpha": alpha, "use_rslora": False, "fan_in_fan_out": False}, f)
        ads[name] = (d, merged)
    return shp, sd, make_model(sd), ads


def lora_pool(m, rows=4, **kw):
    return m.decode_pool(rows, CAP, lora_slots=G, lora_rank=R, **kw)


def test_no_adapter_and_a_zero_adapter_return_the_plain_ids(orc, tok, world):
    _, _, m, ads = world
    ps = rc.prompts(orc, tok, (6, 9, 3), seed0=810)

    def run(pool, adapter):
        ids = [pool.submit(p, max_len=len(p) + 10, seed=30 + k, adapter=adapter(k), **fc.KW) if adapter else
               pool.submit(p, max_len=len(p) + 10, seed=30 + k, **fc.KW) for k, p in enumerate(ps)]
        fc.drain(pool)
        return [pool.result(i) for i in ids]

    with m.decode_pool(4, CAP, seeded=True) as pool:
        want = run(pool, None)
    with lora_pool(m, seeded=True) as pool:
        assert pool.ses is None or pool.ses.g_net is not None
        got = run(pool, None)
        assert pool.ses.g_net is not None and pool.ses.g_steps is not None, "captured graphs"
    with lora_pool(m, seeded=True) as pool:
        pool.load_adapter(ads["r8"][0])
        z = pool.load_adapter(ads["zero"][0])
        zero = run(pool, lambda k: z)
    for a, b, c in zip(want, got, zero):
        assert fc.same(a, b) and fc.same(a, c)


def test_adapted_request_alone_and_among_neighbours(orc, tok, world):
    _, _, m, ads = world
    x, a, b = rc.prompts(orc, tok, (6, 9, 3), seed0=740)
    got = []
    for among in (False, True):
        with lora_pool(m, seeded=True, logprobs=True) as pool:
            a8, a64 = pool.load_adapter(ads["r8"][0]), pool.load_adapter(ads["r64"][0])
            if among:
                pool.submit(a, max_len=40, seed=21, adapter=a8, **fc.KW)
                pool.submit(b, max_len=40, seed=22, temp=0.7, top_k=3, ban_eos=True)
                pool.step()
            rid = pool.submit(x, max_len=16, seed=77, adapter=a64, **fc.KW)
            pool.step()
            assert pool.requests[rid].row == (2 if among else 0)
            while not pool.requests[rid].done:
                pool.step()
            got.append((pool.result(rid), pool.logprobs(rid)))
    with m.decode_pool(4, CAP, seeded=True) as pool:
        rid = pool.submit(x, max_len=16, seed=77, **fc.KW)
        fc.drain(pool)
        assert not fc.same(pool.result(rid), got[0][0]), "the adapter changes nothing"
    assert fc.same(got[0][0], got[1][0])
    assert got[0][1].shape == (10,) and (got[0][1].view(np.int32) == got[1][1].view(np.int32)).all(), (got[0][1], got[1][1])


def errors(orc, tok, shp, sd_ref, arity, results):
    """[(result, prompt length, logprobs)] -> the differences logprobs - oracle ll on ``sd_ref``, all events"""
    out = []
    for res, first, lp in results:
        want, _ = lc.oracle_ll(orc, tok, sd_ref, shp, res, first, arity)
        out.append(lp.astype(np.float64) - want)
    return np.concatenate(out)


def rms(x):
    return float(np.sqrt(np.mean(np.square(x))))


def accuracy(orc, tok, world, name, run_lora, label):
    shp, sd, m, ads = world
    merged = ads[name][1]
    arity = m._grammar()[3]
    ps = rc.prompts(orc, tok, (5, 8, 3), seed0=860)
    res_lora = run_lora(ps)
    mm_merged = make_model(merged)
    with mm_merged.decode_pool(4, CAP, logprobs=True, generator=torch.Generator(device="cuda").manual_seed(5)) as pool:
        ids = [pool.submit(p, max_len=len(p) + 24, ban_eos=True, **lc.KW) for p in ps]
        fc.drain(pool)
        res_merged = [(pool.result(i), len(p), pool.logprobs(i)) for i, p in zip(ids, ps)]
    d_lora, d_merged = errors(orc, tok, shp, merged, arity, res_lora), errors(orc, tok, shp, merged, arity, res_merged)
    assert len(d_lora) >= 60 and len(d_merged) >= 60
    e_lora, e_merged = rms(d_lora), rms(d_merged)
    base = np.concatenate([lc.oracle_ll(orc, tok, sd, shp, r, f, arity)[0] - lc.oracle_ll(orc, tok, merged, shp, r, f, arity)[0]
                           for r, f, _ in res_lora])
    print(f"{label}: e_lora {e_lora:.4e}  e_merged {e_merged:.4e}  ratio {e_lora / e_merged:.3f}  base against merged {rms(base):.4e}")
    assert rms(base) >= 10 * e_merged, (rms(base), e_merged)
    assert e_lora <= 1.5 * e_merged, (e_lora, e_merged)


@pytest.mark.parametrize("name", ["r8", "r64"])
def test_logprobs_against_the_oracle_on_the_merged_weights(orc, tok, world, name):
    """measured on one MI355X: printed by the test (DESIGN 7.13 records the values)"""
    m, ads = world[2], world[3]

    def run_lora(ps):
        with lora_pool(m, logprobs=True, generator=torch.Generator(device="cuda").manual_seed(5)) as pool:
            pool.load_adapter(ads["zero"][0])
            aid = pool.load_adapter(ads[name][0])
            ids = [pool.submit(p, max_len=len(p) + 24, ban_eos=True, adapter=aid, **lc.KW) for p in ps]
            fc.drain(pool)
            return [(pool.result(i), len(p), pool.logprobs(i)) for i, p in zip(ids, ps)]

    accuracy(orc, tok, world, name, run_lora, name)


def test_a_child_on_its_parents_seed_repeats_the_adapted_parent(orc, tok, world):
    m, ads = world[2], world[3]
    p, q = rc.prompts(orc, tok, (7, 9), seed0=500)
    with lora_pool(m, seeded=True) as pool:
        a8, a64 = pool.load_adapter(ads["r8"][0]), pool.load_adapter(ads["r64"][0])
        par = pool.submit(p, max_len=30, seed=77, adapter=a64, **fc.KW)
        pool.submit(q, max_len=25, seed=5, adapter=a8, **fc.KW)
        for _ in range(3):
            pool.step()
        a, b = pool.fork(par, count=2, seed=[77, 78])
        assert pool.requests[a].adapter == a64 and pool.ses.row_adapter.cpu().tolist() == [pool.adapters[a64], pool.adapters[a8]] + [pool.adapters[a64]] * 2
        with pytest.raises(ValueError):
            pool.unload_adapter(a64)
        fc.drain(pool)
        out = [pool.result(r) for r in (par, a, b)]
        assert pool.ses.row_adapter.cpu().tolist() == [-1] * 4, "release clears the row's adapter"
        # a held parent, forked later with a larger max_len
        h = pool.submit(p, max_len=12, seed=9, adapter=a64, hold=True, **fc.KW)
        fc.drain(pool)
        c, = pool.fork(h, max_len=20, seed=9)
        fc.drain(pool)
        held_child = pool.result(c)
        u = pool.submit(p, max_len=20, seed=9, adapter=a64, **fc.KW)
        fc.drain(pool)
        assert fc.same(held_child, pool.result(u)), "held then forked == uninterrupted"
    assert fc.same(out[1], out[0]) and (out[2][10:] != out[0][10:]).any()


def test_reload_into_a_freed_slot_while_other_rows_run(orc, tok, world):
    m, ads = world[2], world[3]
    x, y = rc.prompts(orc, tok, (6, 4), seed0=900)

    def running(pool, disturb):
        a8 = pool.load_adapter(ads["r8"][0])
        a64 = pool.load_adapter(ads["r64"][0])
        r1 = pool.submit(x, max_len=40, seed=1, adapter=a8, **fc.KW)
        r2 = pool.submit(y, max_len=40, seed=2, **fc.KW)
        for _ in range(4):
            pool.step()
        late = None
        if disturb:
            slot = pool.adapters[a64]
            pool.unload_adapter(a64)
            late = pool.load_adapter(ads["late"][0])
            assert pool.adapters[late] == slot
        while not (pool.requests[r1].done and pool.requests[r2].done):
            pool.step()
        return [pool.result(r1), pool.result(r2)], late

    with lora_pool(m, seeded=True) as pool:
        want, _ = running(pool, False)
    with lora_pool(m, seeded=True) as pool:
        got, _ = running(pool, True)
    assert fc.same(want[0], got[0]) and fc.same(want[1], got[1])

    def run_lora(ps):
        with lora_pool(m, logprobs=True, generator=torch.Generator(device="cuda").manual_seed(5)) as pool:
            a8, a64 = pool.load_adapter(ads["r8"][0]), pool.load_adapter(ads["r64"][0])
            bg = pool.submit(x, max_len=200, ban_eos=True, adapter=a8, **lc.KW)
            pool.step()
            pool.unload_adapter(a64)
            late = pool.load_adapter(ads["late"][0])
            ids = [pool.submit(p, max_len=len(p) + 24, ban_eos=True, adapter=late, **lc.KW) for p in ps]
            while not all(pool.requests[i].done for i in ids):
                pool.step()
            assert not pool.requests[bg].done
            return [(pool.result(i), len(p), pool.logprobs(i)) for i, p in zip(ids, ps)]

    accuracy(orc, tok, world, "late", run_lora, "late (reloaded slot)")
