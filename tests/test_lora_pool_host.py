"""A LoRA adapter per request on the CPU: DecodePool.load_adapter / unload_adapter / submit(adapter=), DecodeSession(lora_slots=) and
its admit / fork / release, through the fake backend plus the stand-ins of tests/emu_lora.py.  Tiny 4-layer bf16 model with I = 1024
(the token-level I = 256 is a contraction the fused decode form serves; with I = 512 it is 128 and the session is refused).  The
kernels: test_lora_kernels_gpu.py; the production session: test_lora_pool_gpu.py."""
import json
import os

import pytest
import torch

import midi_model_amd as mm
from midi_model_amd.decode import DecodeSession

import emu_kvq
import emu_lora
import fork_common as fc
import ragged_common as rc

G, R = 4, 64
LORA_OPS = ("lora_shrink_rows", "gemm_skinny_ext")
MODS = {"self_attn.q_proj": (0, 0), "self_attn.v_proj": (0, 0), "mlp.up_proj": (1, 0), "mlp.down_proj": (0, 1)}


@pytest.fixture(scope="module")
def tok():
    return mm.MIDITokenizerV2()


@pytest.fixture(scope="module")
def tiny(orc, tok):
    shp = orc.Shape(n_layer=4, n_head=4, n_embd=256, n_inner=1024, vocab=tok.vocab_size)
    return shp, orc.make_state_dict(shp, seed=0)


def _model(sd, dtype=torch.bfloat16, inner=1024):
    m = mm.MIDIModel(mm.MIDIModelConfig.get_config("v2", True, 4, 4, 256, inner))
    m.load_state_dict(sd)
    return m.to(dtype)


def save_adapter(d, r, mods=MODS, extra=None, seed=1):
    """a directory in peft's layout; targets ``mods`` on every layer of both stacks"""
    from safetensors.torch import save_file
    g = torch.Generator().manual_seed(seed)
    tensors = {}
    for stack, n_layer, inner in (("net", 4, 1024), ("net_token", 1, 256)):
        for li in range(n_layer):
            for t, (oi, ii) in mods.items():
                o, i = (inner if oi else 256), (inner if ii else 256)
                key = f"base_model.model.{stack}.layers.{li}.{t}"
                tensors[key + ".lora_A.weight"] = (torch.randn((r, i), generator=g) * i ** -0.5).to(torch.bfloat16)
                tensors[key + ".lora_B.weight"] = (torch.randn((o, r), generator=g) * 0.05).to(torch.bfloat16)
    tensors.update(extra or {})
    os.makedirs(d, exist_ok=True)
    save_file(tensors, os.path.join(d, "adapter_model.safetensors"))
    with open(os.path.join(d, "adapter_config.json"), "w") as f:
        json.dump({"peft_type": "LORA", "r": r, "lora_alpha": 2.0 * r, "use_rslora": False}, f)
    return str(d)


def test_refusals_come_before_any_call(orc, tok, tiny, tmp_path):
    p = rc.prompts(orc, tok, (5,), seed0=600)[0]
    ok8 = save_adapter(tmp_path / "r8", 8)
    big = save_adapter(tmp_path / "r128", 128)
    bad = save_adapter(tmp_path / "bad", 8, extra={"base_model.model.lm_head.lora_A.weight": torch.zeros((8, 256)),
                                                    "base_model.model.lm_head.lora_B.weight": torch.zeros((64, 8))})
    with emu_lora.install() as log:
        m, m32 = _model(tiny[1]), _model(tiny[1], torch.float32)
        del log[:]
        for kw, match in ((dict(lora_slots=3, lora_rank=64), "multiple of 256"), (dict(lora_slots=4, lora_rank=60), "multiple of 8"),
                          (dict(lora_slots=4, lora_rank=64, rows=257), "256 rows")):
            with pytest.raises(ValueError, match=match):
                m.decode_pool(kw.pop("rows", 4), 64, **kw)
        with pytest.raises(ValueError, match="bf16 model"):
            m32.decode_pool(4, 64, lora_slots=4, lora_rank=64)
        with pytest.raises(ValueError, match="row_params"):
            DecodeSession(m, 4, 256, 1.0, 0.98, 1, ragged=True, lora_slots=4)
        with m.decode_pool(4, 64) as pool:
            with pytest.raises(ValueError, match="no adapter slots"):
                pool.load_adapter(ok8)
            with pytest.raises(ValueError, match="not loaded"):
                pool.submit(p, adapter=0)
        assert log == [], log
        with m.decode_pool(4, 64, lora_slots=G, lora_rank=R) as pool:
            pool.load_adapter(ok8)                      # (takes the session: its construction and warm-up are logged)
            del log[:]
            with pytest.raises(ValueError, match="rank 128"):
                pool.load_adapter(big)
            with pytest.raises(ValueError, match="lm_head"):
                pool.load_adapter(bad)
            with pytest.raises(ValueError, match="not loaded"):
                pool.submit(p, adapter=7)
            with pytest.raises(ValueError, match="adapter"):
                pool.ses.admit([0], torch.from_numpy(p), [5], [20], [1.0], [0.9], [5], torch.zeros((1, pool.ses.V), dtype=torch.uint8),
                               torch.zeros((1, pool.ses.V), dtype=torch.uint8), adapter=2)
            for _ in range(3):
                pool.load_adapter(ok8)
            with pytest.raises(ValueError, match="slots are taken"):
                pool.load_adapter(ok8)
            assert not [n for n in log if n in LORA_OPS + ("gemm_nt", "gemm_skinny")], log


def test_slots_padding_admissions_forks_and_unload(orc, tok, tiny, tmp_path):
    ps = rc.prompts(orc, tok, (5, 3, 6, 4), seed0=610)
    d8, d64 = save_adapter(tmp_path / "r8", 8, seed=1), save_adapter(tmp_path / "r64", 64, mods={"self_attn.q_proj": (0, 0)}, seed=2)
    with emu_lora.install() as log:
        m = _model(tiny[1])
        with m.decode_pool(4, 64, seeded=True, lora_slots=G, lora_rank=R) as pool:
            a8, a64 = pool.load_adapter(d8), pool.load_adapter(d64)
            ses = pool.ses
            assert pool.adapters == {a8: 0, a64: 1} and ses.lora1.slot_scale.tolist() == [2.0, 2.0, 0.0, 0.0]
            # padding for r < R and for the targets an adapter lacks
            q = ses.lora1.a[0]["qkv"].view(3, G, R, 256)
            assert q[0, 0, :8].any() and not q[0, 0, 8:].any() and not q[1, 0].any() and q[2, 0, :8].any()      # r8: q and v, no k
            assert q[0, 1].any() and not q[2, 1].any() and not ses.lora1.a[0]["d"].view(G, R, 1024)[1].any()    # r64: q alone
            assert not ses.lora1.dirty and not ses.lora2.dirty and ses.lora2.a[0]["qkv"].view(3, G, R, 256)[0, 0, :8].any()
            # one admit per adapter, in the order the adapters first appear
            seen = []
            real_admit = ses.admit
            ses.admit = lambda rows, *a, **k: (seen.append((list(rows), k.get("adapter"))), real_admit(rows, *a, **k))[1]
            ids = [pool.submit(p, max_len=len(p) + 6, seed=k, adapter=ad, **fc.KW) for k, (p, ad) in enumerate(zip(ps, (a64, None, a64, a8)))]
            del log[:]
            pool.step()
            assert seen == [([0, 2], 1), ([1], None), ([3], 0)], seen
            assert ses.row_adapter.tolist() == [1, -1, 1, 0]
            assert "gemm_nt" in log and log.count("lora_shrink_rows") == log.count("gemm_skinny_ext") > 0
            with pytest.raises(ValueError, match="named by requests"):
                pool.unload_adapter(a64)
            fc.drain(pool)
            assert ses.row_adapter.tolist() == [-1] * 4
            # a fork child inherits its parent's adapter; a held request keeps naming it
            par = pool.submit(ps[0], max_len=12, seed=3, adapter=a8, hold=True, **fc.KW)
            pool.step()
            kid, = pool.fork(par, seed=3)
            assert pool.requests[kid].adapter == a8 and ses.row_adapter.tolist()[:2] == [0, 0]
            fc.drain(pool)
            assert fc.same(pool.result(kid), pool.result(par)) and pool.held() == [par]
            with pytest.raises(ValueError, match="named by requests"):
                pool.unload_adapter(a8)
            pool.drop(par)
            pool.unload_adapter(a8)
            assert pool.adapters == {a64: 1} and ses.lora1.slot_scale.tolist() == [0.0, 2.0, 0.0, 0.0]
            assert not ses.lora1.a[0]["qkv"].view(3, G, R, 256)[:, 0].any() and not ses.lora1.b[0]["qkv"].view(768, G, R)[:, 0].any()
            assert pool.load_adapter(d8) == 2 and pool.adapters[2] == 0


def test_a_pool_without_slots_logs_what_it_logged_and_no_adapter_gives_its_ids(orc, tok, tiny):
    ps = rc.prompts(orc, tok, (5, 3, 6), seed0=620)

    def run(m, **kw):
        with m.decode_pool(4, 64, seeded=True, **kw) as pool:
            ids = [pool.submit(p, max_len=len(p) + 5, seed=k, **fc.KW) for k, p in enumerate(ps)]
            fc.drain(pool)
            return [pool.result(i) for i in ids]

    with emu_kvq.install() as log:
        want = run(_model(tiny[1]))
        before = list(log)
    with emu_lora.install() as log:
        m = _model(tiny[1])
        got = run(m)
        assert list(log) == before and not [n for n in log if n in LORA_OPS]
        del log[:]
        lora = run(m, lora_slots=G, lora_rank=R)
        assert log.count("lora_shrink_rows") == log.count("gemm_skinny_ext") > 0 and "gemm_skinny" in log   # (lm_head stays plain)
    for a, b, c in zip(want, got, lora):
        assert fc.same(a, b) and fc.same(a, c)
