"""engine.LoraStack on the CPU: where an adapter's matrices land in the stacked buffers (zero padding for a rank below R and for
targets the adapter lacks), that the stacks reproduce x (W + s B A)^T row by row through the shrink / expand algebra the kernels
run, the norm fold of ``refresh``, and the refusals -- every ValueError before any kernel call."""
import pytest
import torch

from midi_model_amd import engine

D, I, L, G, R = 256, 512, 2, 4, 64
BF16 = torch.bfloat16


def spec():
    return engine.StackSpec("net", D, 4, I, L, 1e-5, 10000.0, "event")


def adapter(r, targets, seed):
    g = torch.Generator().manual_seed(seed)
    dims = dict(q_proj=(D, D), k_proj=(D, D), v_proj=(D, D), o_proj=(D, D), gate_proj=(I, D), up_proj=(I, D), down_proj=(D, I))
    return [{t: ((torch.randn((r, dims[t][1]), generator=g) * dims[t][1] ** -0.5).to(BF16), (torch.randn((dims[t][0], r), generator=g) * 0.05).to(BF16))
             for t in targets} for _ in range(L)]


def test_slots_padding_and_missing_targets():
    st = engine.LoraStack(spec(), L, G, R, 5, torch.empty(1, dtype=BF16))
    full, part = adapter(8, tuple(engine.LORA_PROJ), 1), adapter(64, ("q_proj", "v_proj", "down_proj"), 2)
    st.load_slot(2, full, 2.0)
    st.load_slot(0, part, 0.5)
    assert st.slot_scale.tolist() == [0.5, 0.0, 2.0, 0.0] and st.row_adapter.tolist() == [-1] * 5
    for li in range(L):
        a, b = st.a[li], st.b[li]
        for name, (proj, p) in engine.LORA_PROJ.items():
            out = b[proj].shape[0] // {"qkv": 3, "gu": 2}.get(proj, 1)
            rows = a[proj].view(-1, G, R, a[proj].shape[1])[p]          # [slot][R][in]
            cols = b[proj][p * out:(p + 1) * out].view(out, G, R)        # [out][slot][R]
            A2, B2 = full[li][name]
            assert torch.equal(rows[2, :8], A2) and not rows[2, 8:].any() and torch.equal(cols[:, 2, :8], B2) and not cols[:, 2, 8:].any()
            if name in part[li]:
                assert torch.equal(rows[0], part[li][name][0]) and torch.equal(cols[:, 0], part[li][name][1])
            else:
                assert not rows[0].any() and not cols[:, 0].any()
            assert not rows[1].any() and not rows[3].any() and not cols[:, 1].any() and not cols[:, 3].any()
    # a slot is overwritten whole: the smaller adapter leaves nothing of the larger one behind
    st.load_slot(2, part, 1.0)
    assert not st.a[0]["o"].any() and not st.b[0]["gu"].view(2 * I, G, R)[:, 2].any()


def test_stacks_reproduce_the_merged_projection_row_by_row():
    st = engine.LoraStack(spec(), L, G, R, 6, torch.empty(1, dtype=BF16))
    ads = {0: (adapter(8, tuple(engine.LORA_PROJ), 3), 2.0), 3: (adapter(64, tuple(engine.LORA_PROJ), 4), 0.5)}
    for g_, (ad, s) in ads.items():
        st.load_slot(g_, ad, s)
    ra = torch.tensor([3, -1, 0, 0, 1, 3])
    x = torch.randn((6, D), generator=torch.Generator().manual_seed(5)).double()
    slot = (torch.arange(3 * G * R) // R) % G
    a, b = st.a[1]["qkv"].double(), st.b[1]["qkv"].double()
    t = torch.where(ra[:, None] == slot[None, :], st.slot_scale.double()[slot][None, :] * (x @ a.T), torch.zeros((), dtype=torch.float64))
    got = torch.cat([t[:, p * G * R:(p + 1) * G * R] @ b[p * D:(p + 1) * D].T for p in range(3)], 1)
    for m, g_ in enumerate(ra.tolist()):
        want = torch.zeros(3 * D, dtype=torch.float64)
        if g_ in ads:
            ad, s = ads[g_]
            want = torch.cat([s * (ad[1][n][1].double() @ (ad[1][n][0].double() @ x[m])) for n in ("q_proj", "k_proj", "v_proj")])
        assert torch.allclose(got[m], want, rtol=1e-12, atol=1e-12), m


def test_refresh_folds_the_norm_weights_into_the_a_stacks():
    st = engine.LoraStack(spec(), L, G, R, 3, torch.empty(1, dtype=BF16))
    st.load_slot(1, adapter(64, tuple(engine.LORA_PROJ), 6), 2.0)
    g = torch.Generator().manual_seed(7)
    W = engine.StackTensors(layers=[engine.LayerTensors(n1=(1 + 0.1 * torch.randn(D, generator=g)).to(BF16), n2=(1 + 0.1 * torch.randn(D, generator=g)).to(BF16))
                                    for _ in range(L)])
    st.refresh(W)
    for li in range(L):
        assert torch.equal(st.a_n[li][0], (st.a[li]["qkv"].float() * W.layers[li].n1.float()[None]).to(BF16))
        assert torch.equal(st.a_n[li][1], (st.a[li]["gu"].float() * W.layers[li].n2.float()[None]).to(BF16))


def test_refusals_come_before_any_call(monkeypatch):
    like = torch.empty(1, dtype=BF16)
    for kw in (dict(G=3, R=64), dict(G=4, R=60), dict(G=0, R=64)):
        with pytest.raises(ValueError):
            engine.LoraStack(spec(), L, kw["G"], kw["R"], 4, like)
    with pytest.raises(ValueError):
        engine.LoraStack(spec(), L, G, R, 4, torch.empty(1))            # fp32
    with pytest.raises(ValueError):
        engine.LoraStack(spec(), L, G, R, 257, like)
    st = engine.LoraStack(spec(), L, G, R, 4, like)
    before = [t.clone() for t in (st.a[0]["qkv"], st.b[0]["qkv"], st.slot_scale)]
    bad = adapter(64, ("q_proj",), 8)
    bad[1]["lm_head"] = bad[1]["q_proj"]
    for layers, g_ in ((bad, 0), (adapter(128, ("q_proj",), 9), 0), (adapter(64, ("q_proj",), 9), 4), (adapter(64, ("q_proj",), 9)[:1], 0)):
        with pytest.raises(ValueError):
            st.load_slot(g_, layers, 1.0)
    assert all(torch.equal(x, y) for x, y in zip(before, (st.a[0]["qkv"], st.b[0]["qkv"], st.slot_scale))), "a refused load wrote"
    # stack_decode: anything but the fused folded form is refused before the first kernel call
    calls = []
    import midi_model_amd.lib as lib

    class NoLib:
        def call(self, name, *a):
            calls.append(name)
            raise AssertionError(f"{name} was called")
    monkeypatch.setattr(lib, "_lib", NoLib())
    import midi_model_amd.ops as ops
    monkeypatch.setattr(ops, "lib", lambda: NoLib())
    sp = spec()
    W = engine.StackTensors(layers=[engine.LayerTensors() for _ in range(L)])
    kv = engine.KVState(sp, 4, 8, like)
    rope = engine.RopeTable(sp.hd, sp.theta, "cpu", 8)
    x = torch.zeros((4, D), dtype=BF16)
    with pytest.raises(ValueError, match="fused folded"):
        engine.stack_decode(sp, W, x, rope, kv, lora=st)                                  # no folded weights
    with pytest.raises(ValueError, match="fused folded"):
        engine.stack_decode(sp, W, x.float(), rope, kv, folded=[(None, None)] * L, lora=st)   # fp32
    with pytest.raises(ValueError, match="rows"):
        engine.stack_decode(sp, W, x[:3], rope, engine.KVState(sp, 3, 8, like), folded=[(None, None)] * L, lora=st)
    assert st.dirty     # loaded into (at construction: never folded) and not refreshed: the folded A stacks are stale
    with pytest.raises(ValueError, match="not refreshed"):
        engine.stack_decode(sp, W, x, rope, kv, folded=[(None, None)] * L, lora=st)
    assert calls == []
