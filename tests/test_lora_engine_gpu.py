"""engine.stack_decode(lora=...) on the MI355X: a LoRA adapter per row, unmerged, on both stacks of a tiny 4-layer model (D = 256,
I = 1024, so that the token-level stack's I = 256 is a contraction the skinny kernels serve; bf16; G = 4 slots of rank 64; adapters of
rank 8 and 64, B drawn as randn * 0.05).

  none        every row without adapter: the bits of stack_decode without ``lora`` -- outputs and K/V cache, narrow and wide,
              with the layer-0 embedding gather of the token stack;
  neighbours  a row's output and cache do not depend on the adapters of the other rows (bit-equal), and a slot whose B is zero
              gives the bits of no adapter;
  accuracy    one step from an empty cache (softmax over one key: o = v), against float64 on W + s B A:  e_lora, the RMS error of
              the unmerged form, against the yardstick e_merged, the same for the plain form on weights merged in fp32 and rounded
              to bf16 -- how an adapter is served without this form.  e_lora <= 1.5 e_merged: the RMS of n >= 16384 values
              spreads by 1 / sqrt(2 n) < 1 %, so 1.5 is far outside the noise of the ratio, and the unmerged form rounds only T
              where merging rounds the whole weight, so the ratio should sit near or below 1.  The adapters must matter: float64
              on the base weights differs from float64 on the merged ones by at least 10 e_merged."""
import pytest
import torch

import midi_model_amd as mm
from midi_model_amd import engine

pytestmark = pytest.mark.gpu

G, R = 4, 64
BF16 = torch.bfloat16
TARGETS = tuple(engine.LORA_PROJ)


def dims(spec):
    D, I = spec.D, spec.I
    return dict(q_proj=(D, D), k_proj=(D, D), v_proj=(D, D), o_proj=(D, D), gate_proj=(I, D), up_proj=(I, D), down_proj=(D, I))


@pytest.fixture(scope="module")
def model(orc):
    tok = mm.MIDITokenizerV2()
    shp = orc.Shape(n_layer=4, n_head=4, n_embd=256, n_inner=1024, vocab=tok.vocab_size)
    m = mm.MIDIModel(mm.MIDIModelConfig.get_config("v2", True, 4, 4, 256, 1024))
    m.load_state_dict(orc.make_state_dict(shp, seed=0), strict=True)
    return m.to("cuda", BF16).eval()


def adapter(spec, n_layers, r, targets, seed, zero_b=False):
    g, dm = torch.Generator().manual_seed(seed), dims(spec)
    return [{t: ((torch.rand((r, dm[t][1]), generator=g) * 2 - 1).mul(dm[t][1] ** -0.5).to(BF16).cuda(),
                 (torch.randn((dm[t][0], r), generator=g) * (0.0 if zero_b else 0.05)).to(BF16).cuda()) for t in targets}
            for _ in range(n_layers)]


ADAPTERS = {0: (8, TARGETS, 2.0), 1: (64, ("q_proj", "v_proj", "down_proj"), 2.0), 2: (64, TARGETS, 2.0)}   # slot 3: B = 0


def loaded(model, name, B):
    spec, W = model._specs[name], model._W[name]
    st = engine.LoraStack(spec, len(W.layers), G, R, B, model._flat)
    ads = {g: (adapter(spec, len(W.layers), r, t, 10 + g), s) for g, (r, t, s) in ADAPTERS.items()}
    ads[3] = (adapter(spec, len(W.layers), 64, TARGETS, 13, zero_b=True), 2.0)
    for g, (ad, s) in ads.items():
        st.load_slot(g, ad, s)
    st.refresh(W)
    return st, ads


def run(model, name, st, x, B, steps=2, x_ids=None, adapters=None):
    """`steps` eager decode steps from an empty cache -> (outputs per step, K cache, V cache)"""
    spec, W = model._specs[name], model._W[name]
    fold = engine.fold_norm_weights(W)
    kv, rope = engine.KVState(spec, B, 8, model._flat), engine.RopeTable(spec.hd, spec.theta, "cuda", 8)
    kv.k.zero_()
    kv.v.zero_()
    if st is not None:
        st.row_adapter.copy_(torch.as_tensor(adapters, dtype=torch.int32))
    outs = []
    for s in range(steps):
        xs = x[s]
        outs.append(engine.stack_decode(spec, W, W.embed if x_ids is not None else xs, rope, kv, folded=fold,
                                        x_ids=None if x_ids is None else x_ids[s], lora=st).clone())
    torch.cuda.synchronize()
    return torch.stack(outs), kv.k[:, :, :, :steps].clone(), kv.v[:, :, :, :steps].clone()


def inputs(B, D, steps=2, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn((B, D), generator=g).to(BF16).cuda() for _ in range(steps)]


@pytest.mark.parametrize("name,B,gather", [("net", 6, False), ("net", 70, False), ("net_token", 5, True), ("net_token", 130, True)])
def test_rows_without_adapter_keep_the_bits_of_the_plain_form(model, name, B, gather):
    with torch.inference_mode():
        st, _ = loaded(model, name, B)
        x = inputs(B, 256)
        ids = [(torch.arange(B, device="cuda") * 37 + 11 * s) % model._W[name].embed.shape[0] for s in range(2)] if gather else None
        want = run(model, name, None, x, B, x_ids=ids)
        got = run(model, name, st, x, B, x_ids=ids, adapters=[-1] * B)
        for a, b in zip(got, want):
            assert bool((a == b).all())


@pytest.mark.parametrize("name,B", [("net", 6), ("net_token", 70)])
def test_a_row_does_not_see_its_neighbours_adapters(model, name, B):
    with torch.inference_mode():
        st, _ = loaded(model, name, B)
        x = inputs(B, 256)
        mixed = [(-1, 0, 1, 2, 3)[(b * 3 + 1) % 5] for b in range(B)]
        got = run(model, name, st, x, B, adapters=mixed)
        plain = run(model, name, None, x, B)
        for g in (0, 1, 2):
            alone = run(model, name, st, x, B, adapters=[g] * B)
            rows = [b for b in range(B) if mixed[b] == g]
            assert rows
            for a, b in zip(got, alone):
                assert torch.equal(a[:, rows], b[:, rows])      # (outputs [steps, B, D], caches [L, B, H, steps, hd])
            assert not torch.equal(alone[0], plain[0]), "the adapter changes nothing"
        rows = [b for b in range(B) if mixed[b] in (-1, 3)]       # no adapter, and the slot whose B is zero
        for a, b in zip(got, plain):
            assert bool((a[:, rows] == b[:, rows]).all())


def eff64(model, name, ads, g):
    """float64 effective weights of slot g (None: the base) per layer: (wqkv, wo, wgu, wd, n1, n2)"""
    out = []
    for li, lw in enumerate(model._W[name].layers):
        w = dict(qkv=lw.wqkv.double().cpu().clone(), o=lw.wo.double().cpu().clone(), gu=lw.wgu.double().cpu().clone(), d=lw.wd.double().cpu().clone())
        if g is not None:
            ad, s = ads[g]
            for t, (A, Bm) in ad[li].items():
                proj, part = engine.LORA_PROJ[t]
                n = dims(model._specs[name])[t][0]
                w[proj][part * n:(part + 1) * n] += s * (Bm.double().cpu() @ A.double().cpu())
        out.append((w["qkv"], w["o"], w["gu"], w["d"], lw.n1.double().cpu(), lw.n2.double().cpu()))
    return out


def step64(model, name, layers, x):
    """one decode step from an empty cache in float64: attention over the one key is the value itself"""
    spec = model._specs[name]
    x = x.double().cpu()
    rms = lambda t, w: t * torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + spec.eps) * w      # noqa: E731
    for wqkv, wo, wgu, wd, n1, n2 in layers:
        v = rms(x, n1) @ wqkv[2 * spec.D:].T
        x = x + v @ wo.T
        gu = rms(x, n2) @ wgu.T
        x = x + (torch.nn.functional.silu(gu[:, :spec.I]) * gu[:, spec.I:]) @ wd.T
    return rms(x, model._W[name].norm.double().cpu())


def test_unmerged_is_as_close_to_float64_as_merged_bf16_weights(model):
    name, B = "net", 64
    spec, W = model._specs[name], model._W[name]
    with torch.inference_mode():
        st, ads = loaded(model, name, B)
        x = inputs(B, 256, steps=1, seed=9)
        worst = 0.0
        for g in (0, 1, 2):
            layers = eff64(model, name, ads, g)
            ref = step64(model, name, layers, x[0])
            base = step64(model, name, eff64(model, name, ads, None), x[0])
            got = run(model, name, st, x, B, steps=1, adapters=[g] * B)[0][0].double().cpu()
            Wm = engine.StackTensors(embed=W.embed, norm=W.norm, layers=[
                engine.LayerTensors(wqkv=l[0].float().to(BF16).cuda(), wo=l[1].float().to(BF16).cuda(), wgu=l[2].float().to(BF16).cuda(),
                                    wd=l[3].float().to(BF16).cuda(), n1=lw.n1, n2=lw.n2) for l, lw in zip(layers, W.layers)])
            kv, rope = engine.KVState(spec, B, 8, model._flat), engine.RopeTable(spec.hd, spec.theta, "cuda", 8)
            merged = engine.stack_decode(spec, Wm, x[0], rope, kv, folded=engine.fold_norm_weights(Wm)).double().cpu()
            rmsd = lambda a, b: float((a - b).pow(2).mean().sqrt())      # noqa: E731
            e_lora, e_merged, moved = rmsd(got, ref), rmsd(merged, ref), rmsd(base, ref)
            print(f"slot {g}: e_lora {e_lora:.3e}  e_merged {e_merged:.3e}  ratio {e_lora / e_merged:.3f}  base-merged {moved:.3e}")
            assert moved >= 10 * e_merged, f"slot {g}: the adapter moves the output by {moved:.3e}, e_merged is {e_merged:.3e}"
            worst = max(worst, e_lora / e_merged)
            assert e_lora <= 1.5 * e_merged, f"slot {g}: e_lora {e_lora:.3e} > 1.5 x e_merged {e_merged:.3e}"
