#!/usr/bin/env python
"""Same-process A/B of the decode step with a LoRA adapter per row, unmerged (engine.stack_decode(lora=...)), at the
level it exists: ONE step of a decoder stack of bf16 tv2o-medium over ``--rows`` rows standing at position ``--pos`` of their caches,
replayed from a captured graph (a decode session's form), the arms alternating:

  plain     stack_decode on the folded weights: 5 launches per layer;
  none      the same step with a LoraStack of G = 4 slots of rank 64 and NO row adapted: the price of the option (9 launches per layer);
  robin     the four slots loaded (rank 64, every target) and the rows adapted round-robin.

Both stacks: "net" (12 layers, once per event) and "net_token" (3 layers, eight times per event, here one of them).  Reports the
median and the fastest replay in microseconds per arm, and each kernel pair alone (shrink, projection with and without the second
operand pair) for the four projections of a layer.  One JSON line on stdout (and in --out).
usage: tools/bench_lora_decode.py [--rows 64] [--pos 256] [--reps 200] [--trials 5] [--out FILE].
Result: profiles/lora_decode_ab.txt (DESIGN 7.13 quotes it)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import midi_model_amd as mm  # noqa: E402
from midi_model_amd import engine, ops  # noqa: E402

G, R = 4, 64


def adapter(spec, n_layers, seed):
    g = torch.Generator().manual_seed(seed)
    D, I = spec.D, spec.I
    dims = dict(q_proj=(D, D), k_proj=(D, D), v_proj=(D, D), o_proj=(D, D), gate_proj=(I, D), up_proj=(I, D), down_proj=(D, I))
    return [{t: ((torch.randn((R, i), generator=g) * i ** -0.5).bfloat16().cuda(), (torch.randn((o, R), generator=g) * 0.02).bfloat16().cuda())
             for t, (o, i) in dims.items()} for _ in range(n_layers)]


def timed(graph, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        graph.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def capture(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def stack_arms(model, name, rows, pos):
    spec, W = model._specs[name], model._W[name]
    fold = engine.fold_norm_weights(W)
    cap = pos + 8
    kv, rope = engine.KVState(spec, rows, cap, model._flat), engine.RopeTable(spec.hd, spec.theta, "cuda", cap)
    kv.k.normal_()
    kv.v.normal_()
    x = torch.randn((rows, spec.D), device="cuda").bfloat16()
    pos_dev = torch.full((1,), pos, dtype=torch.int32, device="cuda")
    st = engine.LoraStack(spec, len(W.layers), G, R, rows, model._flat)
    st.refresh(W)
    out = torch.empty_like(x)

    def step(lora):
        if name == "net":   # the position from device memory, as a session's captured event step reads it
            return engine.stack_decode(spec, W, x, rope, kv, pos_dev=pos_dev, folded=fold, out=out, lora=lora)
        kv.len = pos        # (a session's token steps carry their position in the graph)
        return engine.stack_decode(spec, W, x, rope, kv, folded=fold, out=out, lora=lora)

    arms = {"plain": capture(lambda: step(None)), "lora": capture(lambda: step(st))}
    return arms, st, W


def kernels_alone(model, rows, reps):
    """us per launch of the shrink, the plain projection and the projection with the second operand pair (event-level layer 0)"""
    spec, lw = model._specs["net"], model._W["net"].layers[0]
    D, I, GR = spec.D, spec.I, G * R
    ra = (torch.arange(rows, device="cuda") % G).int()
    sc = torch.full((G,), 2.0, device="cuda")
    res = {}
    skinny = ops.gemm_skinny if rows <= 64 else ops.gemm_skinny_wide
    for key, w, K, N, parts, mode, eps in (("qkv", lw.wqkv, D, 3 * D, 3, 0, spec.eps), ("o", lw.wo, D, D, 1, 0, 0.0),
                                           ("gate_up", lw.wgu, D, I, 2, 1, spec.eps), ("down", lw.wd, I, D, 1, 0, 0.0)):
        a = torch.randn((rows, K), device="cuda").bfloat16()
        astack = torch.randn((parts * GR, K), device="cuda").bfloat16()
        bst = torch.randn((w.shape[0], GR), device="cuda").bfloat16()
        t, out = torch.empty((rows, parts * GR), device="cuda").bfloat16(), torch.empty((rows, N), device="cuda").bfloat16()
        gs = {"shrink": capture(lambda: ops.lora_shrink_rows(a, astack, t, ra, sc, G, R, parts)),
              "plain": capture(lambda: skinny(a, w, out, mode=mode, norm_eps=eps)),
              "ext": capture(lambda: ops.gemm_skinny_ext(a, w, out, t, bst, parts, mode=mode, norm_eps=eps))}
        res[key] = {k: round(min(timed(g, reps) for _ in range(3)), 2) for k, g in gs.items()}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--pos", type=int, default=256)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    model = mm.MIDIModel(mm.MIDIModelConfig.from_name("tv2o-medium")).to("cuda", torch.bfloat16).eval()
    result = {"bench": "lora_decode", "rows": a.rows, "pos": a.pos, "slots": G, "rank": R, "stacks": {}}
    with torch.inference_mode():
        for name in ("net", "net_token"):
            arms, st, W = stack_arms(model, name, a.rows, 3 if name == "net_token" else a.pos)
            samples = {"plain": [], "none": [], "robin": []}
            for phase in ("none", "robin"):
                if phase == "robin":
                    for g in range(G):
                        st.load_slot(g, adapter(model._specs[name], len(W.layers), 20 + g), 2.0)
                    st.refresh(W)
                    st.row_adapter.copy_((torch.arange(a.rows) % G).int())
                for _ in range(a.trials):   # the arms alternate
                    if phase == "none":
                        samples["plain"].append(timed(arms["plain"], a.reps))
                    samples[phase].append(timed(arms["lora"], a.reps))
            result["stacks"][name] = {"layers": len(W.layers), **{k: {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1)}
                                                                  for k, v in samples.items()}}
        result["kernels_us"] = kernels_alone(model, a.rows, a.reps)
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
