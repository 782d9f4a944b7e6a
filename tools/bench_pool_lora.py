#!/usr/bin/env python
"""Same-process A/B of the decode pool's LoRA adapter slots (DecodePool(lora_slots=G, lora_rank=R)).  bf16 tv2o-medium,
``--rows`` rows, G = 4 adapters of rank 64 on every target of both stacks.

  (a) plain   the median decode step of a plain pool whose rows all stand behind ``--prompt`` events;
  (b) none    the same in a pool with adapter slots and no row adapted: the price of the option;
  (c) robin   the same with the four adapters round-robin over the rows;
              (host clock from ``step()`` to a device synchronise, ``--events`` steps, the three arms alternating, ``--trials`` times)
  (d) mixed   the time to finish ONE request set -- ``--requests`` requests, a fifth on each adapter and a fifth on none, prompts of
              ``--prompt`` events, ``--events`` events to generate -- in the LoRA pool, against the same set served adapter by adapter
              on merged weights: for each adapter the weights are merged (W + s B A in place, timed), its requests run in a plain pool,
              and the base weights are put back.

One JSON line on stdout (and in --out).  usage: tools/bench_pool_lora.py [--rows 64] [--prompt 64] [--events 64] [--trials 3]
[--requests 160] [--out FILE].  Result: profiles/pool_lora_ab.txt (DESIGN 7.13 quotes it)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import midi_model_amd as mm  # noqa: E402

from bench_fork import stats, synthetic_prompt  # noqa: E402

G, R, ALPHA = 4, 64, 128.0
MODS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")


def save_adapter(model, d, seed):
    """a rank-64 adapter on every target, in peft's layout; -> {parameter name: delta of the merged weight (bf16, on the device)}"""
    from safetensors.torch import save_file
    g = torch.Generator().manual_seed(seed)
    tensors, delta = {}, {}
    for name, p in model.named_parameters():
        if ".layers." in name and name.endswith(".weight") and any(name[:-7].endswith(t) for t in MODS):
            o, i = p.shape
            A = (torch.randn((R, i), generator=g) * i ** -0.5).bfloat16()
            B = (torch.randn((o, R), generator=g) * 0.02).bfloat16()
            tensors[f"base_model.model.{name[:-7]}.lora_A.weight"], tensors[f"base_model.model.{name[:-7]}.lora_B.weight"] = A, B
    os.makedirs(d)
    save_file(tensors, os.path.join(d, "adapter_model.safetensors"))
    with open(os.path.join(d, "adapter_config.json"), "w") as f:
        json.dump({"peft_type": "LORA", "r": R, "lora_alpha": ALPHA, "use_rslora": False}, f)
    return d


def step_times(pool, prompt, rows, events, adapters):
    """fill the pool, then -> seconds of each of ``events`` decode steps"""
    for k in range(rows):
        kw = dict(adapter=adapters[k % len(adapters)]) if adapters else {}
        pool.submit(prompt, max_len=len(prompt) + events + 2, ban_eos=True, **kw)
    pool.step()          # the admission
    torch.cuda.synchronize()
    out = []
    for _ in range(events):
        t0 = time.perf_counter()
        pool.step()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def finish(pool, reqs):
    for p, kw in reqs:
        pool.submit(p, **kw)
    while pool.pending():
        pool.step()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--prompt", type=int, default=64)
    ap.add_argument("--events", type=int, default=64)
    ap.add_argument("--trials", type=int, default=3)
    ap.add_argument("--requests", type=int, default=160)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    model = mm.MIDIModel(mm.MIDIModelConfig.from_name("tv2o-medium")).to("cuda", torch.bfloat16).eval()
    tok = model.tokenizer
    prompt = synthetic_prompt(tok, a.prompt)
    cap = a.prompt + a.events + 8
    res = {"bench": "pool_lora", "rows": a.rows, "prompt": a.prompt, "events": a.events, "slots": G, "rank": R}
    with tempfile.TemporaryDirectory() as root:
        dirs = [save_adapter(model, os.path.join(root, f"a{g}"), 40 + g) for g in range(G)]
        # ---- (a) (b) (c)
        samples = {"plain": [], "none": [], "robin": []}
        for _ in range(a.trials):
            with model.decode_pool(a.rows, cap) as pool:
                samples["plain"] += step_times(pool, prompt, a.rows, a.events, None)
            with model.decode_pool(a.rows, cap, lora_slots=G, lora_rank=R) as pool:
                samples["none"] += step_times(pool, prompt, a.rows, a.events, None)
            with model.decode_pool(a.rows, cap, lora_slots=G, lora_rank=R) as pool:
                ids = [pool.load_adapter(d) for d in dirs]
                samples["robin"] += step_times(pool, prompt, a.rows, a.events, ids)
        res["decode_step"] = {k: stats(v) for k, v in samples.items()}
        # ---- (d)
        groups = [None] + list(range(G))
        kw = dict(max_len=a.prompt + a.events, ban_eos=True)
        mixed, split, merge_s = [], [], []
        from safetensors.torch import load_file
        params = dict(model.named_parameters())
        for _ in range(a.trials):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with model.decode_pool(a.rows, cap, lora_slots=G, lora_rank=R) as pool:
                ids = [pool.load_adapter(d) for d in dirs]
                finish(pool, [(prompt, dict(kw, adapter=None if groups[k % 5] is None else ids[groups[k % 5]])) for k in range(a.requests)])
            mixed.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            spent = 0.0
            for grp in groups:
                n = sum(1 for k in range(a.requests) if groups[k % 5] == grp)
                if grp is not None:   # merge, as load_merge_lora does: W += s B A
                    t1 = time.perf_counter()
                    sd = {k: v.cuda() for k, v in load_file(os.path.join(dirs[grp], "adapter_model.safetensors")).items()}
                    keep = {}
                    with torch.no_grad():
                        for key, A in sd.items():
                            if key.endswith("lora_A.weight"):
                                name = key[len("base_model.model."):-len(".lora_A.weight")] + ".weight"
                                keep[name] = params[name].data.clone()
                                params[name].data.add_(((ALPHA / R) * (sd[key.replace("lora_A", "lora_B")].float() @ A.float())).bfloat16())
                    torch.cuda.synchronize()
                    spent += time.perf_counter() - t1
                with model.decode_pool(a.rows, cap) as pool:
                    finish(pool, [(prompt, kw)] * n)
                if grp is not None:
                    t1 = time.perf_counter()
                    with torch.no_grad():
                        for name, w in keep.items():
                            params[name].data.copy_(w)
                    torch.cuda.synchronize()
                    spent += time.perf_counter() - t1
            split.append(time.perf_counter() - t0)
            merge_s.append(spent)
        res["mixed_set"] = {"requests": a.requests, "lora_pool": stats(mixed), "adapter_by_adapter_merged": stats(split),
                            "of_which_merging_and_restoring": stats(merge_s),
                            "ratio_split_over_lora": round(statistics.median(split) / statistics.median(mixed), 3)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
