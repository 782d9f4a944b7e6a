#!/usr/bin/env python
"""Same-process A/B of the decode pool's event-level K/V cache in bf16 and in fp8 (DecodePool(kv_dtype="fp8")): e4m3 codes
with an fp32 scale per (row, head, event) for K and for V, 136 bytes where bf16 holds 256.  bf16 tv2o-medium, ``--rows`` rows.

  (1) attention  the two launches alone, ops.attn_decode_append_rows and ops.attn_decode_append_rows_fp8, at rows x P cached events:
                 timed with device events around one pass over the 12 layers' caches (12 launches, each over a cache of its own, as in
                 a decode step), the two forms alternating; us per launch and TB/s over ALGORITHMIC bytes (rows x 16 heads x P x 256
                 or 136).  At short P the 12 caches fit the last-level cache: the rate is then not an HBM rate.
  (2) decode     the median decode step of a pool whose ``--rows`` rows all stand behind P events (one prompt, n = rows siblings:
                 every row owns a copy), host clock from ``step()`` to a device synchronise, ``--events`` steps, the caches alternating;
  (3) admit      the admitting step of ONE request of P events (prefill, the K/V store -- which quantizes -- the first event);
  (4) bytes      the event-level cache of the session, both forms.

One JSON line on stdout (and in --out).  usage: tools/bench_pool_kvq.py [--rows 64] [--lengths 64,512,2048,4000] [--events 32]
[--trials 3] [--reps 20] [--out FILE].  Result: profiles/pool_kvq_ab.txt (DESIGN 7.11 quotes it)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import midi_model_amd as mm  # noqa: E402
from midi_model_amd import ops  # noqa: E402
from midi_model_amd.engine import RopeTable  # noqa: E402

from bench_fork import stats, synthetic_prompt  # noqa: E402

FORMS = {"bf16": {}, "fp8": dict(kv_dtype="fp8")}


def attention_alone(rows, H, P, cap, layers, reps):
    """-> {form: [seconds per launch]} -- `reps` alternating passes over `layers` caches; codes and scales random but finite"""
    dev, D = "cuda", H * 64
    g = torch.Generator(device=dev).manual_seed(P)
    qkv = torch.randn((rows, 3 * D), generator=g, device=dev).bfloat16()
    o = torch.empty((rows, D), dtype=torch.bfloat16, device=dev)
    pos = torch.full((rows,), P, dtype=torch.int32, device=dev)
    rope = RopeTable(64, 10000.0, torch.device(dev), cap)
    kb = torch.randn((layers, rows, H, cap, 64), generator=g, device=dev).bfloat16()
    vb = torch.randn((layers, rows, H, cap, 64), generator=g, device=dev).bfloat16()
    k8 = torch.randint(0, 120, (layers, rows, H, cap, 64), generator=g, device=dev, dtype=torch.uint8)
    v8 = torch.randint(0, 120, (layers, rows, H, cap, 64), generator=g, device=dev, dtype=torch.uint8)
    sc = torch.rand((layers, rows, H, cap, 2), generator=g, device=dev) * 0.01 + 0.001

    def run(form):
        for li in range(layers):
            if form == "bf16":
                ops.attn_decode_append_rows(qkv, rope.cos, rope.sin, kb[li], vb[li], o, rows, H, 64, cap, 0.125, pos)
            else:
                ops.attn_decode_append_rows_fp8(qkv, rope.cos, rope.sin, k8[li], v8[li], sc[li], o, rows, H, 64, cap, 0.125, pos)

    out = {f: [] for f in FORMS}
    for f in FORMS:
        run(f)
    for _ in range(reps):
        for f in FORMS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(f)
            e1.record()
            torch.cuda.synchronize()
            out[f].append(e0.elapsed_time(e1) * 1e-3 / layers)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--lengths", default="64,512,2048,4000")
    ap.add_argument("--admit-lengths", default="64,2048,4000")
    ap.add_argument("--events", type=int, default=32)
    ap.add_argument("--trials", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pool_kvq: needs a GPU (no timing is taken without one)")
    torch.manual_seed(0)
    model = mm.MIDIModel(mm.MIDIModelConfig.from_name("tv2o-medium")).to("cuda", torch.bfloat16).eval()
    tok, spec = model.tokenizer, model._specs["net"]
    lengths = [int(x) for x in a.lengths.split(",")]
    admit_lengths = [int(x) for x in a.admit_lengths.split(",")]
    gen = a.events + 4
    capacity = max(lengths + admit_lengths) + gen + 1
    res = {"tool": "bench_pool_kvq", "device": torch.cuda.get_device_name(0), "model": "tv2o-medium", "dtype": "bf16", "rows": a.rows,
           "capacity": capacity, "events": a.events, "trials": a.trials, "reps": a.reps, "attention": {}, "decode_step": {},
           "admitting_step": {}, "cache_bytes": {}}

    # ---- (1) the attention launches alone
    cap = 256
    while cap < capacity:
        cap *= 2
    for P in lengths:
        t = attention_alone(a.rows, spec.H, P, cap, spec.L, a.reps)
        entry = {}
        for f, per in (("bf16", 256), ("fp8", 136)):
            med = statistics.median(t[f])
            nbytes = a.rows * spec.H * P * per
            entry[f] = {"us": round(1e6 * med, 2), "spread": round((max(t[f]) - min(t[f])) / med, 4), "bytes": nbytes,
                        "TBps": round(nbytes / med / 1e12, 3)}
        entry["bf16_over_fp8"] = round(entry["bf16"]["us"] / entry["fp8"]["us"], 4)
        res["attention"][f"P{P}"] = entry
        print(f"attention P {P}: {entry}", file=sys.stderr, flush=True)
        torch.cuda.empty_cache()

    # ---- (2), (3): pools
    def trial(prompt, n: int, form: str, events: int):
        with model.decode_pool(a.rows, capacity, seeded=True, **FORMS[form]) as pool:
            pool.submit(prompt, max_len=len(prompt) + gen, ban_eos=True, seed=list(range(1, n + 1)) if n > 1 else 1, n=n)
            times = []
            for _ in range(1 + events):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pool.step()
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
            assert len(pool.occupied) == n and pool.ses.kv_dtype == FORMS[form].get("kv_dtype")
            if form not in res["cache_bytes"]:
                kv = pool.ses.kv1
                res["cache_bytes"][form] = kv.nbytes() if form == "fp8" else (kv.k.numel() + kv.v.numel()) * kv.k.element_size()
        return times[0], times[1:]

    for P in lengths:
        prompt = synthetic_prompt(tok, P, seed=P)
        for f in FORMS:
            trial(prompt, a.rows, f, 2)   # untimed: sessions captured, shapes warm
        dec = {f: [] for f in FORMS}
        for _ in range(a.trials):
            for f in FORMS:
                dec[f] += trial(prompt, a.rows, f, a.events)[1]
        entry = {f: stats(dec[f]) for f in FORMS}
        entry["bf16_over_fp8"] = round(entry["bf16"]["median_ms"] / entry["fp8"]["median_ms"], 4)
        res["decode_step"][f"P{P}"] = entry
        print(f"decode step P {P}: {entry}", file=sys.stderr, flush=True)
    for P in admit_lengths:
        prompt = synthetic_prompt(tok, P, seed=P)
        for f in FORMS:
            trial(prompt, 1, f, 0)
        adm = {f: [] for f in FORMS}
        for _ in range(max(a.trials, 5)):
            for f in FORMS:
                adm[f].append(trial(prompt, 1, f, 0)[0])
        entry = {f: stats(adm[f]) for f in FORMS}
        entry["fp8_minus_bf16_ms"] = round(entry["fp8"]["median_ms"] - entry["bf16"]["median_ms"], 4)
        res["admitting_step"][f"P{P}"] = entry
        print(f"admitting step P {P}: {entry}", file=sys.stderr, flush=True)
    faster = [P for P in lengths if res["decode_step"][f"P{P}"]["bf16_over_fp8"] > 1.0]
    res["crossover"] = {"fp8_faster_at": faster, "fp8_slower_at": [P for P in lengths if P not in faster]}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
