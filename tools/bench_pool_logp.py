#!/usr/bin/env python
"""Same-process A/B of the decode pool's log-likelihood output (DecodePool(logprobs=True)): the fused sampler's ``_logp``
forms against the plain forms.  bf16 tv2o-medium, ``--rows`` rows.

  (1) sampler  the eight sampler launches of one event (token positions 0..7 of the v2 grammar, rows x 3406 logits in rows of the padded
               vocabulary), mh_sample_top_p_k_rows against mh_sample_top_p_k_rows_logp and mh_sample_top_p_k_seeded against
               mh_sample_top_p_k_seeded_logp: timed with device events around the eight launches, the forms alternating; us per
               event (eight launches) and per launch;
  (2) decode   the median decode step of a seeded pool whose ``--rows`` rows all stand behind ``--prompt`` events (one prompt, n = rows
               siblings), host clock from ``step()`` to a device synchronise, ``--events`` steps, with and without the option
               alternating.

One JSON line on stdout (and in --out).  usage: tools/bench_pool_logp.py [--rows 64] [--prompt 64] [--events 64] [--trials 3]
[--reps 50] [--out FILE].  Result: profiles/pool_logp_ab.txt (DESIGN 7.12 quotes it)."""
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

from bench_fork import stats, synthetic_prompt  # noqa: E402

SAMPLERS = ("rows", "rows_logp", "seeded", "seeded_logp")


def sampler_alone(model, rows, reps):
    """-> {form: [seconds per event (8 launches)]}"""
    tok = model.tokenizer
    V, Vp, T = tok.vocab_size, model.vocab_padded, tok.max_token_seq
    first, lo, hi, arity = model._grammar()
    span, ranges = ops.mask_spans(first, lo, hi)
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(1)
    logits = (torch.randn((T, rows, Vp), generator=g, device=dev) * 3).bfloat16()
    q = torch.empty((T, rows, V), device=dev).exponential_(1.0, generator=g)
    full = max(range(V), key=lambda i: arity[i])   # an event id with the most parameters: no position samples the pad id
    ev = torch.full((rows,), full, dtype=torch.int64, device=dev)
    fm = first[None].repeat(rows, 1).contiguous()
    ban = torch.zeros_like(fm)
    temp = torch.full((rows,), 1.0, device=dev)
    top_p = torch.full((rows,), 0.98, device=dev)
    top_k = torch.full((rows,), 20, dtype=torch.int32, device=dev)
    seed = torch.arange(1, rows + 1, dtype=torch.int64, device=dev)
    ctr = torch.full((rows,), 5, dtype=torch.int32, device=dev)
    seq = torch.zeros((rows, T), dtype=torch.int64, device=dev)
    sink = torch.zeros((rows,), dtype=torch.int64, device=dev)
    logp = torch.zeros((rows, T), dtype=torch.float32, device=dev)

    def run(form):
        for i in range(T):
            kw = dict(out_b=sink, first_span=span, max_range=ranges[i], fill_rest=T - 1 if i == 0 else 0, fill_id=tok.pad_id)
            noise = (seed, ctr) if form.startswith("seeded") else (q[i],)
            extra = (logp[:, i],) if form.endswith("_logp") else ()
            getattr(ops, "sample_top_p_k_" + form)(logits[i], fm, lo, hi, ev, i, *noise, seq[:, i], V, temp, top_p, top_k, ban, *extra,
                                                   **kw)

    out = {f: [] for f in SAMPLERS}
    for f in SAMPLERS:
        run(f)
    torch.cuda.synchronize()
    for _ in range(reps):
        for f in SAMPLERS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(f)
            e1.record()
            torch.cuda.synchronize()
            out[f].append(e0.elapsed_time(e1) * 1e-3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--prompt", type=int, default=64)
    ap.add_argument("--events", type=int, default=64)
    ap.add_argument("--trials", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pool_logp: needs a GPU (no timing is taken without one)")
    torch.manual_seed(0)
    model = mm.MIDIModel(mm.MIDIModelConfig.from_name("tv2o-medium")).to("cuda", torch.bfloat16).eval()
    tok = model.tokenizer
    res = {"tool": "bench_pool_logp", "device": torch.cuda.get_device_name(0), "model": "tv2o-medium", "dtype": "bf16", "rows": a.rows,
           "prompt": a.prompt, "events": a.events, "trials": a.trials, "reps": a.reps, "sampler_event": {}, "decode_step": {}}

    # ---- (1) the eight sampler launches of an event
    with torch.inference_mode():
        t = sampler_alone(model, a.rows, a.reps)
    for f in SAMPLERS:
        med = statistics.median(t[f])
        res["sampler_event"][f] = {"us_per_event": round(1e6 * med, 2), "us_per_launch": round(1e6 * med / 8, 2),
                                   "spread": round((max(t[f]) - min(t[f])) / med, 4)}
    for f in ("rows", "seeded"):
        res["sampler_event"][f + "_logp_minus_plain_us"] = round(
            res["sampler_event"][f + "_logp"]["us_per_event"] - res["sampler_event"][f]["us_per_event"], 2)
    print(f"sampler: {res['sampler_event']}", file=sys.stderr, flush=True)

    # ---- (2) the decode step of a pool, with and without the option
    gen = a.events + 4
    capacity = a.prompt + gen + 1
    prompt = synthetic_prompt(tok, a.prompt, seed=a.prompt)
    forms = {"plain": {}, "logprobs": dict(logprobs=True)}

    def trial(form, events):
        with model.decode_pool(a.rows, capacity, seeded=True, **forms[form]) as pool:
            pool.submit(prompt, max_len=a.prompt + gen, ban_eos=True, seed=list(range(1, a.rows + 1)), n=a.rows)
            times = []
            for _ in range(1 + events):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pool.step()
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
            assert len(pool.occupied) == a.rows and pool.ses.logprobs == bool(forms[form])
        return times[1:]

    for f in forms:
        trial(f, 2)   # untimed: sessions captured, shapes warm
    dec = {f: [] for f in forms}
    for _ in range(a.trials):
        for f in forms:
            dec[f] += trial(f, a.events)
    entry = {f: stats(dec[f]) for f in forms}
    entry["logprobs_over_plain"] = round(entry["logprobs"]["median_ms"] / entry["plain"]["median_ms"], 4)
    entry["logprobs_minus_plain_us"] = round(1e3 * (entry["logprobs"]["median_ms"] - entry["plain"]["median_ms"]), 2)
    res["decode_step"] = entry
    print(f"decode step: {entry}", file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
