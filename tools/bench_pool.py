#!/usr/bin/env python
"""Same-process A/B of the decode pool (MIDIModel.decode_pool) against generate_ragged over consecutive groups: --requests requests
(default 256) arriving together in a fixed order, prompt lengths spread evenly over [--lmin, --lmax] and events to generate spread
evenly over [--gmin, --gmax], each dealt to the requests by a seeded permutation of its own (so a group of 64 consecutive requests
holds short and long ones, as a serving caller's do); bf16 tv2o-medium, the default sampler, EOS banned, ``--rows`` decode rows.

  (a) pool      ONE DecodePool of --rows rows: all requests submitted, stepped until none is pending
  (b) static    generate_stream_ragged over consecutive groups of --rows requests in the same order, max_len per row

Both are whole runs -- prefills, decode, the host's part -- timed with a host clock around a device synchronise; one untimed run of
each first (it captures the sessions and warms the clocks), then (a) and (b) ALTERNATE, ``--reps`` times each (default 3: every rep
is reported, with the spread).  The figures: USEFUL events/s -- requested events only, sum of the requests' events to generate, the
same number on both sides -- and the time from the start of the run to the first event of the LAST request.  The static form's
waste, sum over groups of sum_b (gen_max - gen_b) parked row-events, is printed beside the measured ratio as the ratio it
predicts: (useful + waste) / useful row-events -- the bound for a pool that is never short of queued requests; a finite list also
drains (its last requests run beside free rows), so each arm reports the event steps it ran, its prefill groups and the time per
step.  One JSON line on stdout (and in --out).

``--seeded``: the A/B is instead the SEEDED pool (decode_pool(seeded=True), request i on seed i: no noise graph, the sampler computes
its variates) against the unseeded pool of (a) on the same request list, alternating in the same way; the same figures per arm,
and ``seeded_over_pool`` (> 1: the seeded pool is faster).

usage: tools/bench_pool.py [--requests 256] [--rows 64] [--lmin 16] [--lmax 512] [--gmin 32] [--gmax 512] [--reps 3] [--seeded]
                           [--out FILE]

Result: profiles/pool_ab.txt when it holds a line of this tool (DESIGN 7.7 quotes it), profiles/seeded_ab.txt for --seeded (DESIGN
7.8); NOT MEASURED otherwise."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import midi_model_amd as mm  # noqa: E402


def synthetic_prompt(tok, P, seed=0):
    """P plausible events (ids inside the grammar's ranges are not needed for timing: any ids below the vocabulary size do)"""
    g = torch.Generator().manual_seed(seed)
    p = torch.randint(4, tok.vocab_size, (P, tok.max_token_seq), generator=g)
    p[0, 0] = tok.bos_id
    return p.numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=256)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--lmin", type=int, default=16)
    ap.add_argument("--lmax", type=int, default=512)
    ap.add_argument("--gmin", type=int, default=32)
    ap.add_argument("--gmax", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--seeded", action="store_true", help="A/B the seeded pool against the unseeded pool")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pool: needs a GPU (no timing is taken without one)")
    torch.manual_seed(0)
    model = mm.MIDIModel(mm.MIDIModelConfig.from_name("tv2o-medium")).to("cuda", torch.bfloat16).eval()
    tok = model.tokenizer
    rng = np.random.RandomState(a.seed)
    n = a.requests
    lengths = [int(round(x)) for x in np.linspace(a.lmin, a.lmax, n)[rng.permutation(n)]]
    gens = [int(round(x)) for x in np.linspace(a.gmin, a.gmax, n)[rng.permutation(n)]]
    max_lens = [L + g for L, g in zip(lengths, gens)]
    prompts = [synthetic_prompt(tok, L, seed=L + 7 * b) for b, L in enumerate(lengths)]
    useful = sum(gens)
    groups = [list(range(i, min(i + a.rows, n))) for i in range(0, n, a.rows)]
    waste = sum(max(gens[b] for b in grp) * len(grp) - sum(gens[b] for b in grp) for grp in groups)
    capacity = max(max_lens) + 1

    def pool_run(seeded=False):
        """-> (seconds, seconds to the first event of the last request, event steps, admission groups)"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        first_last = None
        got = steps = admissions = 0
        gen = None if seeded else torch.Generator(device="cuda").manual_seed(1)
        with model.decode_pool(a.rows, capacity, generator=gen, seeded=seeded) as pool:
            ids = [pool.submit(p, max_len=m, ban_eos=True, seed=i if seeded else None)
                   for i, (p, m) in enumerate(zip(prompts, max_lens))]
            while pool.pending():
                queued = len(pool.queue)
                out = pool.step()
                steps += 1
                admissions += len(pool.queue) < queued
                got += len(out)
                if first_last is None and out and out[-1][0] == ids[-1]:
                    first_last = time.perf_counter() - t0
            torch.cuda.synchronize()
            t = time.perf_counter() - t0
            assert got == useful and all(len(pool.result(i)) == m for i, m in zip(ids, max_lens))
        return t, first_last, steps, admissions

    def static_run():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        first_last = None
        got = steps = 0
        for gi, grp in enumerate(groups):
            for ev, live in model.generate_stream_ragged([prompts[b] for b in grp], max_len=[max_lens[b] for b in grp], ban_eos=True,
                                                         generator=torch.Generator(device="cuda").manual_seed(1)):
                if gi == len(groups) - 1 and first_last is None:
                    first_last = time.perf_counter() - t0
                got += int(live.sum())
                steps += 1
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        assert got == useful, (got, useful)
        return t, first_last, steps, len(groups)

    other = "seeded" if a.seeded else "static"
    other_run = (lambda: pool_run(True)) if a.seeded else static_run
    pool_run(), other_run()   # untimed: sessions captured and pooled, clocks warm
    t = {"pool": [], other: []}
    for _ in range(a.reps):
        t["pool"].append(pool_run())
        t[other].append(other_run())
    res = {"tool": "bench_pool", "device": torch.cuda.get_device_name(0), "model": "tv2o-medium", "dtype": "bf16", "requests": n,
           "rows": a.rows, "prompt_lengths": [a.lmin, a.lmax], "events_to_generate": [a.gmin, a.gmax], "seed": a.seed,
           "capacity": capacity, "useful_events": useful, "static_parked_row_events": waste, "reps": a.reps}
    for k, v in t.items():
        secs = [x[0] for x in v]
        res[k] = {"seconds": [round(x, 4) for x in secs], "useful_events_per_s": [round(useful / x, 1) for x in secs],
                  "median_events_per_s": round(useful / statistics.median(secs), 1),
                  "spread": round((max(secs) - min(secs)) / statistics.median(secs), 4),
                  "first_event_of_last_request_s": [round(x[1], 4) for x in v], "event_steps": v[0][2],
                  "prefill_groups": v[0][3], "ms_per_event_step": round(1e3 * statistics.median(secs) / v[0][2], 3)}
    if a.seeded:
        res["seeded_over_pool"] = round(statistics.median([x[0] for x in t["pool"]]) / statistics.median([x[0] for x in t["seeded"]]), 3)
    else:
        res["pool_over_static"] = round(statistics.median([x[0] for x in t["static"]]) / statistics.median([x[0] for x in t["pool"]]), 3)
        res["ratio_predicted_from_parked_row_events"] = round((useful + waste) / useful, 3)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
