#!/usr/bin/env python
"""Same-process A/B of lookahead decoding in the decode pool (DecodePool(lookahead=k)).  bf16 tv2o-medium with random
weights for the timing arms, R requests behind ``--prompt`` events each, ``--events`` events to generate; for every (k, R):

  (a) plain     a seeded pool of R rows without the option: the median step and events/s (R events a step);
  (b) no draft  a lookahead pool whose proposer returns nothing: the median step -- the pure overhead of the option per step (k + 1
                times the rows, the attention pair instead of the fused launch, the scatter) -- and events/s;
  (c) oracle    the same pool with a proposer that returns the continuation recorded in (b): the ceiling -- events/s over the whole
                run, events per step per request, the median step;
  (a') full     a seeded pool of R (k + 1) rows, all of them requests: the median step.  With n of its rows occupied it yields n
                events a step, so it beats (c) above n* = (c)'s events/s x (a')'s step; reported as n* and n* / (R (k + 1)).
  (d) trained   the built-in n-gram proposer on the TRAINED tiny model of the parity tests (tests/golden/tiny_trained.npz), R = 1, at
                the reference's sampling defaults (temp 1, top-p 0.98, top-k 20), ``--seeds`` requests from a BOS prompt: guesses
                consumed, guesses that proved right, events per step, and the seconds of the same requests with no drafts.  A toy
                model trained on a structured toy corpus: NOT a real checkpoint, and it predicts nothing about one.

Arms alternate inside one process; every step is timed on the host clock from ``step()`` to a device synchronise.  One JSON line on
stdout (and in --out).  usage: tools/bench_pool_lookahead.py [--ks 3,7] [--rs 1,8] [--prompt 64] [--events 128] [--trials 3] [--seeds 8]
[--out FILE].  Result: profiles/pool_lookahead_ab.txt (DESIGN 7.14 quotes it)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import midi_model_amd as mm  # noqa: E402

from bench_fork import stats, synthetic_prompt  # noqa: E402


def no_drafts(history, k):
    return np.zeros((0, 8), dtype=np.int64)


def oracle_of(recorded):
    def propose(history, k):
        n = len(history)
        for rec in recorded:
            if len(rec) > n and (rec[:n] == history).all():
                return rec[n:n + k]
        return np.zeros((0, 8), dtype=np.int64)
    return propose


def run(model, rows, capacity, prompts, gen, seeds, lookahead=None, proposer=None, **kw):
    """one pool, len(prompts) requests admitted in the first step -> (step times behind the admitting step, wall seconds of those
    steps, events they yielded, results, the pool's draft counters)"""
    opt = dict(lookahead=lookahead) if lookahead else {}
    with model.decode_pool(rows, capacity, seeded=True, **opt) as pool:
        if proposer is not None:
            pool.proposer = proposer
        ids = [pool.submit(p, max_len=len(p) + gen, seed=s, **kw) for p, s in zip(prompts, seeds)]
        times, events = [], 0
        first = True
        while pool.pending():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = pool.step()
            torch.cuda.synchronize()
            if not first:
                times.append(time.perf_counter() - t0)
                events += len(out)
            first = False
        return times, sum(times), events, [pool.result(i) for i in ids], (pool.drafted, pool.accepted)


def load_trained():
    """tests/golden/tiny_trained.npz -> the trained tiny model (tests/conftest.py: load_trained), bf16 on the device"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "tiny_trained.npz"), allow_pickle=False)
    sd = {}
    for k in g.files:
        if k.startswith("q8:"):
            sd[k[3:]] = torch.from_numpy(g[k].astype(np.float32)) * 2.0 ** int(g["e:" + k[3:]])
        elif k.startswith("b16:"):
            sd[k[4:]] = torch.from_numpy(g[k].copy()).view(torch.bfloat16).float()
    m = mm.MIDIModel(mm.MIDIModelConfig.get_config("v2", True, 4, 4, 256, 1024))
    m.load_state_dict(sd, strict=True)
    return m.to("cuda", torch.bfloat16).eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="3,7")
    ap.add_argument("--rs", default="1,8")
    ap.add_argument("--prompt", type=int, default=64)
    ap.add_argument("--events", type=int, default=128)
    ap.add_argument("--trials", type=int, default=3)
    ap.add_argument("--seeds", type=int, default=8)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pool_lookahead: needs a GPU (no timing is taken without one)")
    ks, rs = [int(x) for x in a.ks.split(",")], [int(x) for x in a.rs.split(",")]
    torch.manual_seed(0)
    model = mm.MIDIModel(mm.MIDIModelConfig.from_name("tv2o-medium")).to("cuda", torch.bfloat16).eval()
    tok = model.tokenizer
    capacity = a.prompt + a.events + 1
    res = {"tool": "bench_pool_lookahead", "device": torch.cuda.get_device_name(0), "model": "tv2o-medium", "dtype": "bf16",
           "prompt": a.prompt, "events": a.events, "trials": a.trials, "arms": [], "trained": {}}
    kw = dict(ban_eos=True)
    for k in ks:
        for R in rs:
            prompts = [synthetic_prompt(tok, a.prompt, seed=100 + i) for i in range(R)]
            full = [synthetic_prompt(tok, a.prompt, seed=100 + i) for i in range(R * (k + 1))]
            seeds, fseeds = list(range(1, R + 1)), list(range(1, R * (k + 1) + 1))
            with torch.inference_mode():
                # untimed: sessions captured, shapes warm, and the continuation the oracle returns
                run(model, R, capacity, prompts, 4, seeds, **kw)
                run(model, R * (k + 1), capacity, full, 4, fseeds, **kw)
                rec = run(model, R, capacity, prompts, a.events, seeds, lookahead=k, proposer=no_drafts, **kw)[3]
                t = {x: [] for x in ("plain", "no_draft", "oracle", "full")}
                wall = {x: [0.0, 0] for x in t}
                for _ in range(a.trials):
                    for arm, call in (("plain", lambda: run(model, R, capacity, prompts, a.events, seeds, **kw)),
                                      ("no_draft", lambda: run(model, R, capacity, prompts, a.events, seeds, lookahead=k,
                                                               proposer=no_drafts, **kw)),
                                      ("oracle", lambda: run(model, R, capacity, prompts, a.events, seeds, lookahead=k,
                                                             proposer=oracle_of(rec), **kw)),
                                      ("full", lambda: run(model, R * (k + 1), capacity, full, a.events, fseeds, **kw))):
                        times, secs, events, out, _ = call()
                        if arm in ("no_draft", "oracle"):
                            assert all((x == y).all() for x, y in zip(out, rec)), "the drafts changed a result"
                        t[arm] += times
                        wall[arm][0] += secs
                        wall[arm][1] += events
            entry = {"k": k, "R": R, "session_rows": R * (k + 1)}
            for arm in t:
                entry[arm] = dict(stats(t[arm]), steps=len(t[arm]), events_per_s=round(wall[arm][1] / wall[arm][0], 1),
                                  events_per_step_per_request=round(wall[arm][1] / len(t[arm]) / (R * (k + 1) if arm == "full" else R), 3))
            entry["no_draft_over_plain_step"] = round(entry["no_draft"]["median_ms"] / entry["plain"]["median_ms"], 4)
            entry["oracle_over_plain_events_per_s"] = round(entry["oracle"]["events_per_s"] / entry["plain"]["events_per_s"], 3)
            n_star = entry["oracle"]["events_per_s"] * entry["full"]["median_ms"] * 1e-3
            entry["full_pool_beats_oracle_above_rows"] = round(n_star, 2)
            entry["... as a share of the session's rows"] = round(n_star / (R * (k + 1)), 3)
            res["arms"].append(entry)
            print(f"k {k} R {R}: {entry}", file=sys.stderr, flush=True)

    # ---- (d) the built-in proposer on the trained toy model
    tiny = load_trained()
    bos = np.full((1, tok.max_token_seq), tok.pad_id, dtype=np.int64)
    bos[0, 0] = tok.bos_id
    gen = 256
    for k in ks:
        drafted = accepted = steps = events = eos = 0
        secs = {"no_draft": 0.0, "lookahead": 0.0}
        with torch.inference_mode():
            run(tiny, 1, gen + 2, [bos], 4, [1], lookahead=k)
            for s in range(a.seeds):
                times, sec, ev, out, (d, acc) = run(tiny, 1, gen + 2, [bos], gen, [1000 + s], lookahead=k)
                _, sec0, ev0, out0, _ = run(tiny, 1, gen + 2, [bos], gen, [1000 + s], lookahead=k, proposer=no_drafts)
                assert (out[0] == out0[0]).all(), "the drafts changed a result"
                drafted, accepted, steps, events = drafted + d, accepted + acc, steps + len(times), events + ev
                eos += int(out[0][-1, 0] == tok.eos_id)
                secs["lookahead"] += sec
                secs["no_draft"] += sec0
        res["trained"][f"k={k}"] = {
            "requests": a.seeds, "ended_on_eos": eos, "events": events, "steps": steps, "events_per_step": round(events / max(steps, 1), 3),
            "guesses_consumed": drafted, "guesses_right": accepted, "acceptance": round(accepted / max(drafted, 1), 3),
            "seconds_built_in": round(secs["lookahead"], 4), "seconds_no_draft": round(secs["no_draft"], 4)}
        print(f"trained toy model, k {k}: {res['trained'][f'k={k}']}", file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
