#!/usr/bin/env python
"""Same-process A/B of sibling groups in the decode pool with and without a shared prompt: ``submit(prompt, n=k)`` -- every sibling
owns a copy of the prompt's K/V and streams it at every decoded event -- against ``submit(prompt, n=k, share_prefix=True)`` in a pool
with prefix slots, where the prompt's K/V sits once in a slot and is read once per event for the k rows.  bf16
tv2o-medium, seeded pools of ``--rows`` rows, one fresh pool (on its pooled session) per trial; only the group's k rows are occupied.

  (a) copies    decode_pool(rows, cap)                                    submit(prompt, n=k)
  (b) share     decode_pool(rows, cap, prefix_slots=G, prefix_capacity=P)  submit(prompt, n=k, share_prefix=True)
  (c) bystander decode_pool(rows, cap, prefix_slots=G, prefix_capacity=P)  submit(prompt, n=k)      -- rows that share nothing in a
      pool WITH slots, against (a): what the extra launch per layer costs everyone else

Timed with a host clock, each from the start of ``step()`` to a device synchronise: the ADMITTING step (admission, the first event's
token steps, the net step behind them; (b) skips the siblings' K/V copy) and each of the ``--events`` (default 64) decode steps after
it.  Per (k, prompt length) one untimed trial of each form first, then the three ALTERNATE, ``--trials`` times each; medians and spreads
((max - min) / median) are reported, and per k the crossover: the measured prompt lengths between which sharing starts to win.

Beside each measurement the bytes the attention must move per event and layer: k x P x 4096 for the siblings' copies (K and V of an
event: 16 heads x 64 x 2 B x 2) against P x 4096 + k x 16 x ceil(P / 256) x 264 x 2 for one read plus the partials written and read.

One JSON line on stdout (and in --out).  usage: tools/bench_pool_share.py [--rows 64] [--ks 4,8] [--lengths 64,512,2048,4000]
[--events 64] [--trials 3] [--out FILE].  Result: profiles/pool_share_ab.txt when it holds a line of this tool (DESIGN 7.10 quotes
it); NOT MEASURED otherwise."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import midi_model_amd as mm  # noqa: E402

from bench_fork import stats, synthetic_prompt  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--ks", default="4,8")
    ap.add_argument("--lengths", default="64,512,2048,4000")
    ap.add_argument("--events", type=int, default=64)
    ap.add_argument("--trials", type=int, default=3)
    ap.add_argument("--slots", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pool_share: needs a GPU (no timing is taken without one)")
    torch.manual_seed(0)
    model = mm.MIDIModel(mm.MIDIModelConfig.from_name("tv2o-medium")).to("cuda", torch.bfloat16).eval()
    tok, spec = model.tokenizer, model._specs["net"]
    lengths, ks = [int(x) for x in a.lengths.split(",")], [int(x) for x in a.ks.split(",")]
    gen = a.events + 4                        # events a request may generate: the timed ones and a margin
    capacity = max(lengths) + gen + 1
    slots = dict(prefix_slots=a.slots, prefix_capacity=max(lengths))
    forms = {"copies": ({}, False), "share": (slots, True), "bystander": (slots, False)}
    per_event = spec.H * spec.hd * 2 * 2      # bytes of K and V of one event of one row of one layer

    def trial(prompt, k: int, form: str):
        kw, share = forms[form]
        with model.decode_pool(a.rows, capacity, seeded=True, **kw) as pool:
            ids = pool.submit(prompt, max_len=len(prompt) + gen, ban_eos=True, seed=list(range(1, k + 1)), n=k, share_prefix=share)
            times = []
            for _ in range(1 + a.events):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = pool.step()
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
            assert [r for r, _, _ in out] == list(ids) and sorted(pool.occupied) == list(range(k))
            assert (pool.ses.slot_refs[0] == k) if share else not any(getattr(pool.ses, "slot_refs", None) or [])
        return times[0], times[1:]

    res = {"tool": "bench_pool_share", "device": torch.cuda.get_device_name(0), "model": "tv2o-medium", "dtype": "bf16",
           "rows": a.rows, "capacity": capacity, "events": a.events, "trials": a.trials, **slots, "shapes": {}, "crossover": {}}
    for k in ks:
        wins = []
        for P in lengths:
            prompt = synthetic_prompt(tok, P, seed=P)
            for form in forms:                # untimed: both sessions captured, every shape warm
                trial(prompt, k, form)
            adm, dec = {f: [] for f in forms}, {f: [] for f in forms}
            for _ in range(a.trials):
                for form in forms:
                    t_adm, t_dec = trial(prompt, k, form)
                    adm[form].append(t_adm)
                    dec[form] += t_dec
            med = {f: statistics.median(dec[f]) for f in forms}
            nch = (P + 255) // 256
            entry = {"decode_step": {f: stats(dec[f]) for f in forms}, "admitting_step": {f: stats(adm[f]) for f in forms},
                     "copies_over_share": round(med["copies"] / med["share"], 4),
                     "bystander_over_copies": round(med["bystander"] / med["copies"], 4),
                     "bystander_extra_us": round(1e6 * (med["bystander"] - med["copies"]), 2),
                     "attention_bytes_per_event_and_layer": {"copies": k * P * per_event,
                                                             "share": P * per_event + k * spec.H * nch * 264 * 2}}
            res["shapes"][f"k{k}_P{P}"] = entry
            wins.append((P, med["share"] < med["copies"]))
            print(f"k {k} P {P}: {entry}", file=sys.stderr, flush=True)
        lose = [P for P, w in wins if not w]
        win = [P for P, w in wins if w]
        res["crossover"][f"k{k}"] = {"sharing_loses_at": lose, "sharing_wins_at": win}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
