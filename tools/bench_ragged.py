#!/usr/bin/env python
"""Same-process A/B of generate_ragged against what a caller has to do without it: B prompts of B DIFFERENT lengths (spread evenly
over [--lmin, --lmax]), bf16 tv2o-medium, the default sampler, EOS banned, every row generated up to --max-len events.

  (a) ragged    ONE generate_ragged call over the B prompts
  (b) serial    the same prompts as generate() calls, one per distinct length (rows of equal length share a call)

Both are whole calls -- prefill, decode, the host's part -- timed with a host clock around a device synchronise; one untimed call of
each first (it captures the sessions and warms the clocks), then (a) and (b) ALTERNATE, ``--reps`` times each (default 3: every rep
is reported, with the spread).  The figure is USEFUL events/s: only events of live rows count, sum over rows of (max_len - L_b), the
same number on both sides.  One JSON line on stdout (and in --out).

``--row-params`` measures something else: what a CHANGED sampling parameter costs the first call that carries it.  Per rep, a
temperature no call has used yet goes (a) as a scalar -- generate_ragged has to build a session for it: a K/V cache and three
captures -- and (b) as a list of B equal entries -- the pooled row_params session takes it as B-element copies -- alternating, whole
calls timed as above, after one untimed call of each; (c) repeats (a)'s call, now on its pooled session: the call's cost without the
build.  Use a short --max-len (the default becomes lmax + 16) so that the calls are not dominated by decoding.

usage: tools/bench_ragged.py [--B 64] [--max-len 1024] [--lmin 16] [--lmax 512] [--reps 3] [--out FILE] [--row-params]

Result: NOT MEASURED at this commit unless profiles/ holds a line of this tool (DESIGN 7.4 quotes it when it does)."""
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


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--max-len", type=int, default=0, help="default 1024; with --row-params lmax + 16")
    ap.add_argument("--lmin", type=int, default=16)
    ap.add_argument("--lmax", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--row-params", action="store_true", help="first-call cost of a changed parameter: new session vs row_params")
    a = ap.parse_args()
    a.max_len = a.max_len or (a.lmax + 16 if a.row_params else 1024)
    if not torch.cuda.is_available():
        raise SystemExit("bench_ragged: needs a GPU (no timing is taken without one)")
    torch.manual_seed(0)
    model = mm.MIDIModel(mm.MIDIModelConfig.from_name("tv2o-medium")).to("cuda", torch.bfloat16).eval()
    tok = model.tokenizer
    lengths = [int(round(x)) for x in np.linspace(a.lmin, a.lmax, a.B)]
    prompts = [synthetic_prompt(tok, L, seed=L + 7 * b) for b, L in enumerate(lengths)]
    useful = sum(a.max_len - L for L in lengths)
    groups = {}
    for b, L in enumerate(lengths):
        groups.setdefault(L, []).append(b)

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")

    if a.row_params:
        def call(temp):
            out = model.generate_ragged(prompts, max_len=a.max_len, temp=temp, ban_eos=True,
                                        generator=torch.Generator(device="cuda").manual_seed(1))
            assert sum(len(r) - L for r, L in zip(out, lengths)) == useful

        call(1.0), call([1.0] * a.B)   # untimed: one session of each form captured and pooled, clocks warm
        t = {"new_scalar_setting": [], "new_row_params_setting": [], "scalar_setting_again": []}
        for r in range(a.reps):
            temp = 1.0 + 0.01 * (r + 1)
            t["new_scalar_setting"].append(timed(lambda: call(temp)))
            t["new_row_params_setting"].append(timed(lambda: call([temp] * a.B)))
            t["scalar_setting_again"].append(timed(lambda: call(temp)))
        res = {"tool": "bench_ragged --row-params", "device": torch.cuda.get_device_name(0), "model": "tv2o-medium", "dtype": "bf16",
               "B": a.B, "max_len": a.max_len, "lengths": [a.lmin, a.lmax], "useful_events": useful, "reps": a.reps}
        for k, v in t.items():
            res[k] = {"seconds": [round(x, 4) for x in v], "median_seconds": round(statistics.median(v), 4)}
        res["saved_seconds_per_changed_setting"] = round(statistics.median(t["new_scalar_setting"])
                                                         - statistics.median(t["new_row_params_setting"]), 4)
        emit(res)
        return

    def ragged():
        out = model.generate_ragged(prompts, max_len=a.max_len, ban_eos=True, generator=torch.Generator(device="cuda").manual_seed(1))
        assert sum(len(r) - L for r, L in zip(out, lengths)) == useful

    def serial():
        n = 0
        for L, rows in groups.items():
            p = np.stack([prompts[b] for b in rows])
            out = model.generate(p, batch_size=len(rows), max_len=a.max_len, ban_eos=True,
                                 generator=torch.Generator(device="cuda").manual_seed(1))
            n += (out.shape[1] - L) * len(rows)
        assert n == useful

    ragged(), serial()   # untimed: sessions captured and pooled (at most one per distinct batch size), clocks warm
    t = {"ragged": [], "serial": []}
    for _ in range(a.reps):
        t["ragged"].append(timed(ragged))
        t["serial"].append(timed(serial))
    res = {"tool": "bench_ragged", "device": torch.cuda.get_device_name(0), "model": "tv2o-medium", "dtype": "bf16", "B": a.B,
           "max_len": a.max_len, "lengths": [a.lmin, a.lmax], "distinct_lengths": len(groups), "useful_events": useful, "reps": a.reps}
    for k, v in t.items():
        res[k] = {"seconds": [round(x, 4) for x in v], "useful_events_per_s": [round(useful / x, 1) for x in v],
                  "median_events_per_s": round(useful / statistics.median(v), 1),
                  "spread": round((max(v) - min(v)) / statistics.median(v), 4)}
    res["ragged_over_serial"] = round(statistics.median(t["serial"]) / statistics.median(t["ragged"]), 3)
    emit(res)


if __name__ == "__main__":
    main()
