#!/usr/bin/env python
"""Same-process A/B of a sibling admission in the decode pool: ``submit(prompt, n=N)`` -- ONE prefill and one mh_kv_fork_rows launch
that fills the other N - 1 rows -- against N ``submit``s of the same prompt, which prefill it N times in one packed forward.  bf16
tv2o-medium, a seeded pool of ``--rows`` rows, one fresh pool (on the one pooled session) per trial.

  (a) fork      pool.submit(prompt, n=N, seed=[...]);                     pool.step()
  (b) prefill   [pool.submit(prompt, seed=s) for s in seeds];             pool.step()

Timed: from the start of the admitting ``step()`` -- admission, the first event's token steps, the net step behind them, the host's
part -- to a device synchronise, with a host clock.  Per prompt length (``--lengths``) one untimed run of each form first, then the
two ALTERNATE, ``--trials`` times each (default 20); medians and spreads ((max - min) / median) are reported.

Separately the kernel alone: mh_kv_fork_rows on a cache of 8 rows of ``--capacity`` events, N - 1 pairs out of row 0, at the same
lengths, between device events (``--kernel-reps`` launches after 3 untimed ones, the median); the bytes it needs are
(N - 1) pairs x L events x 48 KiB read + the same written (12 layers x 16 heads x 64 x 2 B x K and V), and its rate is given as a share
of ``--copy-rate`` (default 6.29e12 B/s, the chip's measured copy rate).  The N - 1 pairs read ONE source, so the reads after the first
may be served by a cache; the figure counts them as bytes all the same.

One JSON line on stdout (and in --out).  usage: tools/bench_fork.py [--rows 64] [--n 4] [--lengths 64,512,2048,4000] [--trials 20]
[--out FILE].  Result: profiles/fork_ab.txt when it holds a line of this tool (DESIGN 7.9 quotes it); NOT MEASURED otherwise."""
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


def synthetic_prompt(tok, P, seed=0):
    """P events (ids inside the grammar's ranges are not needed for timing: any ids below the vocabulary size do)"""
    g = torch.Generator().manual_seed(seed)
    p = torch.randint(4, tok.vocab_size, (P, tok.max_token_seq), generator=g)
    p[0, 0] = tok.bos_id
    return p.numpy()


def stats(xs):
    med = statistics.median(xs)
    return {"median_ms": round(1e3 * med, 4), "min_ms": round(1e3 * min(xs), 4), "max_ms": round(1e3 * max(xs), 4),
            "spread": round((max(xs) - min(xs)) / med, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--n", type=int, default=4)
    ap.add_argument("--lengths", default="64,512,2048,4000")
    ap.add_argument("--trials", type=int, default=20)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--copy-rate", type=float, default=6.29e12)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fork: needs a GPU (no timing is taken without one)")
    torch.manual_seed(0)
    model = mm.MIDIModel(mm.MIDIModelConfig.from_name("tv2o-medium")).to("cuda", torch.bfloat16).eval()
    tok = model.tokenizer
    lengths = [int(x) for x in a.lengths.split(",")]
    gen = 8                                  # events a request may generate: one is, inside the timed step
    capacity = max(lengths) + gen + 1
    seeds = list(range(1, a.n + 1))

    def trial(prompt, fork: bool) -> float:
        with model.decode_pool(a.rows, capacity, seeded=True) as pool:
            if fork:
                ids = pool.submit(prompt, max_len=len(prompt) + gen, ban_eos=True, seed=seeds, n=a.n)
            else:
                ids = [pool.submit(prompt, max_len=len(prompt) + gen, ban_eos=True, seed=s) for s in seeds]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = pool.step()
            torch.cuda.synchronize()
            t = time.perf_counter() - t0
            assert [r for r, _, _ in out] == list(ids) and sorted(pool.occupied) == list(range(a.n))
        return t

    res = {"tool": "bench_fork", "device": torch.cuda.get_device_name(0), "model": "tv2o-medium", "dtype": "bf16", "rows": a.rows,
           "n": a.n, "capacity": capacity, "trials": a.trials, "admission": {}, "kernel": {}}
    for L in lengths:
        prompt = synthetic_prompt(tok, L, seed=L)
        trial(prompt, True), trial(prompt, False)   # untimed: the session captured, every shape warm
        t = {"fork": [], "prefill": []}
        for _ in range(a.trials):
            t["fork"].append(trial(prompt, True))
            t["prefill"].append(trial(prompt, False))
        res["admission"][str(L)] = {"fork": stats(t["fork"]), "prefill": stats(t["prefill"]),
                                    "prefill_over_fork": round(statistics.median(t["prefill"]) / statistics.median(t["fork"]), 3),
                                    "saved_ms": round(1e3 * (statistics.median(t["prefill"]) - statistics.median(t["fork"])), 4)}
        print(f"L {L}: {res['admission'][str(L)]}", file=sys.stderr, flush=True)
    model._sessions.idle.clear()             # (the pooled session's cache goes before the kernel's own is made)
    torch.cuda.empty_cache()

    # ---- the kernel alone
    spec = model._specs["net"]
    cap = 256
    while cap < capacity:
        cap *= 2
    k = torch.randn((spec.L, 8, spec.H, cap, spec.hd), device="cuda").to(torch.bfloat16)
    v = torch.randn((spec.L, 8, spec.H, cap, spec.hd), device="cuda").to(torch.bfloat16)
    per_event = spec.L * spec.H * spec.hd * 2 * 2   # bytes of K and V of one event of one row
    res["kernel"]["cache"] = list(k.shape)
    src, dst = [0] * (a.n - 1), list(range(1, a.n))
    for L in lengths:
        lens = [L] * (a.n - 1)
        dev = torch.tensor([src, dst, lens], dtype=torch.int32, device="cuda")
        for _ in range(3):
            ops.kv_fork_rows(k, v, src, dst, lens, dev=dev)
        torch.cuda.synchronize()
        times = []
        for _ in range(a.kernel_reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.kv_fork_rows(k, v, src, dst, lens, dev=dev)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e-3)
        assert torch.equal(k[:, 1, :, :L].view(torch.int16), k[:, 0, :, :L].view(torch.int16))
        moved = 2 * (a.n - 1) * L * per_event
        med = statistics.median(times)
        res["kernel"][str(L)] = {"pairs": a.n - 1, "bytes_read_plus_written": moved, "median_us": round(1e6 * med, 2),
                                 "min_us": round(1e6 * min(times), 2), "max_us": round(1e6 * max(times), 2),
                                 "bytes_per_s": round(moved / med, 1), "share_of_copy_rate": round(moved / med / a.copy_rate, 4)}
        print(f"kernel L {L}: {res['kernel'][str(L)]}", file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
