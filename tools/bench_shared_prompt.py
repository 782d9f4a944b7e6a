#!/usr/bin/env python
"""Same-process A/B of generate(share_prompt=True) against the plain path: B continuations of ONE prompt of P events, 256 new
events, bf16 tv2o-medium, the default sampler.  For every (B, P) the two paths ALTERNATE inside one process with warm clocks
(one untimed call of each first: it captures the session), ``--reps`` times each (default 3: the spread is printed).

  prefill ms       DecodeSession.prefill alone, host clock around a device synchronise
  us / event       generate_stream, events 2..256 (host clock, first event to last: the prefill and the first sample excluded),
                   divided by 255 -- one event = B rows
  peak bytes       torch.cuda.max_memory_allocated over a call that builds its session from an empty pool, minus what was
                   allocated before it (weights): session buffers + prefill activations

usage: tools/bench_shared_prompt.py [--reps 3] [--events 256] [--shapes 4x256,4x1024,...] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import midi_model_amd as mm  # noqa: E402

SHAPES = "4x256,4x1024,4x4096,16x4096,64x1024,64x4096"


def synthetic_prompt(tok, P, seed=0):
    """P plausible events (ids inside the grammar's ranges are not needed for timing: any ids below the vocabulary size do)"""
    g = torch.Generator().manual_seed(seed)
    p = torch.randint(4, tok.vocab_size, (P, tok.max_token_seq), generator=g)
    p[0, 0] = tok.bos_id
    return p.numpy()


def prefill_ms(model, inp, B, max_len, shared):
    P = inp.shape[1]
    with torch.inference_mode():
        if shared:
            ses = model._checkout_session(B, max_len - P + 1, 1.0, 0.98, 20, shared_need=P)
        else:
            ses = model._checkout_session(B, max_len + 1, 1.0, 0.98, 20)
        ses.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ses.prefill(inp)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        ses.reset()
    model._return_session(ses)
    return (t1 - t0) * 1e3


def decode_us(model, prompt, B, max_len, shared, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    it = model.generate_stream(prompt, batch_size=B, max_len=max_len, generator=gen, share_prompt=shared)
    # (generate_stream has no ban_eos: a row may end early, and the loop stops when all have; count what was produced)
    next(it)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = sum(1 for _ in it)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / max(n, 1), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--events", type=int, default=256)
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_shared_prompt: needs a GPU (no timing is taken without one)")
    torch.manual_seed(0)
    model = mm.MIDIModel(mm.MIDIModelConfig.from_name("tv2o-medium")).to("cuda", torch.bfloat16).eval()
    tok = model.tokenizer
    lines = [f"# generate(share_prompt) A/B, bf16 tv2o-medium, {a.events} new events, reps {a.reps}, {torch.cuda.get_device_name(0)}",
             "# B P path | prefill ms (each rep) | us/event (each rep) [events timed] | peak bytes over the weights"]
    for shape in a.shapes.split(","):
        B, P = (int(x) for x in shape.split("x"))
        prompt = synthetic_prompt(tok, P, seed=P)
        max_len = P + a.events
        inp = model._prompt_tensor(prompt, B)
        res = {}
        for shared in (False, True):  # untimed first call from an empty pool: captures the session; its peak is the memory figure
            model._sessions.idle.clear()
            torch.cuda.empty_cache()
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            decode_us(model, prompt, B, max_len, shared, 1)
            res[shared] = {"peak": torch.cuda.max_memory_allocated() - base, "pre": [], "dec": [], "n": 0}
            if shared:  # (both sessions stay pooled for the timed calls)
                pass
        # the plain session was dropped by the clear above: warm it again so that both are pooled
        decode_us(model, prompt, B, max_len, False, 1)
        for r in range(a.reps):
            for shared in (False, True):
                res[shared]["pre"].append(prefill_ms(model, inp, B, max_len, shared))
                us, n = decode_us(model, prompt, B, max_len, shared, 2 + r)
                res[shared]["dec"].append(us)
                res[shared]["n"] = n
        for shared in (False, True):
            x = res[shared]
            lines.append(f"{B:3d} {P:5d} {'shared' if shared else 'plain '} | prefill ms " + " ".join(f"{v:9.2f}" for v in x["pre"])
                         + " | us/event " + " ".join(f"{v:8.1f}" for v in x["dec"]) + f" [{x['n']}] | peak {x['peak']:>14,d}")
        mp, ms = (statistics.median(res[s]["dec"]) for s in (False, True))
        pp, ps = (statistics.median(res[s]["pre"]) for s in (False, True))
        lines.append(f"{B:3d} {P:5d} median: us/event plain {mp:.1f} shared {ms:.1f} (x{mp / ms:.2f}); prefill ms plain {pp:.2f} shared "
                     f"{ps:.2f} (x{pp / ps:.2f}); peak bytes x{res[False]['peak'] / max(res[True]['peak'], 1):.2f}")
        print("\n".join(lines[-3:]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
