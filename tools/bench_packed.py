"""What packed batches (data.PackedBatch, the table form of the event-level attention) cost and save, measured on the GPU
(bench.py never packs).

  python tools/bench_packed.py [--config tv2o-medium --batch 16 --max-len 2048 --pieces 256 --len-min 64 --len-max 4096
                                --rounds 5 --steps 2]

Prints ONE JSON line:
  * ``attention``: 16 equal sequences of 2048 rows, 16 heads, bf16 -- mh_attn_fwd_seqs / mh_attn_bwd_seqs (rotation back and
    rowscale, as the folded training step calls it) against the uniform launches on the same rows, alternating round by round in
    one process, and the separate RoPE pass of the packed forward (mh_rope_pos) per layer.  us: median (min, max) over the rounds.
  * ``step``: a SYNTHETIC corpus of ``--pieces`` pieces whose lengths are log-uniform in [--len-min, --len-max] (nothing is claimed
    about real datasets); the same indices go through WindowSampler.batch() and .packed_batch() from equally seeded samplers,
    alternating; per form the rows the step runs on, ms per training_step and REAL (non-pad) events per second.

Every measuring process is a child of this driver under its own time limit; after a child that fails or overruns nothing more is
started.  There is no CPU fallback: without a GPU the tool fails.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LIMITS = {"attention": 180, "step": 420}   # seconds per child


def _events(fn, torch, reps=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def _stat(ts, scale=1.0, nd=1):
    return {"median": round(statistics.median(ts) * scale, nd), "min": round(min(ts) * scale, nd), "max": round(max(ts) * scale, nd)}


def child_attention(a) -> dict:
    import torch
    from midi_model_amd import ops
    from midi_model_amd.engine import RopeTable
    if not torch.cuda.is_available():
        raise RuntimeError("bench_packed measures on the GPU: no device visible")
    B, S, H = 16, 2048, 16
    M, D = B * S, H * 64
    g = torch.Generator(device="cuda").manual_seed(0)
    qkv = torch.randn((M, 3 * D), device="cuda", generator=g).to(torch.bfloat16)
    do = torch.randn((M, D), device="cuda", generator=g).to(torch.bfloat16)
    rs = 0.5 + torch.rand(M, device="cuda", generator=g)
    tab = RopeTable(64, 10000.0, "cuda", S)
    plan = ops.attn_seq_plan([S] * B, H).upload("cuda")
    o = torch.empty((M, D), dtype=torch.bfloat16, device="cuda")
    lse_u, lse_t = torch.empty(B * H * S, device="cuda"), torch.empty(H * M, device="cuda")
    dq = torch.empty_like(qkv)
    rot = qkv.clone()
    run = {
        "fwd_uniform": lambda: ops.attn_fwd(qkv, o, lse_u, B, S, H, 0.125),
        "fwd_table": lambda: ops.attn_fwd_seqs(qkv, o, lse_t, plan, H, 0.125),
        "bwd_uniform": lambda: ops.attn_bwd(qkv, o, do, lse_u, dq, B, S, H, 0.125, tab.cos, tab.sin, rowscale=rs),
        "bwd_table": lambda: ops.attn_bwd_seqs(qkv, o, do, lse_t, dq, plan, H, 0.125, tab.cos, tab.sin, rowscale=rs),
        "rope_pos": lambda: ops.rope_pos_(rot, tab.cos, tab.sin, plan.pos, H, 64, 1),
        "rope_uniform_pass": lambda: ops.rope_(rot, tab.cos, tab.sin, S, 0, H, 64, 1),
    }
    for f in run.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in run}
    for _ in range(a.rounds * 4):
        for k, f in run.items():                # alternating: every form sees the same box state
            times[k].append(_events(f, torch, 5))
    out = {"shape": {"sequences": B, "rows_each": S, "heads": H}, "us": {k: _stat(ts, 1e3) for k, ts in times.items()}}
    out["rope_pos_bytes"] = M * 2 * D * 2 * 2   # q and k thirds, read and written, bf16
    return out


def child_step(a) -> dict:
    import numpy as np
    import torch
    import midi_model_amd as mm
    from midi_model_amd.data import TokenCorpus, WindowSampler
    from midi_model_amd.train import TrainMIDIModel
    if not torch.cuda.is_available():
        raise RuntimeError("bench_packed measures on the GPU: no device visible")
    cfg = mm.MIDIModelConfig.from_name(a.config)
    torch.manual_seed(0)
    m = TrainMIDIModel(cfg, lr=2e-4, warmup=0, accumulate_grad_batches=1).to("cuda", torch.bfloat16)
    tok = m.tokenizer
    rng = np.random.default_rng(0)
    lens = np.exp(rng.uniform(np.log(a.len_min), np.log(a.len_max), a.pieces)).astype(np.int64)
    corpus = TokenCorpus([rng.integers(1, tok.vocab_size, size=(int(n), 8)).astype(np.int16) for n in lens], device="cuda")
    H = m._specs["net"].H
    order = rng.permutation(a.pieces).tolist()
    groups = [order[i:i + a.batch] for i in range(0, a.batch * a.steps, a.batch)]
    samplers = {"padded": WindowSampler(corpus, a.max_len, seed=1), "packed": WindowSampler(corpus, a.max_len, seed=1)}

    def batches(kind):
        s = samplers[kind]
        return [s.batch(g, tok.pad_id) if kind == "padded" else s.packed_batch(g, tok.pad_id, n_head=H) for g in groups]

    def rows(kind, b):
        return b.shape[0] * (b.shape[1] - 1) if kind == "padded" else b.x.shape[0]

    def real(kind, b):  # events that carry a target: (window length - 1) summed
        return int((b[:, 1:] != tok.pad_id).any(-1).sum()) if kind == "padded" else b.real_rows

    for kind in samplers:                         # warm-up on the first round's shapes
        for b in batches(kind):
            m.training_step(b)
            m.zero_grad()
    torch.cuda.synchronize()
    times, nrows, nreal = {k: [] for k in samplers}, {}, {}
    for _ in range(a.rounds):
        for kind in samplers:                     # alternating; both samplers draw the same windows round after round
            bs = batches(kind)
            nrows[kind], nreal[kind] = sum(rows(kind, b) for b in bs), sum(real(kind, b) for b in bs)
            torch.cuda.synchronize()

            def go():
                for b in bs:
                    m.training_step(b)
                    m.zero_grad()
            times[kind].append(_events(go, torch) / len(bs))
    out = {"pieces": a.pieces, "len_min": a.len_min, "len_max": a.len_max, "max_len": a.max_len, "windows_per_batch": a.batch,
           "batches_per_round": len(groups)}
    for kind, ts in times.items():
        med = statistics.median(ts)
        out[kind] = {"ms_per_step": _stat(ts, 1.0, 3), "rows_per_step": nrows[kind] // len(groups),
                     "real_events_per_step": nreal[kind] // len(groups),
                     "real_events_per_s": round(nreal[kind] / len(groups) / med * 1e3, 1)}
    out["real_events_per_s_ratio_packed_over_padded"] = round(out["packed"]["real_events_per_s"] / out["padded"]["real_events_per_s"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="tv2o-medium")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--max-len", type=int, default=2048)
    ap.add_argument("--pieces", type=int, default=256)
    ap.add_argument("--len-min", type=int, default=64)
    ap.add_argument("--len-max", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--only", choices=["attention", "step"])
    ap.add_argument("--child", choices=["attention", "step"])
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps({"attention": child_attention, "step": child_step}[a.child](a)), flush=True)
        return
    common = [x for k in ("config", "batch", "max_len", "pieces", "len_min", "len_max", "rounds", "steps")
              for x in ("--" + k.replace("_", "-"), str(getattr(a, k)))]
    result = {"tool": "bench_packed", "config": a.config}
    for name in ([a.only] if a.only else ["attention", "step"]):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, *common], capture_output=True, text=True,
                               timeout=LIMITS[name])
        except subprocess.TimeoutExpired:
            raise SystemExit(f"bench_packed: {name} overran its {LIMITS[name]} s limit; nothing more is started")
        lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or len(lines) != 1:
            raise SystemExit(f"bench_packed: {name} failed ({r.returncode}); nothing more is started\n{r.stderr[-3000:]}")
        result[name] = json.loads(lines[0][len("RESULT "):])
    print(json.dumps(result))


if __name__ == "__main__":
    main()
