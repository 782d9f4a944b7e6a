"""What ``precision="bf16-mixed"`` costs next to bf16-true, measured on the GPU (bench.py never enters the mixed mode).

  python tools/bench_precision.py [--batch 16 --seq 2048 --config tv2o-medium --rounds 5 --steps 4]

Prints ONE JSON line:
  * ``fit_step``: for accumulate_grad_batches 1 and 2, ms per optimiser step (and per micro-batch) of TrainMIDIModel.fit_step in
    both modes at the headline shape, the ratio mixed / bf16-true, and the peak device memory of each mode.  The two modes
    alternate round by round in one process on the same batch; a round is timed with device events around `steps` optimiser
    steps that end in a synchronise; the figure is the median over the rounds, the spread (min, max) is given next to it.
  * ``adamw``: mh_adamw (bf16: 14 bytes per parameter) and mh_adamw_master (fp32 master + bf16 copy: 30 bytes per parameter) in
    isolation on the model's full parameter count, alternating, as achieved GB/s = bytes the algorithm needs / kernel time.

Every measuring process is a child of this driver started under its own time limit; after a child that fails or overruns
nothing more is started.  There is no CPU fallback: without a GPU the tool fails.
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

LIMITS = {"fit_step": 420, "adamw": 180}   # seconds per child


def _events(fn, torch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def child_fit_step(a) -> dict:
    import torch
    import midi_model_amd as mm
    from midi_model_amd.data import synthetic_events
    from midi_model_amd.train import TrainMIDIModel
    if not torch.cuda.is_available():
        raise RuntimeError("bench_precision measures on the GPU: no device visible")
    cfg = mm.MIDIModelConfig.from_name(a.config)
    nacc = a.acc
    models, static, peak = {}, {}, {}
    batch = None
    for mode, precision in (("bf16-true", None), ("bf16-mixed", "bf16-mixed")):
        torch.manual_seed(0)
        before = torch.cuda.memory_allocated()
        m = TrainMIDIModel(cfg, lr=2e-4, warmup=0, accumulate_grad_batches=nacc, precision=precision).to("cuda", torch.bfloat16)
        m.configure_optimizers()
        if batch is None:
            batch = synthetic_events(m.tokenizer, a.batch, a.seq + 1, seed=5, device="cuda")
            before = torch.cuda.memory_allocated() - sum(t.numel() * t.element_size() for t in (m._flat, m._opt["m"], m._opt["v"]))
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        for _ in range(2 * nacc):               # warm-up: every shape of the timed window, the gradient buffers allocated
            m.fit_step(batch)
        torch.cuda.synchronize()
        # this mode's own peak: what the other model (already resident) holds is taken off
        peak[mode] = (torch.cuda.max_memory_allocated() - sum(static.values())) / 2 ** 30
        static[mode] = torch.cuda.memory_allocated() - before   # what this model keeps between steps
        models[mode] = m
    times = {k: [] for k in models}
    for _ in range(a.rounds):
        for mode, m in models.items():          # alternating: both modes see the same box state
            ms = _events(lambda: [m.fit_step(batch) for _ in range(a.steps * nacc)], torch)
            times[mode].append(ms / a.steps)
    out = {"accumulate_grad_batches": nacc}
    for mode, ts in times.items():
        med = statistics.median(ts)
        out[mode] = {"ms_per_optimizer_step": round(med, 3), "ms_per_micro_batch": round(med / nacc, 3),
                     "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3), "peak_memory_gib": round(peak[mode], 3),
                     "resident_gib": round(static[mode] / 2 ** 30, 3)}
    out["ratio_mixed_over_true"] = round(out["bf16-mixed"]["ms_per_optimizer_step"] / out["bf16-true"]["ms_per_optimizer_step"], 4)
    out["peak_memory_delta_gib"] = round(peak["bf16-mixed"] - peak["bf16-true"], 3)
    out["n_params"] = models["bf16-true"]._flat.numel()
    return out


def child_adamw(a) -> dict:
    import torch
    import midi_model_amd as mm
    from midi_model_amd import mixed, ops
    if not torch.cuda.is_available():
        raise RuntimeError("bench_precision measures on the GPU: no device visible")
    n = mm.MIDIModel(mm.MIDIModelConfig.from_name(a.config))._flat.numel()
    g = torch.Generator(device="cuda").manual_seed(0)
    lo = {k: (0.02 * torch.randn(n, device="cuda", generator=g)).to(torch.bfloat16) for k in ("p", "g")}
    lo["m"], lo["v"] = torch.zeros_like(lo["p"]), torch.zeros_like(lo["p"])
    hi = {"p": lo["p"].float(), "g": lo["g"].float()}
    hi["m"], hi["v"], hi["lo"] = torch.zeros_like(hi["p"]), torch.zeros_like(hi["p"]), torch.empty_like(lo["p"])
    coef = torch.ones(1, device="cuda")
    args = (2e-4, 0.9, 0.99, 1e-8, 0.01, 1 - 0.9 ** 3, 1 - 0.99 ** 3, coef)
    run = {"mh_adamw": lambda: ops.adamw(lo["p"], lo["g"], lo["m"], lo["v"], *args),
           "mh_adamw_master": lambda: mixed.adamw_master(hi["p"], hi["lo"], hi["g"], hi["m"], hi["v"], *args)}
    nbytes = {"mh_adamw": 14 * n, "mh_adamw_master": 30 * n}
    for f in run.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in run}
    for _ in range(a.rounds * 4):
        for k, f in run.items():                # alternating
            times[k].append(_events(lambda: [f() for _ in range(5)], torch) / 5)
    out = {"n_params": n}
    for k, ts in times.items():
        med = statistics.median(ts)
        out[k] = {"ms": round(med, 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4),
                  "bytes_per_param": nbytes[k] // n, "gb_per_s": round(nbytes[k] / med / 1e6, 1)}
    out["bandwidth_ratio_master_over_bf16"] = round(out["mh_adamw_master"]["gb_per_s"] / out["mh_adamw"]["gb_per_s"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="tv2o-medium")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seq", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--acc", type=int, default=1)
    ap.add_argument("--child", choices=["fit_step", "adamw"])
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps({"fit_step": child_fit_step, "adamw": child_adamw}[a.child](a)), flush=True)
        return
    common = ["--config", a.config, "--batch", str(a.batch), "--seq", str(a.seq), "--rounds", str(a.rounds), "--steps", str(a.steps)]
    result = {"tool": "bench_precision", "config": a.config, "batch": a.batch, "seq": a.seq, "fit_step": []}
    for name, extra in (("adamw", []), ("fit_step", ["--acc", "1"]), ("fit_step", ["--acc", "2"])):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, *common, *extra], capture_output=True,
                               text=True, timeout=LIMITS[name])
        except subprocess.TimeoutExpired:
            raise SystemExit(f"bench_precision: {name} {extra} overran its {LIMITS[name]} s limit; nothing more is started")
        lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or len(lines) != 1:
            raise SystemExit(f"bench_precision: {name} {extra} failed ({r.returncode}); nothing more is started\n{r.stderr[-3000:]}")
        d = json.loads(lines[0][len("RESULT "):])
        if name == "adamw":
            result["adamw"] = d
        else:
            result["fit_step"].append(d)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
