"""Generate tests/golden/tiny_mixed.npz: the REAL reference's training recipe (train.py:168-188 step, :121-151 AdamW in two
groups, LambdaLR, gradient_clip_val=1.0, accumulate_grad_batches=2 with Lightning's loss / 2) on the tiny config for six
optimiser steps, three ways on the same weights and batches:

  fp32      the model in float32                                              (the yardstick)
  bf16      ``model.bfloat16()``: the reference's ``--precision bf16-true``
  autocast  float32 parameters, forward under ``torch.autocast("cpu", torch.bfloat16)``: the reference's ``bf16-mixed``

Written: the twelve per-micro-batch losses and the final per-tensor parameter norms of each run, and the seeds the test
rebuilds weights and batches from.  Runs only where the reference exists (like tests/gen_golden.py, whose helpers it uses);
the output is committed.  Usage:  python tests/gen_golden_mixed.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as gg  # noqa: E402

WEIGHT_SEED, BATCH_SEED0 = 1, 300
STEPS, NACC = 6, 2
LR, WARMUP, MAX_STEP, WEIGHT_DECAY = 1e-3, 2, 10, 0.01
BATCH, EVENTS = 2, 17


def run(ref_model, orc, shp, sd, batches, mode):
    model = gg.build_ref(ref_model, shp, sd)
    model.train()
    if mode == "bf16":
        model = model.to(torch.bfloat16)
    params = list(model.named_parameters())
    no_decay = ["bias", "norm"]
    opt = torch.optim.AdamW([{"params": [p for n, p in params if not any(nd in n for nd in no_decay)], "weight_decay": WEIGHT_DECAY},
                             {"params": [p for n, p in params if any(nd in n for nd in no_decay)], "weight_decay": 0.0}],
                            lr=LR, betas=(0.9, 0.99), eps=1e-8)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: orc.lr_lambda(s, WARMUP, MAX_STEP))
    losses = []
    for step in range(STEPS):
        opt.zero_grad(set_to_none=True)
        for mb in range(NACC):
            b = batches[step * NACC + mb]
            if mode == "autocast":
                with torch.autocast("cpu", dtype=torch.bfloat16):
                    loss, _, _ = gg.ref_train_loss(model, b)
            else:
                loss, _, _ = gg.ref_train_loss(model, b)
            (loss / NACC).backward()
            losses.append(float(loss.item()))
        torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
        opt.step()
        sched.step()
    names = [n for n, _ in params]
    norms = np.array([p.detach().float().norm().item() for _, p in params], dtype=np.float64)
    return np.array(losses, dtype=np.float64), names, norms


def main():
    ref_model, ref_tok = gg.import_reference()
    orc = gg.load_oracle()
    tok = ref_tok.MIDITokenizer("v2")
    shp = orc.Shape(n_layer=4, n_head=4, n_embd=256, n_inner=512, vocab=tok.vocab_size)
    sd = orc.make_state_dict(shp, seed=WEIGHT_SEED)
    batches = [orc.synthetic_events(tok, BATCH, EVENTS, seed=BATCH_SEED0 + i) for i in range(STEPS * NACC)]
    out = dict(weight_seed=np.int64(WEIGHT_SEED), batch_seed0=np.int64(BATCH_SEED0), steps=np.int64(STEPS), nacc=np.int64(NACC),
               lr=np.float64(LR), warmup=np.int64(WARMUP), max_step=np.int64(MAX_STEP), weight_decay=np.float64(WEIGHT_DECAY),
               batch=np.int64(BATCH), events=np.int64(EVENTS))
    for mode in ("fp32", "bf16", "autocast"):
        torch.manual_seed(0)
        losses, names, norms = run(ref_model, orc, shp, sd, batches, mode)
        out[f"losses_{mode}"], out[f"param_norms_{mode}"] = losses, norms
        print(mode, losses)
    out["param_names"] = np.array(names)
    path = os.path.join(gg.OUT, "tiny_mixed.npz")
    np.savez_compressed(path, **out)
    print("written", path, os.path.getsize(path))


if __name__ == "__main__":
    main()
