"""Shared by test_ragged_host.py and test_ragged_gpu.py: the inputs of the generate_ragged oracle test and the teacher-forced check
(the check of test_shared_prompt_gpu.py, restated per row: the rows of a ragged batch start generating at different events)."""
import os

import torch

LENGTHS = (1, 5, 127, 130)   # prompt lengths of the oracle test; max_len 140: row 3 retires after 10 events, row 0 runs 139
MAX_LEN = 140


def prompts(orc, tok, lengths=LENGTHS, seed0=41):
    """prompt b: the first L_b events of a synthetic piece of max(L_b, 2) events, seed seed0 + b"""
    return [orc.synthetic_events(tok, 1, max(L, 2), seed=seed0 + b)[0, :L].numpy() for b, L in enumerate(lengths)]


def oracle_argmax_check(orc, tok, sd, shp, row, first, margin_min=1e-3):
    """teacher-forced oracle (one uncached pass) over ONE row ``row`` (L, 8): at every sampling position of events >= ``first`` the
    device's id must be the oracle's grammar-masked arg-max (EOS banned) wherever the oracle's top-2 margin exceeds margin_min;
    -> (checked, total)"""
    ids = torch.from_numpy(row)[None]
    _, L, T = ids.shape
    torch.set_num_threads(min(os.cpu_count() or 8, 32))
    with torch.inference_mode():
        hidden = orc.midi_forward(sd, shp, ids[:, :-1])[:, first - 1:]            # hidden i predicts event i + 1
        n = hidden.shape[1]
        tgt = ids[:, first:].reshape(n, T)
        logits = orc.midi_forward_token(sd, shp, hidden.reshape(n, -1), tgt[:, :-1])
    names = [tok.id_events[int(t)] for t in tgt[:, 0]]
    bad, checked = [], 0
    for i in range(T):
        mask = orc.grammar_mask(tok, i, names if i else [""] * n, [False] * n, ban_eos=True).bool()
        assert mask.gather(1, tgt[:, i:i + 1]).all(), f"position {i}: an id outside the grammar mask"
        legal = logits[:, i].masked_fill(~mask, float("-inf"))
        top2 = legal.topk(2, -1)
        safe = (top2.values[:, 0] - top2.values[:, 1]) > margin_min
        checked += int(safe.sum())
        wrong = (tgt[:, i] != top2.indices[:, 0]) & safe
        bad += [(first + int(k), i) for k in wrong.nonzero().flatten()]
    assert not bad, f"device ids differ from the oracle's arg-max at (event, position): {bad[:8]}"
    return checked, n * T


def n_steps(tok, ids):
    """the reference's break rule (midi_model.py:232-235) from the event ids the LIVE rows sampled at position 0"""
    alive = [len(tok.events[tok.id_events[t]]) for t in ids if t != tok.eos_id]
    if not alive:
        return 2
    return alive[0] + 1 if all(a == alive[0] for a in alive) else tok.max_token_seq
