"""The algebra of the per-vocabulary first token-level block (engine.tok_first_forward / tok_first_backward) on the CPU: the
schedule runs through tests/emu_ops.py with torch stand-ins for the functions of midi_model_amd/tokfirst.py defined here, the
capability question forced on, and is compared with the dense folded schedule on the same bf16 weights."""
import pytest
import torch

import midi_model_amd as mm
from midi_model_amd import engine, tokfirst
from midi_model_amd.train import TrainMIDIModel

import emu_ops


def tiny_config():
    return mm.MIDIModelConfig.get_config("v2", True, 4, 4, 256, 512)


# ---- stand-ins: the C-ABI contracts of include/midihip.h in torch ----------------------------------------------------------------
def _rows(ids, tab0, N):
    return torch.cat([torch.arange(N)[:, None], tab0 + ids[:, :7]], dim=1).reshape(-1)


def tokattn_fwd_rows(zc, ids, tab0, V, o, N, H, scale, cos_t, sin_t):
    return emu_ops.tokattn_fwd(zc[_rows(ids, tab0, N)].contiguous(), o, N, 8, H, scale, cos_t, sin_t)


def tokattn_bwd_rows(zc, ids, tab0, V, dout, dz, dz_hid, rowscale, N, H, scale, cos_t, sin_t):
    rows = _rows(ids, tab0, N)
    full = torch.empty_like(dz)
    emu_ops.tokattn_bwd(zc[rows].contiguous(), dout, full, N, 8, H, scale, cos_t, sin_t,
                        rowscale=None if rowscale is None else rowscale[rows].contiguous())
    dz.copy_(full)
    if dz_hid is not None:
        dz_hid.copy_(full[0::8])
        dz[0::8] = float("nan")                              # (the kernel leaves these rows unwritten)
    return dz


def segment_sum(src_rows, seg_start, rows, out_f32):
    V = out_f32.shape[0]
    ids = torch.repeat_interleave(torch.arange(V), seg_start[1:] - seg_start[:-1])
    out_f32.index_add_(0, ids, rows[src_rows[: int(seg_start[-1])]].float())   # (occurrences behind seg_start[V] are skipped)
    return out_f32


def split_hi_lo(s, hi, lo):
    hi.copy_(s.to(hi.dtype))
    lo.copy_((s - hi.float()).to(lo.dtype))


def table_norm_bwd(t_hi, t_lo, table, rstd, acc32, pad_id):
    Tt, e = t_hi.float() + t_lo.float(), table.float()
    d = Tt - e * (rstd.float() ** 2 * (Tt * e).sum(-1) / e.shape[1])[:, None]
    d[pad_id] = 0
    acc32 += d
    return acc32


STANDINS = dict(tokattn_fwd_rows=tokattn_fwd_rows, tokattn_bwd_rows=tokattn_bwd_rows, segment_sum=segment_sum,
                split_hi_lo=split_hi_lo, table_norm_bwd=table_norm_bwd)


def test_per_vocabulary_first_block_is_the_same_loss_and_gradient(orc, monkeypatch):
    """Two micro-batches inside an accumulation window, ids with a pad in mid-sequence: the loss equals the dense schedule's
    exactly (the forward differs in nothing but where the q|k|v rows lie), every gradient tensor meets the bar of
    test_training_fold_of_the_norms_is_the_same_gradient for a re-associated gradient (cos > 0.995, norm within 5 %)."""
    tok = mm.MIDITokenizerV2()
    shp = orc.Shape(n_layer=4, n_head=4, n_embd=256, n_inner=512, vocab=tok.vocab_size)
    sd = orc.make_state_dict(shp, seed=1)
    g = torch.Generator().manual_seed(7)
    sd = {k: (v * (1.0 + 0.3 * torch.randn(v.shape, generator=g)) if "norm" in k else v) for k, v in sd.items()}
    batch = orc.synthetic_events(tok, 2, 17, seed=2)
    batch[1, 14:] = tok.pad_id
    batch[0, 3, 2] = tok.pad_id                              # pads in mid-sequence, tokens behind them
    batch[1, 6, 1] = tok.pad_id
    assert batch[0, 3, 3] != tok.pad_id and batch[1, 6, 2] != tok.pad_id
    for name, fn in STANDINS.items():
        monkeypatch.setattr(tokfirst, name, fn)
    real_ok = tokfirst.table_first_ok
    monkeypatch.setattr(tokfirst, "table_first_ok",
                        lambda spec, first, slen: first is not None and spec.kind == "token" and slen == 8)
    assert not real_ok(engine.StackSpec("net_token", 256, 1, 128, 1, 1e-6, 1e4, "token"),
                       tokfirst.TokFirst(torch.zeros(4, 256, dtype=torch.bfloat16), None, torch.zeros(8, 256), 0), 8), \
        "host tensors must keep the dense schedule"
    with emu_ops.install():
        outs = []
        for table in (False, True):
            m = TrainMIDIModel(tiny_config(), accumulate_grad_batches=2)
            m.load_state_dict(sd)
            m = m.to(torch.bfloat16)
            m.tok_table_first = table
            calls = []
            real = engine.tok_first_backward
            monkeypatch.setattr(engine, "tok_first_backward", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
            l1 = m.training_step(batch)
            l2 = m.training_step(batch.flip(0))
            monkeypatch.setattr(engine, "tok_first_backward", real)
            assert len(calls) == (2 if table else 0), "the first block did not take the form it was asked for"
            outs.append((l1.clone(), l2.clone(), {k: p.grad.float().clone() for k, p in m.named_parameters()}))
    (a1, a2, ga), (b1, b2, gb) = outs
    assert torch.equal(a1, b1) and torch.equal(a2, b2), (a1, b1, a2, b2)
    pad_row = gb["net_token.embed_tokens.weight"][tok.pad_id]
    assert float(pad_row.abs().max()) == 0
    for k in ga:
        na, nb = ga[k].norm().item(), gb[k].norm().item()
        assert torch.isfinite(gb[k]).all(), k
        if na < 1e-12:
            assert nb < 1e-6, k
            continue
        cos = (ga[k] * gb[k]).sum().item() / (na * nb)
        print(f"{k}: cos {cos:.6f} norm ratio {nb / na:.5f}")
        assert cos > 0.995 and abs(nb / na - 1.0) < 0.05, (k, cos, nb / na)
