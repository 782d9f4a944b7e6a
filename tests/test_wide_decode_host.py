"""Decode batches of 65 to 256 rows on the CPU: which entry point engine.stack_decode and decode.DecodeSession pick for every row
count class (1..64: mh_gemm_skinny; 65..256: mh_gemm_skinny_wide; more, fp32, or MH_DECODE_WIDE=0: the general form), in every form of
the attention step, through the ragged fake backend plus the stand-ins of tests/emu_wide.py, by its call log.  The kernel itself:
test_gemm_skinny_wide_gpu.py; the production session: test_wide_decode_gpu.py."""
import numpy as np
import pytest
import torch

import midi_model_amd as mm
from midi_model_amd import engine

import emu_ragged
import emu_shared
import emu_wide

FOLDED_NARROW = ["gemm_skinny", "attn_decode_append", "gemm_skinny", "gemm_skinny", "gemm_skinny"]   # what test_host_logic.py pins
FOLDED_WIDE = ["gemm_skinny_wide", "attn_decode_append", "gemm_skinny_wide", "gemm_skinny_wide", "gemm_skinny_wide"]
SKINNY_WIDE = ["rmsnorm_fwd", "gemm_skinny_wide", "attn_decode_append", "gemm_skinny_wide", "rmsnorm_fwd", "gemm_skinny_wide",
               "gemm_skinny_wide"]
GENERAL = ["rmsnorm_fwd", "gemm_nt", "kv_append", "attn_decode", "gemm_nt", "rmsnorm_fwd", "gemm_nt", "swiglu_fwd", "gemm_nt"]


def tiny_config():
    # (inner widths 1024 / 256: every contraction of both stacks is a multiple of 256, so a session folds -- with 512 / 128, the
    #  tiny shape of the other host tests, the token-level stack keeps the general form at every batch)
    return mm.MIDIModelConfig.get_config("v2", True, 4, 4, 256, 1024)


@pytest.fixture(scope="module")
def tok():
    return mm.MIDITokenizerV2()


@pytest.fixture(scope="module")
def tiny(orc, tok):
    shp = orc.Shape(n_layer=4, n_head=4, n_embd=256, n_inner=1024, vocab=tok.vocab_size)
    return shp, orc.make_state_dict(shp, seed=0)


def _model(sd, dtype=torch.bfloat16):
    m = mm.MIDIModel(tiny_config())
    m.load_state_dict(sd)
    return m.to(dtype)


def _setup(m, pre, B, cap=16, seed=3):
    spec, W = m._specs[pre], m._W[pre]
    x = torch.randn((B, spec.D), generator=torch.Generator().manual_seed(seed)).to(m.dtype)
    rope = engine.RopeTable(spec.hd, spec.theta, x.device, cap)
    kv = engine.KVState(spec, B, cap, x)
    kv.k.zero_(), kv.v.zero_()
    return spec, W, x, rope, kv


def _run(log, fn):
    del log[:]
    out = fn()
    return out, list(log)


def _swap(per_layer, old, new):
    return [new if n == old else n for n in per_layer]


def test_stack_decode_takes_the_wide_entry_point_from_65_to_256_rows(tiny, monkeypatch):
    monkeypatch.delenv("MH_DECODE_WIDE", raising=False)
    with emu_wide.install() as log, torch.no_grad():
        m = _model(tiny[1])
        for B in (80, 65, 256):
            spec, W, x, rope, kv = _setup(m, "net", B)
            L = len(W.layers)
            fold = engine.fold_norm_weights(W)
            y, names = _run(log, lambda: engine.stack_decode(spec, W, x, rope, kv, folded=fold, final_norm=False))
            assert names == FOLDED_WIDE * L and kv.len == 1, (B, names[:8])
            assert "gemm_nt" not in names and "rmsnorm_fwd" not in names and "gemm_skinny" not in names
            assert y.shape == (B, spec.D) and torch.isfinite(y.float()).all()
            _, names = _run(log, lambda: engine.stack_decode(spec, W, x, rope, kv, final_norm=False))   # the unfolded skinny form
            assert names == SKINNY_WIDE * L and kv.len == 2, (B, names[:8])
            _, names = _run(log, lambda: engine.stack_decode(spec, W, x, rope, kv, folded=fold))         # (final norm: one more call)
            assert names == FOLDED_WIDE * L + ["rmsnorm_fwd"]


def test_x_ids_first_layer_row_pos_and_shared_forms_at_80_rows(tiny, monkeypatch):
    from midi_model_amd import shared as sp
    monkeypatch.delenv("MH_DECODE_WIDE", raising=False)
    B = 80
    with emu_wide.install() as log, torch.no_grad():
        m = _model(tiny[1])
        # the token-level stack with its first layer reading rows of the embedding table by id (repeated ids, the last table row)
        spec, W, _, rope, kv = _setup(m, "net_token", B, cap=8)
        L = len(W.layers)
        fold = engine.fold_norm_weights(W)
        ids = (torch.arange(B) * 37 + 5) % W.embed.shape[0]
        ids[0] = ids[B // 2] = W.embed.shape[0] - 1
        y, names = _run(log, lambda: engine.stack_decode(spec, W, W.embed, rope, kv, folded=fold, final_norm=False, x_ids=ids))
        assert names == FOLDED_WIDE * L and y.shape == (B, spec.D)
        kv2 = engine.KVState(spec, B, 8, y)
        kv2.k.zero_(), kv2.v.zero_()
        y2 = engine.stack_decode(spec, W, W.embed[ids].contiguous(), rope, kv2, folded=fold, final_norm=False)
        assert torch.equal(y, y2) and torch.equal(kv.k, kv2.k)   # the lookup inside the projections is the lookup before them
        # per-row positions (generate_ragged)
        spec, W, x, rope, kv = _setup(m, "net", B)
        fold = engine.fold_norm_weights(W)
        pos = (torch.arange(B, dtype=torch.int32) % 7)
        _, names = _run(log, lambda: engine.stack_decode(spec, W, x, rope, kv, folded=fold, final_norm=False, row_pos=pos))
        assert names == _swap(FOLDED_WIDE, "attn_decode_append", "attn_decode_append_rows") * len(W.layers) and kv.len == 0
        # one shared prompt (share_prompt): the two launches of shared.py stand where the attention step stood
        for n in emu_shared._NAMES:
            monkeypatch.setattr(sp, n, emu_ragged._logged(n, getattr(emu_shared, n), log))
        P = 3
        kvp = engine.KVState(spec, 1, 16, x)
        xp = torch.randn((P, spec.D), generator=torch.Generator().manual_seed(5)).to(x.dtype)
        engine.stack_prefill(spec, W, xp, 1, P, rope, kvp)
        kvs = engine.KVState(spec, B, 16, x)
        ws = torch.zeros((sp.workspace_floats(B, spec.H, kvp.cap),))
        y, names = _run(log, lambda: engine.stack_decode(spec, W, x, rope, kvs, folded=fold, final_norm=False,
                                                        shared=sp.SharedPrefix(kvp, None, ws)))
        want = ["gemm_skinny_wide", "attn_prefix_partial", "attn_decode_append_shared"] + ["gemm_skinny_wide"] * 3
        assert names == want * len(W.layers) and kvs.len == 1 and torch.isfinite(y.float()).all(), names[:8]


def test_64_rows_and_fewer_never_name_the_wide_call(tiny, monkeypatch):
    monkeypatch.delenv("MH_DECODE_WIDE", raising=False)
    with emu_wide.install() as log, torch.no_grad():
        m = _model(tiny[1])
        for B in (2, 64):
            spec, W, x, rope, kv = _setup(m, "net", B)
            fold = engine.fold_norm_weights(W)
            _, names = _run(log, lambda: engine.stack_decode(spec, W, x, rope, kv, folded=fold, final_norm=False))
            assert names == FOLDED_NARROW * len(W.layers)
            _, names = _run(log, lambda: engine.stack_decode(spec, W, x, rope, kv, final_norm=False))
            assert names == _swap(SKINNY_WIDE, "gemm_skinny_wide", "gemm_skinny") * len(W.layers)


def test_general_form_past_256_rows_in_fp32_and_with_the_switch_off(tiny, monkeypatch):
    with emu_wide.install() as log, torch.no_grad():
        m = _model(tiny[1])
        monkeypatch.delenv("MH_DECODE_WIDE", raising=False)
        spec, W, x, rope, kv = _setup(m, "net", 257)
        _, names = _run(log, lambda: engine.stack_decode(spec, W, x, rope, kv, final_norm=False))
        assert names == GENERAL * len(W.layers)
        spec, W, x, rope, kv = _setup(m, "net", 80)
        _, names = _run(log, lambda: engine.stack_decode(spec, W, x, rope, kv, final_norm=False, wide=False))
        assert names == GENERAL * len(W.layers)
        monkeypatch.setenv("MH_DECODE_WIDE", "0")
        _, names = _run(log, lambda: engine.stack_decode(spec, W, x, rope, kv, final_norm=False))
        assert names == GENERAL * len(W.layers)
        _, names = _run(log, lambda: engine.stack_decode(spec, W, x, rope, kv, final_norm=False, wide=True))   # the caller's word holds
        assert names == SKINNY_WIDE * len(W.layers)
        monkeypatch.delenv("MH_DECODE_WIDE")
        m32 = _model(tiny[1], torch.float32)
        spec, W, x, rope, kv = _setup(m32, "net", 80)
        _, names = _run(log, lambda: engine.stack_decode(spec, W, x, rope, kv, final_norm=False))
        assert names == GENERAL * len(W.layers)


def test_stand_in_refuses_what_the_entry_point_refuses():
    z = torch.zeros
    for M, K, dt, match in ((64, 256, torch.bfloat16, "rows"), (257, 256, torch.bfloat16, "rows"), (128, 384, torch.bfloat16, "multiple of 256"),
                            (128, 256, torch.float32, "bf16")):
        with pytest.raises(RuntimeError, match=match):
            emu_wide.gemm_skinny_wide(z((M, K), dtype=dt), z((16, K), dtype=dt), z((M, 16), dtype=dt))


def test_session_of_80_rows_has_its_folds(tiny, monkeypatch):
    from midi_model_amd.decode import DecodeSession
    with emu_wide.install() as log:
        m = _model(tiny[1])
        monkeypatch.delenv("MH_DECODE_WIDE", raising=False)
        for B in (80, 256):
            ses = DecodeSession(m, B, 256, 1.0, 0.98, 1)
            assert ses.wide and ses.fold1 is not None and ses.fold2 is not None and ses.lm_fold is not None and ses.fused_sampler, B
        ses = DecodeSession(m, 64, 256, 1.0, 0.98, 1)
        assert not ses.wide and ses.fold1 is not None and ses.lm_fold is not None           # as before
        ses = DecodeSession(m, 257, 256, 1.0, 0.98, 1)
        assert not ses.wide and ses.fold1 is None and ses.lm_fold is None                   # out of scope: the general form
        ses = DecodeSession(_model(tiny[1], torch.float32), 80, 256, 1.0, 0.98, 1)
        assert not ses.wide and ses.fold1 is None
        # the switch is read when the session is created, and the session keeps what it read
        monkeypatch.setenv("MH_DECODE_WIDE", "0")
        off = DecodeSession(m, 80, 256, 1.0, 0.98, 1)
        assert not off.wide and off.fold1 is None and off.lm_fold is None
        monkeypatch.delenv("MH_DECODE_WIDE")
        on = DecodeSession(m, 80, 256, 1.0, 0.98, 1)
        del log[:]
        on.seq.fill_(m.tokenizer.pad_id)
        on._net_body()
        on._tok_body(0)
        on._tok_body(1)
        L1, L2 = len(m._W["net"].layers), len(m._W["net_token"].layers)
        step = FOLDED_WIDE * L2 + ["gemm_skinny_wide", "sample_top_p_k"]
        assert [n for n in log if n != "exponential_"] == ["embed_sum_fwd"] + FOLDED_WIDE * L1 + ["rmsnorm_fwd"] + step + step, log
        monkeypatch.setenv("MH_DECODE_WIDE", "0")   # (set after the sessions were created: each keeps its form)
        del log[:]
        on._tok_body(2)
        assert log.count("gemm_skinny_wide") == 4 * L2 + 1 and "gemm_nt" not in log
        del log[:]
        off._net_body()
        assert "gemm_skinny_wide" not in log and log.count("gemm_nt") == 4 * L1


def _oracle_follows(orc, tok, sd, shp, out, first, bound):
    """teacher-forced oracle (one uncached fp32 pass over all rows of ``out`` [R, L, 8]): at every sampling position of events >=
    ``first`` the device's id must lie inside the grammar mask (EOS banned) and be the oracle's masked arg-max wherever its top-2
    margin exceeds ``bound``.  Positions with ONE legal id (margin inf) check nothing about a logit and are counted apart.
    -> (free positions checked, free positions, forced positions)"""
    ids = torch.from_numpy(out)
    R, L, T = ids.shape
    with torch.inference_mode():
        hidden = orc.midi_forward(sd, shp, ids[:, :-1])[:, first - 1:]           # hidden i predicts event i + 1
        n = R * hidden.shape[1]
        tgt = ids[:, first:].reshape(n, T)
        logits = orc.midi_forward_token(sd, shp, hidden.reshape(n, -1), tgt[:, :-1])
    names = [tok.id_events[int(t)] for t in tgt[:, 0]]
    checked = free = forced = 0
    bad = []
    for i in range(T):
        mask = orc.grammar_mask(tok, i, names if i else [""] * n, [False] * n, ban_eos=True).bool()
        assert mask.gather(1, tgt[:, i:i + 1]).all(), f"position {i}: an id outside the grammar mask"
        top2 = logits[:, i].masked_fill(~mask, float("-inf")).topk(2, -1)
        margin = top2.values[:, 0] - top2.values[:, 1]
        open_ = torch.isfinite(margin)
        safe = open_ & (margin > bound)
        free, forced, checked = free + int(open_.sum()), forced + int((~open_).sum()), checked + int(safe.sum())
        bad += [(int(k) // (L - first), first + int(k) % (L - first), i) for k in ((tgt[:, i] != top2.indices[:, 0]) & safe).nonzero().flatten()]
    assert not bad, f"device ids differ from the oracle's arg-max at (row, event, position): {bad[:8]}"
    return checked, free, forced


def _generate_80_and_follow(orc, tok, trained, monkeypatch, flaw=None):
    """generate(batch_size=80), greedy, EOS banned, bf16, ALL 80 rows followed by the teacher-forced oracle, each row continuing a
    prompt of its own (the golden's 13-event corpus prompt and four events sampled behind it), 8 events each.

    The criterion of test_ragged_host.py -- a top-2 margin of 1e-3, more than 0.95 of the positions safe -- is an fp32 criterion and
    CANNOT be met by a bf16 forward: the reference's own bf16 run of this model is 0.084 off its fp32 logits.  So the model and the
    bound are those of test_trained_gpu.py, both from the reference itself: the tiny model TRAINED with the reference
    (tests/golden/tiny_trained.npz; hidden 256, inner 1024 / 256, so a session folds; peaked distributions) and twice 1.5 x the
    reference's recorded bf16 logits drift FOR THIS MODEL as the margin that counts as safe (0.253).  The share is a condition on
    the oracle's margins, not a tolerance: of the FREE positions -- more than one legal id; the forced ones are counted apart and
    prove nothing -- more than half must be safe, which the golden's own held-out margins promise (their median, 2.3, is far above
    the bound; asserted below).  On these tokens the oracle is safe at 4144 of 5027 free positions (0.82; one position in eight of a
    note is the corpus's designed four-way velocity tie, so 0.875 is the ceiling).  Every safe position must carry the oracle's
    arg-max, in all 80 rows; a wide path that mixed up rows or roundings from row 64 on would part there.  The log shows that the
    wide path ran (gemm_nt is the prompt's prefill)."""
    monkeypatch.delenv("MH_DECODE_WIDE", raising=False)
    shp, sd, g = trained
    B, P, L = 80, 13 + 4, 13 + 4 + 8
    bound = 2 * 1.5 * float(g["ref_bf16_logits_maxerr"])
    assert float(np.median(g["eval_logits_margin"])) > bound     # the premise of "more than half of the free positions"
    with emu_wide.install() as log:
        # the prompts: the corpus prompt continued by four SAMPLED events (fp32, the general form: not the path under test), so that
        # every row stands somewhere else on the corpus's distribution
        prompt = _model(sd, torch.float32).generate(g["prompt"], batch_size=B, max_len=P, top_k=20, ban_eos=True,
                                                   generator=torch.Generator().manual_seed(5))
        assert prompt.shape == (B, P, 8) and len({prompt[b].tobytes() for b in range(B)}) > B // 2
        m = _model(sd)
        from midi_model_amd import ops
        stand_in = ops.gemm_skinny_wide
        if flaw is not None:   # a wrong wide kernel in the stand-in's place (logged under the same name), put back before install() ends
            ops.gemm_skinny_wide = emu_ragged._logged("gemm_skinny_wide", flaw, log)
        del log[:]
        try:
            out = m.generate(prompt, batch_size=B, max_len=L, top_k=1, ban_eos=True, generator=torch.Generator().manual_seed(2))
        finally:
            ops.gemm_skinny_wide = stand_in
        names = set(log)
        ses = m._sessions.idle[-1]
        assert ses.B == B and ses.wide and ses.fold1 is not None and ses.lm_fold is not None
    assert out.shape == (B, L, 8) and out.dtype == np.int64 and (out[:, :P] == prompt).all()
    assert "gemm_skinny_wide" in names and not names & {"gemm_skinny", "swiglu_fwd", "kv_append", "attn_decode"}, sorted(names)
    assert len({out[b, P:].tobytes() for b in range(B)}) > B // 2    # the rows do continue differently
    checked, free, forced = _oracle_follows(orc, tok, sd, shp, out, P, bound)
    total = free + forced
    print(f"generate(batch_size=80) bf16 (trained tiny): safe margin {bound:.4f}; {checked}/{free} free positions and {forced} forced ones "
          f"checked against the oracle's arg-max, all equal")
    assert total == B * (L - P) * 8
    assert checked > 0.5 * free, (checked, free)


def test_generate_80_rows_bf16_follows_the_oracle(orc, tok, trained, monkeypatch):
    _generate_80_and_follow(orc, tok, trained, monkeypatch)


@pytest.mark.parametrize("flaw", ["rows >= 64 read activation row m - 64", "rstd of row m taken from row m mod 64"])
def test_the_oracle_check_rejects_a_wrong_wide_path(orc, tok, trained, monkeypatch, flaw):
    """the same run with a wrong kernel behind ops.gemm_skinny_wide: the comparison above must fail -- it is not carried by forced
    positions or by rows below 64"""
    def wrong(a, w, out, *, mode=0, res=None, norm_eps=0.0, row_ids=None, res_ids=None):
        M = out.shape[0]
        rows = (a[row_ids] if row_ids is not None else a).clone()
        if flaw.startswith("rows"):
            rows[64:] = rows[:M - 64].clone()
            return emu_wide.gemm_skinny_wide(rows, w, out, mode=mode, res=res, norm_eps=norm_eps, res_ids=res_ids)
        emu_wide.gemm_skinny_wide(rows, w, out, mode=mode, res=None, norm_eps=0.0)   # the bare product, then the row scale by hand
        x = rows.float() @ w.float().T
        if norm_eps > 0:
            rstd = torch.rsqrt(rows.float().pow(2).mean(-1, keepdim=True) + norm_eps)
            x = x * rstd[torch.arange(M) % 64]
        if mode == 1:
            return emu_wide.emu_ops.swiglu_fwd(x.to(rows.dtype), out)
        if res is not None:
            x = x + (res[res_ids] if res_ids is not None else res).float()
        return out.copy_(x.to(out.dtype))
    with pytest.raises(AssertionError, match="differ from the oracle's arg-max|outside the grammar mask"):   # (_oracle_follows' two refusals)
        _generate_80_and_follow(orc, tok, trained, monkeypatch, flaw=wrong)


def test_equal_length_prompts_are_prefilled_as_generate_prefills_them(orc, tok, tiny, monkeypatch):
    """DecodeSession.prefill_ragged with prompts of ONE length runs the uniform forward of prefill() -- no sequence table, no packed
    store -- and leaves the state prefill() leaves, bit for bit; one prompt shorter and the packed forward runs.  80 rows, bf16."""
    from midi_model_amd.decode import DecodeSession
    monkeypatch.delenv("MH_DECODE_WIDE", raising=False)
    B, P = 80, 5
    prompt = orc.synthetic_events(tok, B, P, seed=33)
    with emu_wide.install() as log, torch.no_grad():
        m = _model(tiny[1])
        a = DecodeSession(m, B, 256, 1.0, 0.98, 1)
        r = DecodeSession(m, B, 256, 1.0, 0.98, 1, ragged=True)
        a.reset(), r.reset()
        _, plain = _run(log, lambda: a.prefill(prompt))
        _, names = _run(log, lambda: r.prefill_ragged(prompt.reshape(B * P, 8), [P] * B))
        assert names == plain and "attn_fwd_seqs" not in names and "kv_store_seqs" not in names, names[:8]
        assert torch.equal(a.hidden, r.hidden)   # (the caches are uninitialised memory behind the P rows written)
        assert torch.equal(a.kv1.k[:, :, :, :P], r.kv1.k[:, :, :, :P]) and torch.equal(a.kv1.v[:, :, :, :P], r.kv1.v[:, :, :, :P])
        assert r.pos.tolist() == [P] * B and r.kv1.len == 0 and int(a.pos.item()) == P
        lengths = [P] * (B - 1) + [P - 1]
        r.reset()
        _, names = _run(log, lambda: r.prefill_ragged(prompt.reshape(B * P, 8)[:-1], lengths))
        assert "attn_fwd_seqs" in names and "kv_store_seqs" in names and r.pos.tolist() == lengths
