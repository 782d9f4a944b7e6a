"""Packed training batches on the CPU: the launch tables of the table-form attention (ops.attn_seq_plan), the batch layout
(data.PackedBatch, WindowSampler.packed_batch / fill) and -- through the stand-ins of emu_packed.py over emu_ops.py -- the equality
of the packed step with the padded step on the same windows."""
import numpy as np
import pytest
import torch

import midi_model_amd as mm
from midi_model_amd import ops
from midi_model_amd.data import PackedBatch, TokenCorpus, WindowSampler
from midi_model_amd.train import TrainMIDIModel

import emu_packed

TABLES = [([1], 2), ([64], 2), ([65], 1), ([1, 1, 1], 2), ([63, 1, 64], 3), ([33, 200, 7, 128, 129], 2), ([515, 40], 2),
          ([128] * 3, 4), ([2048] * 16, 16), ([700, 13, 2048, 260, 1, 129, 5] * 3, 16)]


@pytest.mark.parametrize("passes", [5, 1, 64])
@pytest.mark.parametrize("lengths,H", TABLES, ids=[f"n{len(t)}max{max(t)}H{h}" for t, h in TABLES])
def test_seq_plan(lengths, H, passes):
    plan = ops.attn_seq_plan(lengths, H, passes=passes)
    seq_start, pos, work = (t.numpy() for t in plan.host_views())
    L = np.asarray(lengths)
    assert seq_start.tolist() == [0] + np.cumsum(L).tolist() and plan.M == L.sum() and plan.n == len(lengths)
    assert plan.Mpad == ((L + 63) // 64 * 64).sum() and plan.max_len == L.max()
    # pos[m] = m - start of m's sequence
    for i in range(len(lengths)):
        assert pos[seq_start[i]:seq_start[i + 1]].tolist() == list(range(lengths[i]))
    assert work.shape == (plan.nwork, 4) and plan.nwork % 8 == 0 and plan._off_work % 4 == 0
    live = work[work[:, 0] >= 0]
    # every (sequence, head, tile) exactly once
    want = {(i, h, r) for i in range(len(lengths)) for h in range(H) for r in range((lengths[i] + 127) // 128)}
    got = [tuple(r) for r in live[:, :3].tolist()]
    assert len(got) == len(want) and set(got) == want
    # the scratch offsets: 64-aligned, disjoint, in sequence order
    soff = np.concatenate([[0], np.cumsum((L + 63) // 64 * 64)])
    assert (live[:, 3] == soff[live[:, 0]]).all() and (live[:, 3] % 64 == 0).all()
    xcd_of = {}
    nt = (L + 127) // 128
    for x in range(8):
        mine = work[x::8]
        mine = mine[mine[:, 0] >= 0]
        for s, h in mine[:, :2].tolist():  # one (sequence, head) pair lives on one XCD
            assert xcd_of.setdefault((s, h), x) == x
        weight = nt[mine[:, 0]] - mine[:, 2]  # 128-row tiles the item reaches back over
        if passes >= nt.max():  # strict order: heaviest first across all sequences
            assert (np.diff(weight) <= 0).all()
        else:  # the weights' classes are non-increasing; a class never holds a heavier item than an earlier class's lightest
            P = min(passes, int(nt.max()))
            lo = np.arange(P) * int(nt.max()) // P
            cls = np.searchsorted(lo, nt.max() - weight, side="right") - 1
            assert (np.diff(cls) >= 0).all()
            for c in range(1, P):
                if (cls == c).any() and (cls < c).any():
                    assert weight[cls == c].max() <= weight[cls < c].min()
    # the XCDs' loads (sum of weights) differ by no more than the heaviest pair
    load = [int((nt[work[x::8][work[x::8][:, 0] >= 0][:, 0]] - work[x::8][work[x::8][:, 0] >= 0][:, 2]).sum()) for x in range(8)]
    heaviest = int(nt.max() * (nt.max() + 1) // 2)
    assert max(load) - min(load) <= heaviest


def test_seq_plan_equal_lengths_is_the_uniform_order():
    """16 x 2048, H = 16, 5 passes: an XCD walks pass after pass, pair after pair, ranks ascending -- what attn_work computes"""
    plan = ops.attn_seq_plan([2048] * 16, 16)
    work = plan.host_views()[2].numpy()
    assert plan.nwork == 16 * 16 * 16
    mine = work[0::8]
    bounds = [p * 16 // 5 for p in range(6)]
    k = 0
    for p in range(5):
        for pair in range(32):
            for r in range(bounds[p], bounds[p + 1]):
                assert mine[k, 2] == r and (mine[k, 0] * 16 + mine[k, 1]) == pair * 8, (k, mine[k])
                k += 1


def test_seq_plan_rejects_bad_tables():
    for bad in ([], [4, 0, 3], [-1], [3, 0]):
        with pytest.raises(ValueError):
            ops.attn_seq_plan(bad, 2)
    with pytest.raises(ValueError):
        ops.attn_seq_plan([4], 0)


def _padded(tok, lens, seed):
    g = torch.Generator().manual_seed(seed)
    L1 = max(lens)
    b = torch.randint(1, tok.vocab_size, (len(lens), L1, 8), generator=g)
    for i, n in enumerate(lens):
        b[i, n:] = tok.pad_id
    return b


@pytest.mark.parametrize("lens", [[18, 6, 3, 13], [1, 2, 9], [1, 1], [65, 2], [130]])
def test_from_padded_against_a_numpy_restatement(lens):
    tok = mm.MIDITokenizerV2()
    b = _padded(tok, lens, 3)
    pb = PackedBatch.from_padded(b, lens, tok.pad_id, n_head=4)
    bn = b.numpy()
    xs = [bn[i, :n - 1] for i, n in enumerate(lens)]
    ys = [bn[i, 1:n] for i, n in enumerate(lens)]
    real = sum(n - 1 for n in lens)
    M = max(64, (real + 63) // 64 * 64)
    want_x = np.full((M, 8), tok.pad_id, dtype=np.int64)
    want_y = want_x.copy()
    want_x[:real], want_y[:real] = np.concatenate(xs), np.concatenate(ys)
    assert pb.x.shape == (M, 8) and np.array_equal(pb.x.numpy(), want_x) and np.array_equal(pb.y.numpy(), want_y)
    seqs = [n - 1 for n in lens if n > 1] + ([M - real] if M > real else [])
    assert list(pb.lengths) == seqs and pb.tail == M - real and pb.real_rows == real
    assert pb.plan.lengths == tuple(seqs) and pb.plan.M == M and pb.plan.H == 4


def _corpus(tok, sizes, seed=5):
    rng = np.random.default_rng(seed)
    return TokenCorpus([rng.integers(1, tok.vocab_size, size=(n, 8)).astype(np.int16) for n in sizes], device="cpu")


def test_packed_batch_holds_the_windows_of_batch_and_leaves_the_rng_equal():
    tok = mm.MIDITokenizerV2()
    with emu_packed.install():
        corpus = _corpus(tok, [40, 3, 1, 25, 300, 2])
        a = WindowSampler(corpus, max_len=32, rand_start=True, seed=9)
        b = WindowSampler(corpus, max_len=32, rand_start=True, seed=9)
        for idx in ([0, 1, 2, 3], [4, 5, 0], [2, 2]):
            padded = a.batch(idx, tok.pad_id)
            wins = [n for n in (min(32, corpus.piece_len(i)) for i in idx)]  # upper bounds; the true lengths come from the pads
            pb = b.packed_batch(idx, tok.pad_id)
            lens = [int((padded[i] != tok.pad_id).any(-1).sum()) for i in range(len(idx))]
            assert all(n <= w for n, w in zip(lens, wins))
            ref = PackedBatch.from_padded(padded, lens, tok.pad_id)
            assert torch.equal(pb.x, ref.x) and torch.equal(pb.y, ref.y) and pb.lengths == ref.lengths
            assert a.rng.getstate() == b.rng.getstate()


def test_fill_never_crops_and_never_drops():
    tok = mm.MIDITokenizerV2()
    corpus = _corpus(tok, [40, 3, 1, 25, 300, 2, 64, 65, 10])
    s = WindowSampler(corpus, max_len=128, seed=1)
    order = [4, 0, 1, 2, 3, 4, 5, 6, 7, 8, 8, 0]
    state = s.rng.getstate()
    for budget in (1, 64, 100, 10 ** 6):
        batches = list(s.fill(iter(order), budget))
        assert [i for b in batches for i in b] == order  # nothing dropped, nothing reordered
        for b in batches:
            rows = sum(max(min(128, corpus.piece_len(i)) - 1, 0) for i in b)
            assert rows <= budget or len(b) == 1  # only a window that alone exceeds the budget goes over it -- whole
    assert s.rng.getstate() == state


def test_packed_step_equals_the_padded_step(orc):
    """Through the CPU stand-ins, the whole step in float64 (emu_packed.float64_arithmetic): the packed step's loss and every
    gradient equal the padded step's on the same windows to float64 rounding.  Both steps take the same non-ignored targets and
    every target's logits depend on rows of its own window only, so the two differ in nothing but the order of sums over rows.
    Bound: the longest such sum has R = 512 terms (64 rows x 8 tokens), so an entry may move by R eps64 times the sum of the
    magnitudes of its terms, taken here as the tensor's largest entry: 512 x 2.2e-16 = 1.2e-13 of it (a wrong row, mask or position
    moves entries by 1e-3 and more); entries that are not small against it must also agree to 1e-9 relative.  Losses: 64 eps64.
    The tail sequence: the gradient that reaches its rows of the event-level stack's input is exactly zero -- observed where the
    step hands it to the embedding's backward, whose skipping of pad ids would otherwise hide it."""
    from midi_model_amd import ops as real_ops
    tok = mm.MIDITokenizerV2()
    shp = orc.Shape(n_layer=4, n_head=4, n_embd=256, n_inner=512, vocab=tok.vocab_size)
    sd = orc.make_state_dict(shp, seed=1)
    lens = [18, 6, 3, 13, 1]
    batch = orc.synthetic_events(tok, len(lens), max(lens), seed=2)
    for i, n in enumerate(lens):
        batch[i, n:] = tok.pad_id
    cfg = mm.MIDIModelConfig.get_config("v2", True, 4, 4, 256, 512)
    eps = torch.finfo(torch.float64).eps
    with emu_packed.install(), emu_packed.float64_arithmetic():
        outs, seen = [], []
        inner = real_ops.embed_segment_bwd

        def spy(src_rows, seg_start, dout, ld, dtable_f32, pad_id):
            seen.append(dout.detach().clone())
            return inner(src_rows, seg_start, dout, ld, dtable_f32, pad_id)

        real_ops.embed_segment_bwd = spy
        try:
            for packed in (False, True):
                m = TrainMIDIModel(cfg, accumulate_grad_batches=1)
                m.load_state_dict(sd)
                m = m.to(torch.float64)
                b = PackedBatch.from_padded(batch, lens, tok.pad_id) if packed else batch
                del seen[:]
                loss = m.training_step(b)
                dx = [t for t in seen if t.shape == (64, 256)] if packed else []
                vloss, acc = m.validation_step(b)
                outs.append((loss.item(), vloss.item(), float(acc), {k: p.grad.clone() for k, p in m.named_parameters()}, dx))
        finally:
            real_ops.embed_segment_bwd = inner
        pb = PackedBatch.from_padded(batch, lens, tok.pad_id)
        assert pb.tail == 28 and pb.real_rows == 36 and pb.plan is None
        assert (pb.x[pb.real_rows:] == tok.pad_id).all() and (pb.y[pb.real_rows:] == tok.pad_id).all()
        m = TrainMIDIModel(cfg, accumulate_grad_batches=1, sample_seq=True)
        m.load_state_dict(sd)
        with pytest.raises(NotImplementedError):
            m.training_step(pb)
    (la, va, aa, ga, _), (lb, vb, ab, gb, dx) = outs
    assert ga["lm_head.weight"].dtype == torch.float64
    assert abs(la - lb) <= 64 * eps * abs(la) and abs(va - vb) <= 64 * eps * abs(va) and aa == ab, (la, lb, va, vb, aa, ab)
    for k in ga:
        top = ga[k].abs().max().item()
        d = (ga[k] - gb[k]).abs()
        assert top > 0 and d.max().item() <= 512 * eps * top, (k, d.max().item(), top)
        big = ga[k].abs() > 1e-4 * top
        assert (d[big] <= 1e-9 * ga[k].abs()[big]).all(), k
    # the tail: d loss / d (its rows of the event-level net's input) as the step computed it
    assert len(dx) == 1, [tuple(t.shape) for t in dx]
    assert dx[0][:36].abs().max().item() > 0 and (dx[0][36:] == 0).all(), dx[0][36:].abs().max().item()
