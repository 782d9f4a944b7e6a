"""Forking inside the decode pool on the CPU: DecodeSession.fork / hold (decode.py), DecodePool.submit(n=, hold=) / fork / held / drop
(pool.py) and ops.kv_fork_rows' checks, through the fake backend plus the stand-in of mh_kv_fork_rows (tests/emu_fork.py).  Tiny
4-layer model, fp32.  The kernel itself: test_fork_kernels_gpu.py; the production session: test_fork_gpu.py."""
import numpy as np
import pytest
import torch

import midi_model_amd as mm

import emu_fork
import emu_seeded
import fork_common as fc
import ragged_common as rc

FORWARD_OPS = ("embed", "gemm", "attn", "norm", "rope", "swiglu", "kv_store", "kv_append")   # (substrings of the forward's op names)


@pytest.fixture(scope="module")
def tok():
    return mm.MIDITokenizerV2()


@pytest.fixture(scope="module")
def tiny(orc, tok):
    shp = orc.Shape(n_layer=4, n_head=4, n_embd=256, n_inner=512, vocab=tok.vocab_size)
    return shp, orc.make_state_dict(shp, seed=0)


def _model(sd):
    m = mm.MIDIModel(mm.MIDIModelConfig.get_config("v2", True, 4, 4, 256, 512))
    m.load_state_dict(sd)
    return m.to(torch.float32)


def test_a_child_repeats_its_parent(orc, tok, tiny):
    with emu_fork.install() as log:
        m = _model(tiny[1])
        fc.child_repeats_parent(m, orc, tok, 64)
        assert log.count("kv_fork_rows") == 1 and len(m._sessions.idle) == 1


def test_siblings_equal_lone_requests(orc, tok, tiny):
    with emu_fork.install() as log:
        m = _model(tiny[1])
        fc.siblings_equal_lone_requests(m, orc, tok, 64)
        assert log.count("kv_fork_rows") == 1 and len(m._sessions.idle) == 1


@pytest.mark.parametrize("alone", (False, True))
def test_a_held_request_forked_later_equals_an_uninterrupted_one(orc, tok, tiny, alone):
    with emu_fork.install() as log:
        m = _model(tiny[1])
        ses = fc.held_then_forked_equals_uninterrupted(m, orc, tok, 64, 3, alone)
        assert log.count("kv_fork_rows") == 1 and m._sessions.idle == [ses]
        assert ses.held_hidden is not None and ses.held_hidden.shape == ses.hidden.shape


def test_a_greedy_child_in_an_unseeded_pool(orc, tok, tiny):
    with emu_fork.install():
        m = _model(tiny[1])
        ses = fc.greedy_child_in_an_unseeded_pool(m, orc, tok, 64)
        assert not ses.seeded and ses.q_all is not None


def test_call_log(orc, tok, tiny):
    """a fork is ONE kv_fork_rows and nothing else; an admission of n=3 is the forward of one prompt + one kv_fork_rows; a pool that
    never forks logs what it logs without this feature's stand-in installed"""
    p, q = rc.prompts(orc, tok, (7, 4), seed0=560)

    def never_forks(m):
        with m.decode_pool(3, 64, seeded=True) as pool:
            ids = [pool.submit(x, max_len=len(x) + n, seed=s, **fc.KW) for x, n, s in ((p, 5, 1), (q, 3, 2), (p, 4, 3), (q, 6, 4))]
            fc.drain(pool)
            return [pool.result(i) for i in ids]

    with emu_seeded.install() as log0:
        m = _model(tiny[1])
        del log0[:]
        a, la = never_forks(m), list(log0)
    with emu_fork.install() as log:
        m = _model(tiny[1])
        del log[:]
        b, lb = never_forks(m), list(log)
        assert la == lb and "kv_fork_rows" not in lb and all(fc.same(x, y) for x, y in zip(a, b))
        assert any(any(s in name for s in FORWARD_OPS) for name in lb), "FORWARD_OPS names nothing the forward logs"
        # ---- one lone admission against an admission of three siblings, each the first step of a fresh pool
        with m.decode_pool(4, 64, seeded=True) as pool:
            pool.submit(p, max_len=20, seed=1, **fc.KW)
            del log[:]
            pool.step()
            lone = list(log)
        with m.decode_pool(4, 64, seeded=True) as pool:
            par, _, _ = pool.submit(p, max_len=20, seed=[1, 2, 3], n=3, **fc.KW)
            del log[:]
            pool.step()
            three = list(log)
            assert three.count("kv_fork_rows") == 1 and [n for n in three if n != "kv_fork_rows"] == lone
            assert three.count("embed_sum_fwd") == lone.count("embed_sum_fwd") and "embed_sum_fwd" in lone
            # the fork sits right behind the prefill's last K/V store, ahead of everything the token steps log
            at = three.index("kv_fork_rows")
            assert three[at - 1] == "kv_store_seqs_rows" and "kv_store_seqs_rows" not in three[at:]
            # ---- a fork: exactly one kv_fork_rows, no forward op
            del log[:]
            pool.fork(par, seed=9)
            assert list(log) == ["kv_fork_rows"], log
            assert not any(s in name for name in log for s in FORWARD_OPS)


def test_bookkeeping(orc, tok, tiny):
    """rows lowest first, held() / pending(), drop() frees the row at pos == 0 == pos_limit, a sibling group waits whole and later
    requests wait behind it"""
    p, q = rc.prompts(orc, tok, (4, 6), seed0=570)
    with emu_fork.install():
        m = _model(tiny[1])
        with m.decode_pool(4, 64) as pool:
            a = pool.submit(p, max_len=7, top_k=1, ban_eos=True, hold=True)    # 3 events, then held in row 0
            b = pool.submit(q, max_len=30, top_k=1, ban_eos=True)              # row 1
            pool.step()
            ses = pool.ses
            assert pool.occupied == {0: a, 1: b} and pool.free == [2, 3] and ses.pos.tolist() == [5, 7, 0, 0]
            # a group of three does not fit two free rows: it waits whole, and the lone request behind it waits too
            g = pool.submit(q, max_len=12, top_k=1, ban_eos=True, n=3)
            c = pool.submit(p, max_len=9, top_k=1, ban_eos=True)
            assert g == [2, 3, 4] and c == 5 and pool.pending() == 6
            pool.step()
            assert list(pool.queue) == g + [c] and pool.free == [2, 3] and pool.occupied == {0: a, 1: b}
            out = pool.step()   # a reaches max_len 7: held, its row is NOT freed, so the group still waits
            assert [(r, d) for r, _, d in out] == [(a, True), (b, False)]
            assert pool.held() == [a] and pool.pending() == 5 and pool.free == [2, 3] and pool.held_rows == {0: a}
            assert ses.pos.tolist()[:2] == [7, 9] and ses.pos_limit.tolist()[:2] == [7, 30]
            out = pool.step()
            assert [r for r, _, _ in out] == [b] and list(pool.queue) == g + [c]
            # a fork takes the lowest free rows, ahead of the queue
            k = pool.fork(a, count=2, max_len=10)
            assert k == [6, 7] and pool.occupied == {1: b, 2: 6, 3: 7} and pool.free == [] and pool.pending() == 7
            assert ses.pos.tolist() == [7, 10, 7, 7] and ses.pos_limit.tolist() == [7, 30, 10, 10]
            with pytest.raises(ValueError, match="0 are free"):
                pool.fork(a, max_len=10)
            for _ in range(3):
                pool.step()   # the children finish (10 events) and free rows 2 and 3; the group of three still needs one more
            assert pool.free == [2, 3] and list(pool.queue) == g + [c] and pool.held() == [a]
            assert fc.same(pool.result(6), pool.result(7)) and len(pool.result(6)) == 10 and (pool.result(6)[:7] == pool.result(a)).all()
            pool.drop(a)
            assert pool.held() == [] and pool.free == [0, 2, 3] and ses.pos.tolist()[0] == 0 and ses.pos_limit.tolist()[0] == 0
            assert pool.requests[a].row is None and len(pool.result(a)) == 7
            with pytest.raises(ValueError, match="holds no row"):
                pool.drop(a)
            pool.step()   # the group goes in whole, rows 0, 2, 3; c waits for a row
            assert pool.occupied == {1: b, 0: g[0], 2: g[1], 3: g[2]} and list(pool.queue) == [c]
            fc.drain(pool)
            res = [pool.result(i) for i in g]
            assert all(len(r) == 12 for r in res) and fc.same(res[0], res[1]) and fc.same(res[0], res[2]), "greedy siblings"
            assert len(pool.result(c)) == 9 and pool.free == [0, 1, 2, 3]
        # held rows that block a group with nothing running: step() says so instead of spinning
        with m.decode_pool(2, 64) as pool:
            a = pool.submit(p, max_len=5, top_k=1, ban_eos=True, hold=True)
            fc.drain(pool)
            pool.submit(p, max_len=6, top_k=1, ban_eos=True, n=2)
            with pytest.raises(RuntimeError, match="drop"):
                pool.step()
            pool.drop(a)
            fc.drain(pool)
            assert pool.free == [0, 1]


def test_refusals_come_before_any_backend_call(orc, tok, tiny):
    from midi_model_amd import ops
    from midi_model_amd.decode import DecodeSession
    from midi_model_amd.ops_fork import check_pairs
    p, q = rc.prompts(orc, tok, (4, 6), seed0=580)
    V = tok.vocab_size
    with emu_fork.install() as log:
        m = _model(tiny[1])
        # ---- submit(n=), in a seeded and in an unseeded pool
        pool = m.decode_pool(3, 64, seeded=True)
        del log[:]
        for kw, match in ((dict(n=0, seed=1), "n = 0"), (dict(n=4, seed=[1, 2, 3, 4]), "n = 4"), (dict(n=1.0, seed=1), "n = 1.0"),
                          (dict(n=True, seed=1), "n = True"), (dict(n=2, seed=7), "not the scalar 7"),
                          (dict(n=2, seed=[1]), "it holds 1"), (dict(n=2, seed=[1, 2, 3]), "it holds 3"),
                          (dict(n=2, seed=[1, -1]), "row 0"), (dict(n=2, seed=[True, 1]), "row 0"), (dict(n=2), "needs a seed"),
                          (dict(n=2, seed=[1, 2], top_k=65), "top_k"), (dict(n=2, seed=[1, 2], max_len=64), "capacity 64")):
            with pytest.raises(ValueError, match=match):
                pool.submit(p, **{"max_len": 9, **kw})
        assert pool.pending() == 0 and not pool.requests and not log and pool.ses is None
        plain = m.decode_pool(3, 64)
        with pytest.raises(ValueError, match="seeded=True"):
            plain.submit(p, max_len=9, n=2, seed=[1, 2])
        assert not log
        plain.close()
        # ---- fork
        with pytest.raises(ValueError, match="no request"):
            pool.fork(0, seed=1)
        a = pool.submit(p, max_len=6, seed=1, hold=True, **fc.KW)       # held after two steps
        b = pool.submit(q, max_len=8, seed=2, **fc.KW)                  # released after two steps
        w = pool.submit(q, max_len=30, seed=3, **fc.KW)
        queued = pool.submit(q, max_len=9, seed=4, **fc.KW)
        with pytest.raises(ValueError, match="still queued"):
            pool.fork(a, seed=1)
        pool.step()
        pool.step()
        assert pool.held() == [a] and pool.requests[b].done and pool.occupied == {2: w} and pool.free == [1]
        pool.step()   # the queued request takes row 1
        assert pool.occupied == {2: w, 1: queued} and pool.free == []
        del log[:]
        for rid, kw, match in ((99, dict(seed=1), "no request"), ("0", dict(seed=1), "no request"), (True, dict(seed=1), "no request"),
                               (b, dict(seed=1), "released")):
            with pytest.raises(ValueError, match=match):
                pool.fork(rid, **kw)
        with pytest.raises(ValueError, match="0 are free"):
            pool.fork(a, max_len=12, seed=1)
        while not pool.requests[queued].done:
            pool.step()
        del log[:]
        assert pool.free == [1]
        with pytest.raises(ValueError, match="released"):
            pool.fork(queued, max_len=20, seed=1)
        for kw, match in ((dict(seed=1), "nothing to generate"),                      # (max_len defaults to the parent's 6)
                          (dict(max_len=6, seed=1), "nothing to generate"), (dict(max_len=5, seed=1), "nothing to generate"),
                          (dict(max_len=64, seed=1), "capacity 64"), (dict(max_len=12.5, seed=1), "not an integer"),
                          (dict(max_len=12), "needs a seed"), (dict(max_len=12, seed=[1]), "one seed"),
                          (dict(max_len=12, seed=-1), "row 0"), (dict(max_len=12, seed=1, count=0), "count = 0"),
                          (dict(max_len=12, seed=1, count=4), "count = 4"), (dict(max_len=12, seed=1, count=2), "1 are free"),
                          (dict(max_len=12, seed=1, temp=0.0), "temperature"), (dict(max_len=12, seed=1, top_k=0), "top_k"),
                          (dict(max_len=12, seed=1, disable_channels=[16]), "disable_channels")):
            with pytest.raises(ValueError, match=match):
                pool.fork(a, **kw)
        assert not log and pool.free == [1] and pool.held() == [a]
        with pytest.raises(ValueError, match="holds no row"):
            pool.drop(w)
        with pytest.raises(ValueError, match="holds no row"):
            pool.drop(99)
        assert not log
        pool.close()
        for call in (lambda: pool.fork(a, max_len=12, seed=1), lambda: pool.drop(a)):
            with pytest.raises(ValueError, match="closed|holds no row"):
                call()
        plain = m.decode_pool(2, 64)
        c = plain.submit(p, max_len=9, top_k=1)
        plain.step()
        del log[:]
        with pytest.raises(ValueError, match="seeded=True"):
            plain.fork(c, seed=1)
        assert not log
        plain.close()
        # ---- the session itself
        masks, toks = torch.zeros((1, V), dtype=torch.uint8), torch.from_numpy(p)
        with torch.inference_mode():
            flat = DecodeSession(m, 3, 64, 1.0, 0.98, 1, ragged=True)
            ses = DecodeSession(m, 3, 64, 1.0, 0.98, 1, ragged=True, row_params=True)
            seeded = DecodeSession(m, 3, 64, 1.0, 0.98, 1, ragged=True, row_params=True, seeded=True)
        del log[:]
        with pytest.raises(ValueError, match="row_params"):
            flat.fork([0], [1], [4], [9], [1.0], [0.98], [1], masks, masks)
        with pytest.raises(ValueError, match="row_params"):
            flat.hold([0])
        two = masks.repeat(2, 1)
        for src, dst, lens, lims, k, fm, kw, match in (
                ([0], [3], [4], [9], [1], masks, {}, "outside"),
                ([-1], [1], [4], [9], [1], masks, {}, "outside"),
                ([0, 0], [1, 1], [4, 4], [9, 9], [1, 1], two, {}, "named twice"),
                ([0, 1], [1, 2], [4, 4], [9, 9], [1, 1], two, {}, "source and destination"),
                ([0], [0], [4], [9], [1], masks, {}, "source and destination"),
                ([0, 0], [1], [4], [9], [1], masks, {}, "one of each"),
                ([], [], [], [], [], masks[:0], {}, "one of each"),
                ([0], [1], [0], [9], [1], masks, {}, r"length outside \[1, 64\]"),
                ([0], [1], [65], [70], [1], masks, {}, "length outside"),
                ([0], [1], [10], [9], [1], masks, {}, "capacity"),
                ([0], [1], [4], [64], [1], masks, {}, "capacity"),
                ([0], [1], [4], [9, 9], [1], masks, {}, "limits"),
                ([0], [1], [4], [9], [0], masks, {}, "top_k"),
                ([0], [1], [4], [9], [65], masks, {}, "top_k"),
                ([0], [1], [4], [9], [1], masks[:, :-1], {}, "uint8"),
                ([0], [1], [4], [9], [1], masks.long(), {}, "uint8"),
                ([0], [1], [4], [9], [1], masks, dict(seeds=[1]), "seeded=True session only"),
                ([0], [1], [4], [9], [1], masks, dict(from_held=[True, False]), "from_held"),
                ([0], [1], [4], [9], [1], masks, dict(from_held=[True]), "has kept none"),
        ):
            n = len(lens)
            with pytest.raises(ValueError, match=match):
                ses.fork(src, dst, lens, lims, [1.0] * n, [0.98] * n, k, fm, masks.repeat(n, 1), **kw)
        for seeds, match in ((None, "no seeds"), ([1, 2], "2 seeds for 1"), ([True], "not an integer"), ([1 << 64], "not an integer")):
            with pytest.raises(ValueError, match=match):
                seeded.fork([0], [1], [4], [9], [1.0], [0.98], [1], masks, masks, seeds=seeds)
        with pytest.raises(ValueError, match="outside"):
            ses.hold([3])
        with pytest.raises(ValueError, match="twice"):
            ses.hold([1, 1])
        assert not log and ses.held_hidden is None
        # ---- the wrapper's own checks (the stand-in restates them) and the device copy
        assert check_pairs([0, 0], (1, 2), np.array([3, 40]), 6, 40) == ([0, 0], [1, 2], [3, 40])
        k = torch.zeros((2, 6, 2, 40, 8))
        for src, dst, lens, match in (([0], [6], [3], "outside"), ([0], [1, 2], [3], "destinations"), ([0, 3], [1, 1], [3, 3], "twice"),
                                      ([0, 1], [1, 2], [3, 3], "at once"), ([0], [1], [41], "length"), ([0], [1], [0], "length")):
            with pytest.raises(ValueError, match=match):
                check_pairs(src, dst, lens, 6, 40)
            with pytest.raises(ValueError, match=match):
                ops.kv_fork_rows(k, k.clone(), src, dst, lens)
        assert log == ["kv_fork_rows"] * 6   # (the stand-in was reached and refused; the real wrapper refuses before lib().call)
