"""Prefix slots inside the decode pool on the CPU: DecodeSession(prefix_slots=, prefix_capacity=) with admit(slots=) / fork(join=) /
release (decode.py), DecodePool.submit(share_prefix=) / fork / drop / close (pool.py), through the fake backend plus the stand-ins of
the two slot kernels (tests/emu_poolshare.py, layered on emu_fork).  Tiny 4-layer model, fp32.  The kernels themselves:
test_poolshare_kernels_gpu.py; the production session: test_poolshare_gpu.py."""
import numpy as np
import pytest
import torch

import midi_model_amd as mm

import emu_fork
import emu_poolshare
import fork_common as fc
import poolshare_common as pc
import ragged_common as rc

SLOTS = dict(prefix_slots=2, prefix_capacity=16)
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


def test_a_child_of_a_sharing_parent_repeats_it(orc, tok, tiny):
    with emu_poolshare.install() as log:
        m = _model(tiny[1])
        ses = pc.child_repeats_parent(m, orc, tok, 4, 64, SLOTS, 7)
        assert log.count("kv_fork_rows") == 1 and m._sessions.idle == [ses] and ses.prefix_slots == 2 and ses.prefix_capacity == 256


def test_a_held_sharing_request_forked_later_equals_an_uninterrupted_one(orc, tok, tiny):
    with emu_poolshare.install() as log:
        m = _model(tiny[1])
        ses = pc.held_then_forked_equals_uninterrupted(m, orc, tok, 4, 64, SLOTS, 3)
        assert log.count("kv_fork_rows") == 1 and m._sessions.idle == [ses]


def test_ids_do_not_depend_on_the_group_or_the_other_slots(orc, tok, tiny):
    with emu_poolshare.install() as log:
        m = _model(tiny[1])
        pc.ids_do_not_depend_on_the_group(m, orc, tok, 8, 64, SLOTS, 9)
        assert "kv_fork_rows" not in log, "siblings that share a prompt copy nothing"


def test_rows_that_share_nothing_equal_a_pool_without_slots(orc, tok, tiny):
    with emu_poolshare.install():
        m = _model(tiny[1])
        pc.rows_that_share_nothing(m, orc, tok, 8, 64, SLOTS, (5, 8, 3))


def test_in_the_exact_emulation_a_sharing_request_equals_the_same_request_unshared(orc, tok, tiny):
    """the stand-in attends to the slot's rows and the row's own in ONE float64 softmax -- the keys of a row that owns a copy of its
    prompt, in the same order -- so sharing changes no id here (on the device the prefix half rounds P to bf16: no such promise)"""
    p = rc.prompts(orc, tok, (11,), seed0=680)[0]
    with emu_poolshare.install():
        m = _model(tiny[1])
        out = []
        for share in (False, True):
            with m.decode_pool(4, 64, seeded=True, **SLOTS) as pool:
                ids = pool.submit(p, max_len=24, seed=[3, 4, 5], n=3, share_prefix=share, **fc.KW)
                fc.drain(pool)
                out.append([pool.result(i) for i in ids])
        for a, b in zip(*out):
            assert a.shape == (24, 8) and fc.same(a, b), np.argwhere(a != b)[:4]
        assert not fc.same(out[0][0], out[0][1])


def test_call_log(orc, tok, tiny):
    """an admission of n = 3 with share_prefix is ONE prompt's forward and no kv_fork_rows; a fork of a sharing parent is one
    kv_fork_rows of the suffix length, or nothing at all when the suffix is empty; a pool without slots logs what it logs without this
    feature's stand-ins installed"""
    import midi_model_amd.ops as real
    p, q = rc.prompts(orc, tok, (7, 4), seed0=560)

    def without_slots(m):
        with m.decode_pool(5, 64, seeded=True) as pool:
            ids = [pool.submit(x, max_len=len(x) + n, seed=s, **fc.KW) for x, n, s in ((p, 5, 1), (q, 3, 2))]
            ids += pool.submit(p, max_len=12, seed=[3, 4], n=2, **fc.KW)
            pool.step()
            ids += pool.fork(ids[0], seed=9)
            fc.drain(pool)
            return [pool.result(i) for i in ids]

    with emu_fork.install() as log0:
        m = _model(tiny[1])
        del log0[:]
        a, la = without_slots(m), list(log0)
    with emu_poolshare.install() as log:
        m = _model(tiny[1])
        del log[:]
        b, lb = without_slots(m), list(log)
        assert la == lb and lb.count("kv_fork_rows") == 2 and all(fc.same(x, y) for x, y in zip(a, b))
        assert not any(n in lb for n in emu_poolshare._NAMES)
        # ---- one lone admission against an admission of three sharing siblings, each the first step of a fresh pool with slots
        with m.decode_pool(4, 64, seeded=True, **SLOTS) as pool:
            pool.submit(p, max_len=20, seed=1, **fc.KW)
            del log[:]
            pool.step()
            lone = list(log)
        with m.decode_pool(4, 64, seeded=True, **SLOTS) as pool:
            par, sib, _ = pool.submit(p, max_len=20, seed=[1, 2, 3], n=3, share_prefix=True, **fc.KW)
            del log[:]
            pool.step()
            three = list(log)
            assert three == lone and "kv_fork_rows" not in three and three.count("embed_sum_fwd") == 2  # (the prompt's, the event's)
            layers = len(m._W["net"].layers)
            assert three.count("attn_prefix_partial_slots") == layers == three.count("attn_decode_append_rows_shared")
            assert "attn_decode_append_rows" not in three
            ses = pool.ses
            assert ses.slot_refs == [3, 0] and ses.row_slot.tolist() == [0, 0, 0, -1] and ses.slot_len.tolist() == [7, 0]
            # ---- a fork of a sharing parent: one copy, of the parent's own rows alone, and no forward op
            seen, inner = [], real.kv_fork_rows
            real.kv_fork_rows = lambda *a, **k: (seen.append((list(a[2]), list(a[3]), list(a[4]))), inner(*a, **k))[1]
            try:
                pool.step()
                pool.step()     # the parent now holds 7 + 3 events: 3 cache rows of its own behind the slot's 7
                del log[:]
                kid, = pool.fork(par, seed=9)
                assert list(log) == ["kv_fork_rows"] and seen == [([0], [3], [3])], (log, seen)
                k1 = ses.kv1.k
                assert torch.equal(k1[:, 3, :, :3], k1[:, 0, :, :3]) and ses.pos.tolist()[3] == 10 and ses.slot_refs == [4, 0]
            finally:
                real.kv_fork_rows = inner
        # ---- an empty suffix is a parent that stands right behind its prompt: straight from the session, no launch at all
        with torch.inference_mode():
            from midi_model_amd.decode import DecodeSession
            s2 = DecodeSession(m, 4, 64, 1.0, 0.98, 1, ragged=True, row_params=True, **SLOTS)
            masks = torch.zeros((1, tok.vocab_size), dtype=torch.uint8)
            s2.admit([1], torch.from_numpy(p), [7], [20], [1.0], [0.98], [1], masks, masks, slots=[1])
            del log[:]
            s2.fork([1], [2], [7], [20], [1.0], [0.98], [1], masks, masks, join=[True])
            assert list(log) == [] and s2.slot_refs == [0, 2] and s2.row_slot.tolist() == [-1, 1, 1, -1] and s2.pos.tolist() == [0, 7, 7, 0]
            assert torch.equal(s2.hidden[2], s2.hidden[1])
            s2.release([1])
            assert s2.slot_refs == [0, 1] and s2.slot_len.tolist() == [0, 7]
            s2.release([2])
            assert s2.slot_refs == [0, 0] and s2.slot_len.tolist() == [0, 0] and s2.free_slots() == [0, 1]


def test_bookkeeping(orc, tok, tiny):
    """slot reference counts through release, hold, drop, fork and close; a slot is reused after its last member leaves; a group
    waits for a slot at the head of the queue, what is queued behind it waits too, and step() says so when nothing can run"""
    p, q = rc.prompts(orc, tok, (4, 6), seed0=570)
    one = dict(prefix_slots=1, prefix_capacity=16)
    greedy = dict(top_k=1, ban_eos=True)
    with emu_poolshare.install():
        m = _model(tiny[1])
        with m.decode_pool(4, 64, **one) as pool:
            a0, a1 = pool.submit(p, max_len=7, n=2, share_prefix=True, hold=True, **greedy)
            b = pool.submit(q, max_len=8, share_prefix=True, **greedy)     # waits for the one slot
            c = pool.submit(p, max_len=9, **greedy)                        # shares nothing, but waits behind b
            pool.step()
            ses = pool.ses
            assert pool.occupied == {0: a0, 1: a1} and list(pool.queue) == [b, c] and pool.free == [2, 3]
            assert ses.slot_refs == [2] and ses.row_slot.tolist() == [0, 0, -1, -1] and ses.slot_len.tolist() == [4]
            assert ses.pos.tolist() == [5, 5, 0, 0]
            pool.step()
            pool.step()
            assert pool.held() == [a0, a1] and ses.slot_refs == [2] and list(pool.queue) == [b, c], "held rows keep their slot"
            with pytest.raises(RuntimeError, match="0 of 1 prefix slots"):
                pool.step()
            k, = pool.fork(a0, max_len=10)
            assert ses.slot_refs == [3] and ses.row_slot.tolist() == [0, 0, 0, -1] and pool.requests[k].share
            pool.drop(a0)
            assert ses.slot_refs == [2] and ses.row_slot.tolist() == [-1, 0, 0, -1] and ses.slot_len.tolist() == [4]
            pool.step()
            assert list(pool.queue) == [b, c], "the slot is still in use: b waits, and c behind it"
            pool.drop(a1)
            assert ses.slot_refs == [1] and ses.slot_len.tolist() == [4]
            pool.step()
            out = pool.step()    # the child's third event: it holds 10, leaves, and the slot is emptied behind it
            assert [(r, d) for r, _, d in out] == [(k, True)] and ses.slot_refs == [0] and ses.slot_len.tolist() == [0]
            assert fc.same(pool.result(k)[:7], pool.result(a0)) and fc.same(pool.result(a0), pool.result(a1)), "greedy"
            pool.step()          # b takes the slot that was freed, c a row
            assert pool.occupied == {0: b, 1: c} and ses.slot_refs == [1] and ses.slot_len.tolist() == [6]
            assert ses.row_slot.tolist() == [0, -1, -1, -1]
            fc.drain(pool)
            assert pool.free == [0, 1, 2, 3] and ses.slot_refs == [0] and ses.slot_len.tolist() == [0] and ses.free_slots() == [0]
            assert len(pool.result(b)) == 8 and len(pool.result(c)) == 9
        # ---- close() ends everything
        pool = m.decode_pool(4, 64, **one)
        pool.submit(p, max_len=20, n=3, share_prefix=True, hold=True, **greedy)
        pool.step()
        assert pool.ses is ses and ses.slot_refs == [3]
        pool.close()
        assert ses.slot_refs == [0] and ses.slot_len.tolist() == [0] and ses.row_slot.tolist() == [-1] * 4 and ses.pos.tolist() == [0] * 4


def test_refusals_come_before_any_backend_call(orc, tok, tiny):
    from midi_model_amd.decode import DecodeSession
    p, q = rc.prompts(orc, tok, (4, 20), seed0=580)
    V = tok.vocab_size
    with emu_poolshare.install() as log:
        m = _model(tiny[1])
        del log[:]
        # ---- decode_pool and submit
        for kw, match in ((dict(prefix_slots=1), "prefix_slots=1"), (dict(prefix_capacity=16), "prefix_slots=0"),
                          (dict(prefix_slots=-1, prefix_capacity=16), "prefix_slots=-1"),
                          (dict(prefix_slots=True, prefix_capacity=16), "prefix_slots=True"),
                          (dict(prefix_slots=1.5, prefix_capacity=16), "prefix_slots=1.5")):
            with pytest.raises(ValueError, match=match):
                m.decode_pool(3, 64, **kw)
        plain = m.decode_pool(3, 64)
        with pytest.raises(ValueError, match="needs a pool with prefix slots"):
            plain.submit(p, max_len=9, share_prefix=True)
        pool = m.decode_pool(3, 64, prefix_slots=1, prefix_capacity=16)
        with pytest.raises(ValueError, match="20 events in a pool whose prefix slots hold 16"):
            pool.submit(q, max_len=30, share_prefix=True)
        assert pool.submit(q, max_len=30) == 0, "the same prompt, shared with nobody, is admitted"
        assert not log and pool.ses is None and plain.pending() == 0
        plain.close()
        pool.close()
        # ---- the session
        masks, toks = torch.zeros((1, V), dtype=torch.uint8), torch.from_numpy(p)
        with pytest.raises(ValueError, match="per-row session"):
            DecodeSession(m, 3, 64, 1.0, 0.98, 1, ragged=True, prefix_slots=1, prefix_capacity=16)
        with pytest.raises(ValueError, match="at least one slot"):
            DecodeSession(m, 3, 64, 1.0, 0.98, 1, ragged=True, row_params=True, prefix_slots=1, prefix_capacity=0)
        with torch.inference_mode():
            flat = DecodeSession(m, 3, 64, 1.0, 0.98, 1, ragged=True, row_params=True)
            ses = DecodeSession(m, 3, 64, 1.0, 0.98, 1, ragged=True, row_params=True, prefix_slots=2, prefix_capacity=16)
            assert flat.kvs is None and flat.key != ses.key and ses.key[-1][-1] == ("slots", 2, 16)
            assert flat.key == DecodeSession.make_key(m, 3, 64, 1.0, 0.98, 1, ragged=True, row_params=True)
            ses.admit([0], toks, [4], [9], [1.0], [0.98], [1], masks, masks, slots=[1])
            del log[:]
            one = lambda s, **kw: s.admit([1], toks, [4], [9], [1.0], [0.98], [1], masks, masks, **kw)
            with pytest.raises(ValueError, match="with prefix slots only"):
                one(flat, slots=[0])
            for slots, match in (([2], "outside"), ([-1], "outside"), ([0, 1], "2 slots for 1"), ([1], "in use")):
                with pytest.raises(ValueError, match=match):
                    one(ses, slots=slots)
            with pytest.raises(ValueError, match="named twice"):
                ses.admit([1, 2], torch.cat([toks, toks]), [4, 4], [9, 9], [1.0] * 2, [0.98] * 2, [1, 1], masks.repeat(2, 1),
                          masks.repeat(2, 1), slots=[0, 0])
            with pytest.raises(ValueError, match="20 events into a prefix slot of 16"):
                ses.admit([1], torch.from_numpy(q), [20], [30], [1.0], [0.98], [1], masks, masks, slots=[0])
            with pytest.raises(ValueError, match="still name a prefix slot"):
                ses.admit([0], toks, [4], [9], [1.0], [0.98], [1], masks, masks)
            fork = lambda s, src, dst, **kw: s.fork([src], [dst], [4], [9], [1.0], [0.98], [1], masks, masks, **kw)
            with pytest.raises(ValueError, match="with prefix slots only"):
                fork(flat, 0, 1, join=[True])
            for src, dst, kw, match in ((0, 1, {}, "joins its slot"), (0, 1, dict(join=[False]), "joins its slot"),
                                        (1, 2, dict(join=[True]), "joins its slot"), (0, 1, dict(join=[True, True]), "2 values for 1")):
                with pytest.raises(ValueError, match=match):
                    fork(ses, src, dst, **kw)
            with pytest.raises(ValueError, match=r"rows of \[3\] events behind prompts of \[4\]"):
                ses.fork([0], [1], [3], [9], [1.0], [0.98], [1], masks, masks, join=[True])
            assert not log and ses.slot_refs == [0, 1] and ses.row_slot_host == [1, -1, -1]
