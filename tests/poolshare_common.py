"""Shared by test_poolshare_host.py and test_poolshare_gpu.py: the id-equality properties of a decode pool whose requests share a
prompt's K/V through prefix slots (submit(share_prefix=True), fork of a sharing parent).  Every function runs on the model it is given
(the CPU stand-ins or the production session), in seeded pools of ``rows`` rows, and asserts.  ``slots``: the pool's slot keywords
(prefix_slots, prefix_capacity); ``length``: the shared prompt's events."""
import numpy as np

import ragged_common as rc
from fork_common import KW, drain, same


def child_repeats_parent(m, orc, tok, rows, capacity, slots, length):
    """a sharing parent (seed 77) beside a neighbour that shares nothing is forked after 3 steps into two children that JOIN its slot:
    the one on seed 77 repeats the parent event for event, the one on seed 78 shares the first 3 events and then differs"""
    p, q = rc.prompts(orc, tok, (length, 9), seed0=600)
    with m.decode_pool(rows, capacity, seeded=True, **slots) as pool:
        par = pool.submit(p, max_len=length + 10, seed=77, share_prefix=True, **KW)
        pool.submit(q, max_len=9 + 8, seed=5, **KW)
        for _ in range(3):
            pool.step()
        ses = pool.ses
        assert ses.slot_refs[0] == 1 and ses.row_slot_host[:2] == [0, -1] and ses.slot_len_host[0] == length
        a, b = pool.fork(par, count=2, seed=[77, 78])
        assert ses.slot_refs[0] == 3 and ses.row_slot.tolist()[:4] == [0, -1, 0, 0] and ses.pos.tolist()[2:4] == [length + 3] * 2
        assert pool.requests[a].share and same(pool.result(a), pool.result(par))
        drain(pool)
        out = [pool.result(r) for r in (par, a, b)]
        assert ses.slot_refs[0] == 0 and ses.slot_len.tolist()[0] == 0 and ses.row_slot.tolist() == [-1] * rows
    at = length + 3
    assert out[0].shape == (length + 10, 8) and (out[0][:length] == p).all()
    assert same(out[1], out[0]), np.argwhere(out[1] != out[0])[:4]
    assert (out[2][:at] == out[0][:at]).all() and (out[2][at:] != out[0][at:]).any()
    return ses


def held_then_forked_equals_uninterrupted(m, orc, tok, rows, capacity, slots, length):
    """a sharing hold=True request (max_len length + 3, seed 9) finishes beside a longer neighbour and keeps its row AND its slot; two
    steps later fork(rid, max_len=length + 8, seed=9) == an uninterrupted sharing request with that max_len in the same surroundings"""
    x, q = rc.prompts(orc, tok, (length, 6), seed0=620)

    def surroundings(pool):
        pool.submit(q, max_len=6 + 14, seed=100, **KW)

    with m.decode_pool(rows, capacity, seeded=True, **slots) as pool:
        rid = pool.submit(x, max_len=length + 3, seed=9, hold=True, share_prefix=True, **KW)
        surroundings(pool)
        while not pool.requests[rid].done:
            pool.step()
        ses = pool.ses
        assert pool.held() == [rid] and ses.slot_refs[0] == 1, "a held row keeps its slot"
        for _ in range(2):
            pool.step()
        assert ses.slot_len.tolist()[0] == length and ses.row_slot.tolist()[0] == 0
        short = pool.result(rid)
        child, = pool.fork(rid, max_len=length + 8, seed=9)
        assert ses.slot_refs[0] == 2
        drain(pool)
        got = pool.result(child)
        assert ses.slot_refs[0] == 1 and pool.held() == [rid]
        pool.drop(rid)
        assert ses.slot_refs[0] == 0 and ses.slot_len.tolist()[0] == 0
    with m.decode_pool(rows, capacity, seeded=True, **slots) as pool:
        rid = pool.submit(x, max_len=length + 8, seed=9, share_prefix=True, **KW)
        surroundings(pool)
        drain(pool)
        want = pool.result(rid)
        assert pool.ses is ses
    assert short.shape == (length + 3, 8) and (want[:length + 3] == short).all()
    assert same(got, want), np.argwhere(got != want)[:4]
    return ses


def ids_do_not_depend_on_the_group(m, orc, tok, rows, capacity, slots, length):
    """a sharing request on seed 31 gives the same ids as the leader of a group of n = 2 and of n = 5, and whether or not another slot
    is in use (another sharing group, admitted one step earlier: the request then sits in other rows and in slot 1).  Its siblings
    differ from it (other seeds)."""
    p, q = rc.prompts(orc, tok, (length, 7), seed0=640)
    assert rows >= 7 and slots["prefix_slots"] >= 2

    def run(n, other_first):
        with m.decode_pool(rows, capacity, seeded=True, **slots) as pool:
            if other_first:
                pool.submit(q, max_len=7 + 12, seed=[500, 501], n=2, share_prefix=True, **KW)
                pool.step()
            ids = pool.submit(p, max_len=length + 8, seed=[31] + [900 + i for i in range(n - 1)], n=n, share_prefix=True, **KW)
            pool.step()
            ses = pool.ses
            g = 1 if other_first else 0
            assert ses.slot_refs[g] == n and ses.slot_len.tolist()[g] == length
            assert [ses.row_slot_host[pool.requests[i].row] for i in ids] == [g] * n
            drain(pool)
            return [pool.result(i) for i in ids], ses

    two, ses = run(2, False)
    five, ses5 = run(5, False)
    beside, ses_b = run(2, True)
    assert ses5 is ses and ses_b is ses, "one pooled session"
    assert two[0].shape == (length + 8, 8)
    assert same(two[0], five[0]), np.argwhere(two[0] != five[0])[:4]
    assert same(two[0], beside[0]), np.argwhere(two[0] != beside[0])[:4]
    assert same(two[1], five[1]) and same(two[1], beside[1])
    assert not same(two[0], two[1]) and not same(five[3], five[4])
    return ses


def rows_that_share_nothing(m, orc, tok, rows, capacity, slots, lengths):
    """requests that share nothing give the same ids in a pool WITH slots (next to a sharing group) as in a pool without, at equal rows
    and equal admission groups.  -> (the slots session, the plain session)"""
    ps = rc.prompts(orc, tok, lengths, seed0=660)
    s = rc.prompts(orc, tok, (6,), seed0=670)[0]

    def run(kw, share):
        with m.decode_pool(rows, capacity, seeded=True, **kw) as pool:
            ids = [pool.submit(x, max_len=len(x) + 6 + i, seed=40 + i, **KW) for i, x in enumerate(ps)]
            pool.step()
            if share:  # (admitted one step later, by a forward of its own: the others' launches keep their shapes)
                pool.submit(s, max_len=6 + 5, seed=[1, 2], n=2, share_prefix=True, **KW)
            drain(pool)
            return [pool.result(i) for i in ids], pool.ses

    plain, ses0 = run({}, False)
    quiet, ses1 = run(slots, False)
    busy, ses2 = run(slots, True)
    assert ses1 is ses2 and ses1 is not ses0 and ses0.kvs is None and ses1.kvs is not None
    for a, b, c in zip(plain, quiet, busy):
        assert same(a, b), np.argwhere(a != b)[:4]
        assert same(a, c), np.argwhere(a != c)[:4]
    return ses1, ses0
