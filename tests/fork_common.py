"""Shared by test_fork_host.py and test_fork_gpu.py: the four id-equality properties of DecodePool.fork / submit(n=) / submit(hold=) on a
pool of 4 rows.  Every function runs on the model it is given (the CPU stand-ins or the production session) and asserts."""
import numpy as np
import torch

import ragged_common as rc

ROWS = 4
KW = dict(temp=1.2, top_k=20, ban_eos=True)   # sampled, not greedy: a seeded request reads its variates at every position


def drain(pool):
    while pool.pending():
        pool.step()


def same(a, b):
    return a.shape == b.shape and bool((a == b).all())


def child_repeats_parent(m, orc, tok, capacity):
    """a parent (7 events, seed 77) beside a neighbour is forked after 3 steps into two children: the one on seed 77 and the parent's
    settings repeats the parent event for event, the one on seed 78 shares the prefix and then differs"""
    p, q = rc.prompts(orc, tok, (7, 9), seed0=500)
    with m.decode_pool(ROWS, capacity, seeded=True) as pool:
        par = pool.submit(p, max_len=30, seed=77, **KW)
        pool.submit(q, max_len=25, seed=5, **KW)
        for _ in range(3):
            pool.step()
        at = len(pool.result(par))
        assert at == 7 + 3
        a, b = pool.fork(par, count=2, seed=[77, 78])
        assert pool.occupied == {0: par, 1: par + 1, 2: a, 3: b} and same(pool.result(a), pool.result(par))
        first = {rid: ev for rid, ev, _ in pool.step()}
        assert set(first) == {par, par + 1, a, b}, "a child's first event is reported by the next step"
        drain(pool)
        out = [pool.result(r) for r in (par, a, b)]
        ses = pool.ses
    assert out[0].shape == (30, 8) and (out[0][:7] == p).all()
    assert same(out[1], out[0]), np.argwhere(out[1] != out[0])[:4]
    assert (out[1][at] == first[a]).all()
    assert out[2].shape == (30, 8) and (out[2][:at] == out[0][:at]).all() and (out[2][at:] != out[0][at:]).any()
    return ses


def siblings_equal_lone_requests(m, orc, tok, capacity):
    """submit(n=3, seed=[a, b, c]) == three lone submit(seed=...) calls, each in a fresh pool of the same size"""
    p = rc.prompts(orc, tok, (8,), seed0=510)[0]
    seeds = (11, (1 << 64) - 1, 1 << 40)
    with m.decode_pool(ROWS, capacity, seeded=True) as pool:
        ids = pool.submit(p, max_len=24, seed=list(seeds), n=3, **KW)
        assert isinstance(ids, list) and len(ids) == 3 and pool.pending() == 3
        pool.step()
        assert pool.occupied == {0: ids[0], 1: ids[1], 2: ids[2]}
        drain(pool)
        together = [pool.result(i) for i in ids]
        ses = pool.ses
    for s, got in zip(seeds, together):
        with m.decode_pool(ROWS, capacity, seeded=True) as pool:
            rid = pool.submit(p, max_len=24, seed=s, **KW)
            assert isinstance(rid, int)
            drain(pool)
            lone = pool.result(rid)
            assert pool.ses is ses
        assert lone.shape == (24, 8) and same(got, lone), (s, np.argwhere(got != lone)[:4])
    assert not same(together[0], together[1]) and not same(together[1], together[2])
    return ses


def held_then_forked_equals_uninterrupted(m, orc, tok, capacity, length, alone):
    """a hold=True request (``length`` prompt events, max_len 6, seed 9) finishes and keeps its row; ``alone``: it was the only one
    running (the forced net step), else it ran beside two longer requests and five more steps pass.  fork(rid, max_len=12,
    seed=9) == an uninterrupted request with max_len 12 in the same surroundings"""
    x = rc.prompts(orc, tok, (length,), seed0=520)[0]
    others = [] if alone else rc.prompts(orc, tok, (6, 9), seed0=530)

    def surroundings(pool):
        for i, q in enumerate(others):
            pool.submit(q, max_len=len(q) + 20, seed=100 + i, **KW)

    with m.decode_pool(ROWS, capacity, seeded=True) as pool:
        rid = pool.submit(x, max_len=6, seed=9, hold=True, **KW)
        surroundings(pool)
        steps = 0
        while not pool.requests[rid].done:
            pool.step()
            steps += 1
        assert steps == 6 - length and pool.held() == [rid] and pool.pending() == len(others) and pool.requests[rid].row == 0
        assert 0 not in pool.free and 0 not in pool.occupied
        if alone:
            assert pool.step() == []   # nothing runs: nothing is launched, the row stays held
        else:
            for _ in range(5):
                pool.step()
            assert pool.pending() == 2, "the other requests are long enough"
        short = pool.result(rid)
        child, = pool.fork(rid, max_len=12, seed=9)
        assert pool.held() == [rid] and pool.requests[child].row == (1 if alone else 3), "the lowest free row"
        drain(pool)
        got = pool.result(child)
        assert pool.held() == [rid]
        pool.drop(rid)
        assert pool.held() == [] and 0 in pool.free and same(pool.result(rid), short)
        ses = pool.ses
    with m.decode_pool(ROWS, capacity, seeded=True) as pool:
        rid = pool.submit(x, max_len=12, seed=9, **KW)
        surroundings(pool)
        drain(pool)
        want = pool.result(rid)
    assert short.shape == (6, 8) and want.shape == (12, 8) and (want[:6] == short).all()
    assert same(got, want), np.argwhere(got != want)[:4]
    return ses


def greedy_child_in_an_unseeded_pool(m, orc, tok, capacity):
    """unseeded pool: a greedy (top_k=1) child, forked after 3 steps with the parent's settings, equals its greedy parent"""
    p, q = rc.prompts(orc, tok, (5, 9), seed0=540)
    with m.decode_pool(ROWS, capacity, generator=torch.Generator(device=m.device).manual_seed(3)) as pool:
        par = pool.submit(p, max_len=28, top_k=1, ban_eos=True)
        pool.submit(q, max_len=20, temp=1.1, top_k=20, ban_eos=True)
        for _ in range(3):
            pool.step()
        child, = pool.fork(par)
        drain(pool)
        a, b = pool.result(par), pool.result(child)
        ses = pool.ses
    assert a.shape == (28, 8) and same(a, b), np.argwhere(a != b)[:4]
    return ses
