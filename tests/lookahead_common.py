"""Shared by test_lookahead_host.py and test_lookahead_pool_gpu.py: the promise of a lookahead pool -- a request's ids and
log-likelihoods do not depend on what the drafts were -- on the model it is given (the CPU stand-ins or the production session).

Every run submits its requests in WAVES that are admitted whole in one step and drained before the next, so that a request's admission
group (the packed prefill's launch shape, the seeded pool's stated limit) is the same whatever the drafts did to the step count."""
import math

import numpy as np

import fork_common as fc
import ragged_common as rc

KW = dict(temp=1.2, top_k=20)   # sampled, EOS allowed: a request may end before its max_len


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _none(history, k):
    return np.zeros((0, 8), dtype=np.int64)


def oracle_of(recorded, V, wrong_from=None):
    """a proposer that returns the recorded continuation of the request whose recorded result ``history`` is a prefix of (the first
    such one: siblings on one prompt are told apart only once they differ); ``wrong_from`` = j: guesses j, j + 1, ... are spoiled
    in token 1 (a valid id that is not the recorded one)"""
    def propose(history, k):
        n = len(history)
        for rec in recorded:
            if len(rec) > n and (rec[:n] == history).all():
                d = rec[n:n + k].copy()
                if wrong_from is not None:
                    d[wrong_from:, 1] = (d[wrong_from:, 1] + 1) % V
                return d
        return np.zeros((0, 8), dtype=np.int64)
    return propose


def steps_of(events: int, k: int) -> int:
    """step() calls an admitted request takes for ``events`` generated events when every guess is right: the admitting step samples
    one event (nothing was drafted before the prefill), every later step k + 1"""
    return 1 + math.ceil((events - 1) / (k + 1)) if events > 0 else 0


def waves(m, orc, tok, capacity, rows, k, proposer, eos_seed, uninterrupted=False):
    """-> (results, logprobs, steps per wave, ids): wave 1 = three (rows == 2: two) requests on prompts of 5, 20 and 9 events -- one
    that runs to its max_len, one whose seed ``eos_seed`` ends it on EOS, and (rows >= 3) one with hold=True, max_len 9 + 6, that is
    forked afterwards with max_len 9 + 17 (``uninterrupted``: the same request with max_len 9 + 17 and no hold in its place);
    wave 2 = an n=2 sibling submit on a prompt of 12 events"""
    pa, pb, pc, pd = rc.prompts(orc, tok, (5, 20, 9, 12), seed0=900)
    res, lps, steps, ids = [], [], [], {}
    with m.decode_pool(rows, capacity, seeded=True, lookahead=k, logprobs=True) as pool:
        if proposer is not None:
            pool.proposer = proposer

        def drain():
            s0 = pool.steps
            fc.drain(pool)
            steps.append(pool.steps - s0)

        ids["a"] = pool.submit(pa, max_len=5 + 19, seed=17, ban_eos=True, **KW)
        ids["b"] = pool.submit(pb, max_len=40, seed=eos_seed, **KW)
        if rows >= 3:
            if uninterrupted:
                ids["c"] = pool.submit(pc, max_len=9 + 17, seed=13, ban_eos=True, **KW)
            else:
                ids["c"] = pool.submit(pc, max_len=9 + 6, seed=13, ban_eos=True, hold=True, **KW)
        drain()
        if rows >= 3 and not uninterrupted:
            assert pool.held() == [ids["c"]] and len(pool.result(ids["c"])) == 15
            ids["child"], = pool.fork(ids["c"], max_len=9 + 17, seed=13)
            drain()
            pool.drop(ids["c"])
        ids["s0"], ids["s1"] = pool.submit(pd, max_len=12 + 10, seed=[21, 22], n=2, ban_eos=True, **KW)
        drain()
        assert pool.free == list(range(rows)) and not pool.held()
        for name, rid in ids.items():
            res.append(pool.result(rid))
            lps.append(pool.logprobs(rid))
        assert pool.ses.lookahead == k and pool.ses.B == rows * (k + 1) and pool.ses.kv1.B == rows
    return res, lps, steps, ids


def drafts_do_not_matter(m, orc, tok, capacity, rows, k, eos_seed=None):
    """five runs of ``waves`` -- no drafts (recorded), the recorded continuation, wrong events, right for two events then wrong, the
    built-in proposer: results and logprobs() bit-equal; the oracle run's step counts are exactly ``steps_of`` its longest request"""
    V = tok.vocab_size
    eos_seed = EOS_SEED if eos_seed is None else eos_seed
    rec, rec_lp, steps0, ids = waves(m, orc, tok, capacity, rows, k, _none, eos_seed)
    names = list(ids)
    gen = {n: len(r) - {"a": 5, "b": 20, "c": 9, "child": 15, "s0": 12, "s1": 12}[n] for n, r in zip(names, rec)}
    by = dict(zip(names, rec))
    # the cases the set must hold
    assert by["a"].shape == (24, 8) and (gen["a"] - 1) % (k + 1) >= 2, "a reaches max_len in the middle of a run of k + 1"
    assert len(by["b"]) < 40 and by["b"][-1, 0] == tok.eos_id and gen["b"] >= 3, \
        f"request b (seed {eos_seed}) is to end on EOS before max_len 40: {len(by['b'])} events, last id {by['b'][-1, 0]}"
    assert by["s0"].shape == by["s1"].shape == (22, 8) and not fc.same(by["s0"], by["s1"])
    assert all(len(lp) == gen[n] and lp.dtype == np.float32 and (lp < 0).all() for n, lp in zip(names, rec_lp))
    # without drafts every step yields one event per request
    assert steps0[0] == max(gen[n] for n in ("a", "b", "c") if n in gen)
    runs = {"oracle": oracle_of(rec, V), "wrong": oracle_of(rec, V, wrong_from=0), "two right": oracle_of(rec, V, wrong_from=2),
            "built-in": None}
    for what, proposer in runs.items():
        got, got_lp, steps, _ = waves(m, orc, tok, capacity, rows, k, proposer, eos_seed)
        for n, a, b, la, lb in zip(names, rec, got, rec_lp, got_lp):
            assert same_bits(a, b), (what, n, a.shape, b.shape, np.argwhere(a != b)[:4] if a.shape == b.shape else None)
            assert same_bits(la, lb), (what, n, la, lb)
        if what == "oracle":   # wave 1: different prompts, every guess right; its longest request sets the count
            assert steps[0] == max(steps_of(gen[n], k) for n in ("a", "b", "c") if n in gen), (steps, gen)
            if "child" in gen:
                assert steps[1] == steps_of(gen["child"], k), (steps, gen)
            assert steps[-1] <= steps0[-1]
        if what == "wrong":
            assert steps == steps0, "a wrong guess costs no step"
        if what == "two right":   # a step yields 3 events (2 right guesses), the admitting step 1
            assert steps[0] == max(1 + math.ceil((gen[n] - 1) / min(3, k + 1)) for n in ("a", "b", "c") if n in gen), (steps, gen)
    return gen


def held_then_forked_equals_uninterrupted(m, orc, tok, capacity, rows, k, eos_seed=None):
    """request c (hold=True, max_len 15), forked afterwards on its own seed with max_len 26, equals the uninterrupted request with
    max_len 26 in the same pool shape and admission group -- without drafts, and with every guess right"""
    V = tok.vocab_size
    eos_seed = EOS_SEED if eos_seed is None else eos_seed
    want, want_lp, _, wid = waves(m, orc, tok, capacity, rows, k, _none, eos_seed, uninterrupted=True)
    u, u_lp = want[list(wid).index("c")], want_lp[list(wid).index("c")]
    assert u.shape == (26, 8)
    for proposer in (_none, oracle_of(want, V)):
        got, got_lp, _, ids = waves(m, orc, tok, capacity, rows, k, proposer, eos_seed)
        names = list(ids)
        short, child = got[names.index("c")], got[names.index("child")]
        assert short.shape == (15, 8) and same_bits(short, u[:15]) and same_bits(child, u), np.argwhere(child != u)[:4]
        lp = np.concatenate([got_lp[names.index("c")], got_lp[names.index("child")]])
        assert same_bits(lp, u_lp), (lp, u_lp)


# request b's seed, found on the CPU emulation: of the seeds 0..59, tried in turn in a lookahead pool without drafts (the tiny model of
# either test file, fp32 stand-ins), 11 is the first that ends request b on EOS after more than 10 events -- 11 of them, on both
# models: with k = 3 the EOS is then the second event of the last run of k + 1 (1 + 4 + 4 + 2); the bf16 production session ends it on
# EOS after 14 (1 + 4 + 4 + 4 + 1).  ``drafts_do_not_matter`` asserts that
# request b ends on EOS before its max_len, so a change of the sampler that moves it shows as that assertion, not as a weaker test.
EOS_SEED = 11
