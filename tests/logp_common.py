"""Shared by test_logp_host.py and test_logp_pool_gpu.py: the oracle's teacher-forced log-likelihoods of a request's result, and the
scenario both run against them.  Test infrastructure only."""
import numpy as np
import torch

import ragged_common as rc
import ref_logp

KW = dict(temp=1.2, top_k=20)   # sampled, not greedy; EOS allowed


def oracle_token_logp(orc, sd, shp, row, first):
    """teacher-forced oracle (one uncached pass, float64 log-softmax of its fp32 logits) over ONE result ``row`` (L, 8): -> float64
    [L - first, 8], entry [j, i] = logp of token i of event first + j given everything before it"""
    ids = torch.from_numpy(np.ascontiguousarray(row))[None]
    _, L, T = ids.shape
    with torch.inference_mode():
        hidden = orc.midi_forward(sd, shp, ids[:, :-1])[:, first - 1:]   # hidden i predicts event i + 1
        n = hidden.shape[1]
        tgt = ids[:, first:].reshape(n, T)
        logits = orc.midi_forward_token(sd, shp, hidden.reshape(n, -1), tgt[:, :-1])
    return ref_logp.logp64(logits, tgt).numpy()


def oracle_ll(orc, tok, sd, shp, row, first, arity):
    """-> (ll float64 [L - first], tokens counted int [L - first]) of events first.. of ``row``"""
    lp = oracle_token_logp(orc, sd, shp, row, first)
    n = [1 if int(e[0]) == tok.eos_id else 1 + int(arity[int(e[0])]) for e in row[first:]]
    return np.array([lp[j, :k].sum() for j, k in enumerate(n)]), np.array(n)


def pool_against_oracle(m, orc, tok, sd, shp, per_token, rel=0.0, rows=4, capacity=64, **pool_kw):
    """five requests of different lengths and settings (the fifth admitted later, into a reused row) in a pool with logprobs=True:
    every request's logprobs() against the oracle's ll of its result, |difference| <= sum over the event's tokens of (per_token + rel
    x |the oracle's value for the token|); -> the worst difference as a fraction of that tolerance"""
    arity = m._grammar()[3]
    ps = rc.prompts(orc, tok, (5, 3, 6, 4, 2), seed0=700)
    seeded = pool_kw.get("seeded", False)
    with m.decode_pool(rows, capacity, logprobs=True, **pool_kw) as pool:
        ids = []
        for k, p in enumerate(ps):
            kw = dict(KW, seed=900 + k) if seeded else dict(KW)
            if k == 1:
                kw.update(temp=0.8, top_k=5, top_p=0.9)
            ids.append(pool.submit(p, max_len=len(p) + 4 + 2 * k, **kw))
        while pool.pending():
            pool.step()
        worst = 0.0
        for rid, p in zip(ids, ps):
            res, lp = pool.result(rid), pool.logprobs(rid)
            assert lp.dtype == np.float32 and lp.shape == (len(res) - len(p),) and len(lp) > 0
            want, n = oracle_ll(orc, tok, sd, shp, res, len(p), arity)
            d = oracle_token_logp(orc, sd, shp, res, len(p))
            tol = np.array([(per_token + rel * np.abs(d[j, :k])).sum() for j, k in enumerate(n)])
            frac = np.abs(lp.astype(np.float64) - want) / tol
            worst = max(worst, float(frac.max()))
            assert (frac <= 1).all(), (rid, frac.max(), per_token, rel)
    return worst
