"""Shared by test_seeded_host.py and test_seeded_gpu.py: request X of the seeded decode pool in its surroundings, and the pool
against generate_ragged."""
import ragged_common as rc

X_KW = dict(temp=1.2, top_k=20, ban_eos=True)   # sampled, not greedy: X reads its noise at every position
CASES = ("one_step", "five_steps", "reused_row", "alone_row0")


def run_x(m, orc, tok, case, seed=77):
    """request X (17 prompt events, 24 to generate, X_KW, ``seed``) admitted ALONE into a 4-row seeded pool of capacity 128: into
    row 3 in the three surroundings of test_pool_host._run_x (other neighbours after 1 step, after 5 steps, a reused row), or into
    row 0 of an otherwise empty pool; -> (X's result, the session it ran on, that session's graphs before X was admitted)"""
    x = rc.prompts(orc, tok, (17,), seed0=300)[0]
    with m.decode_pool(4, 128, seeded=True) as pool:
        if case == "one_step":       # three other requests have run one step
            for i, p in enumerate(rc.prompts(orc, tok, (3, 9, 30), seed0=310)):
                pool.submit(p, max_len=len(p) + 40, top_k=20, temp=1.2, ban_eos=True, seed=1000 + i)
            before = 1
        elif case == "five_steps":   # three DIFFERENT requests have run five steps
            for i, p in enumerate(rc.prompts(orc, tok, (12, 2, 21), seed0=320)):
                pool.submit(p, max_len=len(p) + 33, top_k=5, temp=0.8, ban_eos=True, seed=(1 << 64) - 1 - i)
            before = 5
        elif case == "reused_row":   # row 3 first hosted a longer request, which finished
            for i, (p, n) in enumerate(zip(rc.prompts(orc, tok, (5, 8, 11, 40), seed0=330), (40, 40, 40, 3))):
                pool.submit(p, max_len=len(p) + n, top_k=20, ban_eos=True, seed=77 if i == 3 else 5 + i)
            before = 3
        else:
            before = 0
        for _ in range(before):
            pool.step()
        row = 3 if before else 0
        if before:
            assert sorted(pool.occupied) == [0, 1, 2] and pool.free == [3], case
        rid = pool.submit(x, max_len=17 + 24, seed=seed, **X_KW)
        pool.step()
        ses = pool.ses
        graphs = (ses.g_net, ses.g_steps, ses.g_noise)
        assert pool.occupied[row] == rid
        while not pool.requests[rid].done:
            pool.step()
        out = pool.result(rid)
        assert pool.ses is ses and (ses.g_net, ses.g_steps, ses.g_noise) == graphs
    assert out.shape == (41, 8) and (out[:17] == x).all()
    return out, ses, graphs


DIST_ROWS, DIST_IDS = 4096, (5, 40, 41, 77, 130, 131)                 # six candidates inside one 128-id span
DIST_P = (0.40, 0.25, 0.15, 0.10, 0.06, 0.04)


def distribution_case(V):
    """4096 rows sharing ONE logit row (fp32) whose first mask leaves the six ids DIST_IDS, their filtered probabilities DIST_P up
    to fp32 rounding; seeds 0..4095, ctr 0, temp 1, top_p 1, top_k 6.  -> dict of CPU tensors"""
    import torch
    row = torch.zeros(V)
    row[list(DIST_IDS)] = torch.tensor(DIST_P).log() + 3.0
    first = torch.zeros(V, dtype=torch.uint8)
    first[list(DIST_IDS)] = 1
    B = DIST_ROWS
    return dict(logits=row[None].repeat(B, 1), first=first, ban=torch.zeros(V, dtype=torch.uint8), span=(0, 192),
                seed=torch.arange(B, dtype=torch.int64), ctr=torch.zeros(B, dtype=torch.int32),
                temp=torch.ones(B), top_p=torch.ones(B), top_k=torch.full((B,), 6, dtype=torch.int32),
                tabs=torch.zeros((1, 8), dtype=torch.int32), ev=torch.zeros(B, dtype=torch.int64))


def chi_square(ids, V):
    """(statistic against the filtered probabilities of distribution_case, counts of the six ids); every id must be one of them"""
    import numpy as np
    import torch
    row = torch.zeros(V)
    row[list(DIST_IDS)] = torch.tensor(DIST_P).log() + 3.0
    p = torch.softmax(row, -1)[list(DIST_IDS)].double()
    p = (p / p.sum()).numpy()
    ids = np.asarray(ids)
    counts = np.array([(ids == i).sum() for i in DIST_IDS])
    assert counts.sum() == len(ids), "an id outside the six candidates"
    exp = p * len(ids)
    return float(((counts - exp) ** 2 / exp).sum()), counts


def chi_square_bound(df=5, tail=1e-9):
    """the 1 - tail quantile of chi-square(df): scipy.stats where it is installed, else Wilson-Hilferty"""
    try:
        from scipy.stats import chi2
        return float(chi2.ppf(1.0 - tail, df))
    except ImportError:
        from statistics import NormalDist
        z = NormalDist().inv_cdf(1.0 - tail)
        return df * (1.0 - 2.0 / (9 * df) + z * (2.0 / (9 * df)) ** 0.5) ** 3


def pool_together(m, prompts, n_gen, seeds, **kw):
    """a seeded pool of len(prompts) rows that admits the prompts together into rows 0..B-1; -> the results"""
    B = len(prompts)
    with m.decode_pool(B, max(len(p) + n for p, n in zip(prompts, n_gen)) + 1, seeded=True) as pool:
        ids = [pool.submit(p, max_len=len(p) + n, seed=s, **kw) for p, n, s in zip(prompts, n_gen, seeds)]
        pool.step()
        assert [pool.occupied[b] for b in range(B)] == ids
        while pool.pending():
            pool.step()
        return [pool.result(i) for i in ids]
