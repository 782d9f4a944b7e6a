"""Test-only references, input generators and checks for the index-driven kernels (csrc/elementwise.hip, augment.hip, the
transpose of gemm.hip): mh_embed_sum_fwd, mh_concat_tok_fwd, mh_embed_scatter_bwd, mh_embed_segment_bwd, mh_embed_segment_sum,
mh_embed_split_hi_lo, mh_embed_table_norm_bwd, mh_token_segments, mh_transpose, mh_collate_windows, mh_augment_piece_stats,
mh_augment_collate_windows.  Everything is plain vectorised torch (gather, index_add_, sort, cumsum) on whatever device the
backend names, in float64 or int64; nothing here calls tests/emu_ops.py.

Every check takes a *backend* (tests/test_index_kernels_gpu.py: `Hip`, the C ABI on the device; tests/test_index_bounds_host.py:
`Emu`, emu_ops, and named wrong kernels) and returns the number of bad elements (0 = pass); structural failures raise.

Two families of values.

EXACT.  Tables, gradients and rows are integers of magnitude <= 8.  No case sums more than 2^17 of them per element, so every
partial sum is an integer below 2^24 (exact in fp32) in any order, with or without atomics; embed_sum's bf16 output is at most
16 x 8 = 128 <= 2^8 (exact in bf16).  The result must therefore have THE SAME BITS as the int64 reference.  Accumulating
kernels start from a table of integers, not zeros ("adds to", not "writes"), and run twice.  A kernel that rounds to bf16
after every add passes this family (every partial sum is representable); the random family is there for it.

RANDOM against float64, u = 2^-24, E_T = ref_streamers.E (2^-8 bf16, 2^-24 fp32), TINY = ref_streamers.TINY:
  embed_sum_fwd     |got - ref64| <= (E_T + (TT - 1) u) sum_j |table[id_j]| + TINY: an fp32 sum of TT terms in some order
                    ((TT - 1) u sum|terms| to first order) and one rounding to the output type (E_T |sum| <= E_T sum|terms|).
  scatter / segment_bwd / segment_sum
                    |got - ref64| <= n 2^-23 sum|terms| per table element, n = the number of terms the element received (its
                    prior value counts as one): an fp32 sum of n terms in any order is within (n - 1) u sum|terms| (1 + O(n u));
                    2^-23 = 2 u leaves the second order its room (the bound test_tokfirst_kernels_gpu.py uses).  An element that
                    receives nothing must keep its bits.
  table_norm_bwd    the bound derived in test_tokfirst_kernels_gpu.py::test_table_norm_backward_against_fp64: T = t_hi + t_lo one
                    rounding, the row dot D products and D additions, cf = r r dot / D three more, e cf, T - e cf and acc + (.)
                    one each: |err| <= 3 u (|acc| + |T| + |e cf|) + |e| (r^2 / D) (D + 6) u sum|T_k e_k|, asserted at twice
                    that for the second-order terms.
  split_hi_lo       hi == rnd_T(s) bit for bit; |hi + lo - s| <= E_T^2 |s| (s - hi is exact in fp32 and at most E_T |s|; lo is
                    its rounding).
None of these was tuned on a device; tests/test_index_bounds_host.py holds the float64 reference rounded once, and emu_ops, to
them on the CPU.

Hygiene of every check: the output is a view inside a larger buffer of a fence value and everything outside the view -- in
front, behind, and the gap columns of a strided output -- must keep its bits (`stray`); input the operation must not read is
NaN (floating point) or an id that shows (integers); a NaN in an output fails; table rows that receive nothing keep their bits.

The integer kernels (token_segments, transpose, collate, augment) are exact by nature.  The augment checks come with a BRANCH
CENSUS (`augment_census`), a condition on the inputs alone: the constructed corpus must reach every rare rule branch, or the
test fails before it compares anything."""
import collections
import os
import re

import numpy as np
import torch

from ref_streamers import BF16, E, F32, F64, TINY, bad

U24, U23 = 2.0 ** -24, 2.0 ** -23
I16, I32, I64 = torch.int16, torch.int32, torch.int64
NVEC = {BF16: 8, F32: 4}
FENCE = 64                      # elements of fence in front of and behind every output view (a multiple of 16 bytes)
FENCE_F, FENCE_I = -12352.0, -30607   # (the float is a bf16 value)

_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "midi-model_amd", "csrc", "elementwise.hip")


def source_constant(name):
    """`constexpr int NAME = value;` of csrc/elementwise.hip"""
    m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, open(_SRC).read())
    assert m, name
    return int(m.group(1))


def grid_cap(entry):
    """the block cap of `grid_for(..., cap)` in the launcher of mh_<entry>"""
    src = open(_SRC).read()
    body = src[src.index('extern "C" int mh_%s(' % entry):]
    m = re.search(r"grid_for\([^;]*?,\s*(\d+)\s*,\s*(\d+)\)", body[: body.index("MH_LAUNCH_CHECK")])
    assert m, entry
    return int(m.group(1)), int(m.group(2))      # (items per block, cap)


SEG_OWN = source_constant("SEG_OWN")
SEG_CH = source_constant("SEG_CH")


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(shape, dtype, g, lim=8):
    return torch.randint(-lim, lim + 1, shape, generator=g).to(dtype)


def values(shape, dtype, g, exact):
    return ints(shape, dtype, g) if exact else torch.randn(shape, generator=g).to(dtype)


def bits(t):
    return t.view({2: I16, 4: I32, 8: I64}[t.element_size()]) if t.is_floating_point() else t


def fenced(shape, dtype, dev, ld=None, off=0):
    """-> (buf, view): `view` of `shape` (2-D with row stride `ld` when given) inside the flat fence-filled `buf`, FENCE + off
    elements from its start"""
    fill = FENCE_F if dtype.is_floating_point else FENCE_I
    if ld is None:
        n = int(np.prod(shape))
        buf = torch.full((2 * FENCE + off + n,), fill, dtype=dtype, device=dev)
        return buf, buf[FENCE + off: FENCE + off + n].view(shape)
    rows, cols = shape
    assert ld >= cols
    buf = torch.full((2 * FENCE + off + rows * ld,), fill, dtype=dtype, device=dev)
    return buf, buf[FENCE + off: FENCE + off + rows * ld].view(rows, ld)[:, :cols]


def stray(buf, buf0, view):
    """elements of `buf` outside `view` whose bits changed"""
    m = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    torch.as_strided(m, view.shape, view.stride(), view.storage_offset()).fill_(False)
    return int(((bits(buf) != bits(buf0)) & m).sum())


def inexact(got, ref64):
    """elements whose bits differ from the integer reference's"""
    return int((bits(got) != bits(ref64.to(got.dtype))).sum())


# ------------------------------------------------------------------------------------------------------------ embed_sum / concat
EMBED_D = {BF16: (8, 504, 512, 520, 1024), F32: (8, 248, 256, 264, 512)}
EMBED_SUM_CASES = [(M, TT, D, dt) for dt in (BF16, F32) for D in EMBED_D[dt] for M, TT in ((1, 1), (5, 7), (5, 8), (1, 9), (5, 16))]
EMBED_SUM_CAP = (4 * grid_cap("embed_sum_fwd")[1] + 5, 2, 8)        # one wave per row, 4 rows per block: the second pass of 5 rows


def unused_rows(tok, V):
    """table rows no id names: they hold NaN"""
    return torch.bincount(tok.reshape(-1), minlength=V) == 0


def embed_sum_inputs(M, TT, D, dtype, exact, V=37, seed=0):
    g = gen(1000 + seed)
    table = values((V, D), dtype, g, exact)
    tok = torch.randint(0, V, (M, TT), generator=g)
    tok.view(-1)[0], tok.view(-1)[-1] = 0, V - 1
    if M * TT > 2:
        tok.view(-1)[1] = V - 1
    table[unused_rows(tok, V)] = float("nan")
    return table, tok


def check_embed_sum(be, M, TT, D, dtype, exact, seed=0):
    table, tok = (t.to(be.dev) for t in embed_sum_inputs(M, TT, D, dtype, exact, seed=seed))
    buf, out = fenced((M, D), dtype, be.dev)
    buf0 = buf.clone()
    be.embed_sum(tok, table, out)
    rows = table[tok].to(F64)
    ref = rows.sum(1)
    if exact:
        n = inexact(out, ref)
    else:
        n = bad(out, ref, (E[dtype] + (TT - 1) * U24) * rows.abs().sum(1) + TINY)
    return n + stray(buf, buf0, out)


CONCAT_CASES = [(M, T, D, dt) for dt in (BF16, F32) for D in EMBED_D[dt] for M, T in ((1, 1), (5, 2), (5, 8))]
CONCAT_CAP = ((4 * grid_cap("concat_tok_fwd")[1]) // 2 + 3, 2, 8)
TOK_SENTINEL = 1 << 40     # what unused id columns hold: no kernel may read it


def check_concat(be, M, T, D, dtype, seed=0, V=37):
    g = gen(2000 + seed)
    table, hidden = ints((V, D), dtype, g).to(be.dev), ints((M, D), dtype, g).to(be.dev)
    wide = torch.full((M, T + 2), TOK_SENTINEL, dtype=I64)
    wide[:, : T - 1] = torch.randint(0, V, (M, T - 1), generator=g)
    if T > 1:
        wide[0, 0], wide[-1, T - 2] = 0, V - 1
    table[unused_rows(wide[:, : T - 1], V).to(be.dev)] = float("nan")
    tok = wide.to(be.dev)[:, : T - 1]                     # a column slice: ldtok = T + 2 > T - 1
    buf, out = fenced((M, T, D), dtype, be.dev)
    buf0 = buf.clone()
    be.concat(hidden, tok, table, out, T)
    ref = torch.cat([hidden[:, None], table[tok]], 1).to(F64)
    return inexact(out, ref) + stray(buf, buf0, out)


# ---------------------------------------------------------------------------------------------------------------------- scatter
SCATTER_CAP_ITEMS = 4 * grid_cap("embed_scatter_bwd")[1]
# (M, T, D, dtype, seq, pad, one_id): seq = the (T + 1, 1, 1) addressing of the token-sequence embedding, else (1, 0, 0)
SCATTER_CASES = [(M, T, D, dt, seq, pad, one)
                 for dt in (BF16, F32)
                 for (M, T, D, seq, pad, one) in ((5, 8, 8, False, 0, False), (5, 7, 520 if dt == BF16 else 264, True, 11, False),
                                                  (33, 8, 504 if dt == BF16 else 248, False, -1, False), (40, 7, 8, True, 0, True),
                                                  (40, 8, 512 if dt == BF16 else 256, False, 11, True))]
SCATTER_CAP = (SCATTER_CAP_ITEMS // 8 + 3, 8, 8, BF16, False, 11, False)


def check_scatter(be, M, T, D, dtype, seq, pad, one_id, exact, seed=0, V=29):
    g = gen(3000 + seed)
    spare = V - 2                                       # the id of the unused columns of the id matrix: its row must not move
    wide = torch.full((M, T + 2), spare, dtype=I64)
    ids = torch.randint(0, V - 2, (M, T), generator=g)
    if one_id:
        ids[:] = 5
    ids.view(-1)[0], ids.view(-1)[-1] = 0, V - 1
    if pad >= 0:
        ids.view(-1)[1: 4] = pad
    wide[:, :T] = ids
    tok = wide.to(be.dev)[:, :T]
    rpm, js, j0 = (T + 1, 1, 1) if seq else (1, 0, 0)
    dout = values((M * rpm, D), dtype, g, exact)
    if seq:
        dout.view(M, rpm, D)[:, 0] = float("nan")       # the hidden state's rows: not an embedding gradient
    dout = dout.to(be.dev)
    rows = (torch.arange(M)[:, None] * rpm + torch.arange(T)[None, :] * js + j0).to(be.dev)
    buf, dtab = fenced((V, D), F32, be.dev)
    dtab.copy_(values((V, D), F32, g, exact))
    prior = dtab.clone().to(F64)
    buf0 = buf.clone()
    be.scatter(tok, T, dout, rpm, js, j0, dtab, pad)
    keep = (tok != pad).reshape(-1)
    idk, terms = tok.reshape(-1)[keep], dout[rows.reshape(-1)[keep]].to(F64)
    ref = prior.clone().index_add_(0, idk, terms)
    mag = prior.abs().index_add_(0, idk, terms.abs())
    cnt = torch.bincount(idk, minlength=V).to(F64)[:, None]
    return _accumulated(dtab, ref, mag, cnt, prior, exact) + stray(buf, buf0, dtab)


def _accumulated(got, ref, mag, cnt, prior, exact):
    """an fp32 table after an accumulation: same bits as the integer reference, or the summation bound; rows that received
    nothing keep their bits either way"""
    if exact:
        return inexact(got, ref)
    n = bad(got, ref, (cnt + 1) * U23 * mag)
    idle = (cnt[:, 0] == 0)
    return n + inexact(got[idle], prior[idle])


# --------------------------------------------------------------------------------------------------------- segment_bwd / _sum
def seg_distributions(V):
    """name -> (list of (id, occurrences) ascending in id, occurrences of ids outside [0, V) behind seg_start[V], pad id)"""
    W = 8 * 128                                         # occurrences of an 8-wave workgroup
    d = {
        "own": ([(1, 5), (3, SEG_OWN - 1), (4, SEG_OWN), (5, SEG_OWN + 1), (9, 3)], 0, 0),
        "straddle": ([(1, 120), (2, 20), (3, 870), (4, 30), (V - 1, 10)], 0, 0),       # id 2 over the cut at 128, id 4 over 1024
        # id 2: [340, 2988), the whole second workgroup of 8 waves; id 3 follows inside the third: two groups meet in one LDS
        "long": ([(0, 40), (1, 300), (2, 2 * W + 600), (3, SEG_OWN + 76), (4, 200), (V - 1, 1)], 0, 0),
        "sparse": ([(1, 70), (V - 1, 90)], 0, 0),
        "outside": ([(0, 7), (2, 130), (7, 1), (V - 2, 60), (V - 1, 33)], 300, 0),
        "longpad": ([(3, 50), (6, SEG_OWN + 500), (7, 2), (V - 1, 4)], 5, 6),
        "oneid": ([(V // 2, 777)], 0, 0),
    }
    for n in (1, 127, 128, 129, 1023, 1024, 1025):
        segs, left, v = [], n, 0
        while left:
            c = min(left, 1 + (7 * v + n) % 41)
            segs.append((v * 3 if v else 0, c))
            left -= c
            v += 1
        segs[-1] = (V - 1, segs[-1][1])
        d["n%d" % n] = (segs, 0, 0)
    return d


SEG_DISTS = sorted(seg_distributions(4095))
SEG_CLASS_D = {BF16: (512, 520, 1024, 1032, 2048, 2056, 4096), F32: (256, 264, 512, 520, 1024, 1032, 2048)}   # each class's edge, edge + 8
SEG_SUM_D = {BF16: (8, 520, 1032, 2056), F32: (8, 264, 520, 1032)}                                              # 1, 1, 2, 3 slabs, the last partial


# every distribution at the width of one lane's vector and at one with a partial last chunk, V on both sides of the LDS switch
SEG_SMALL_CASES = [(op, dist, (4095, 4096)[i % 2], D, dt) for op in ("bwd", "sum") for i, dist in enumerate(SEG_DISTS)
                   for dt, D in ((BF16, 8), (F32, 264))] + \
                  [(op, dist, 4096, 520, BF16) for op in ("bwd", "sum") for dist in ("long", "longpad", "outside")]
# every dispatch class: (op, distribution, V, D, dtype, exact)
SEG_CLASS_CASES = [("bwd", "long", V, D, dt, True) for dt in (BF16, F32) for D in SEG_CLASS_D[dt] for V in (4095, 4096)] + \
                  [("bwd", "longpad", (4096, 4095)[i % 2], D, dt, False) for dt in (BF16, F32) for i, D in enumerate(SEG_CLASS_D[dt])] + \
                  [("sum", "long", (4095, 4096)[i % 2], D, dt, ex) for dt in (BF16, F32) for i, D in enumerate(SEG_SUM_D[dt]) for ex in (True, False)]


def check_segment(be, op, dist, V, D, dtype, exact, seed=0):
    """op = "bwd" (mh_embed_segment_bwd: pad id skipped, table [V, D] contiguous) or "sum" (mh_embed_segment_sum: every id,
    table rows D + 4 floats apart); rows of the gradient D + 8 apart with NaN in the gap; run twice into the same table"""
    g = gen(4000 + seed)
    segs, n_out, pad = seg_distributions(V)[dist]
    if op == "sum":
        pad = -1
    ids = torch.cat([torch.full((c,), v, dtype=I64) for v, c in segs])
    n_in = ids.numel()
    n = n_in + n_out
    seg = torch.searchsorted(ids, torch.arange(V + 1))
    ld = D + 8
    x = torch.full((n, ld), float("nan"), dtype=dtype)
    x[:, :D] = values((n, D), dtype, g, exact)
    src = torch.randperm(n, generator=g)
    x[src[n_in:]] = float("nan")                          # rows of the occurrences behind seg_start[V]: skipped
    if pad >= 0:
        x[src[:n_in][ids == pad]] = float("nan")          # the pad id's rows: skipped by segment_bwd
    src, seg, x, ids = src.to(be.dev), seg.to(be.dev), x.to(be.dev), ids.to(be.dev)
    buf, tab = fenced((V, D), F32, be.dev, ld=(D + 4) if op == "sum" else None)
    tab.copy_(values((V, D), F32, g, exact))
    prior = tab.clone().to(F64)
    buf0 = buf.clone()
    for _ in range(2):
        if op == "sum":
            be.segment_sum(src, seg, x[:, :D], tab, n)
        else:
            be.segment_bwd(src, seg, x, ld, tab, n, pad)
    keep = ids != pad
    idk, terms = ids[keep], x[src[:n_in][keep], :D].to(F64)
    ref = prior.clone().index_add_(0, idk, 2 * terms)
    mag = prior.abs().index_add_(0, idk, 2 * terms.abs())
    cnt = 2 * torch.bincount(idk, minlength=V).to(F64)[:, None]
    return _accumulated(tab, ref, mag, cnt, prior, exact) + stray(buf, buf0, tab)


# ------------------------------------------------------------------------------------------------------- split_hi_lo / table_norm
SPLIT_CAP = 4 * (grid_cap("embed_split_hi_lo")[1] * 256) + 4
SPLIT_SIZES = (4, 1028, SPLIT_CAP)


def check_split(be, n, dtype, exact, seed=0):
    g = gen(5000 + seed)
    s = (ints((n,), F32, g, lim=200) if exact else torch.randn(n, generator=g) * 3).to(be.dev)
    bh, hi = fenced((n,), dtype, be.dev)
    bl, lo = fenced((n,), dtype, be.dev)
    bh0, bl0 = bh.clone(), bl.clone()
    be.split_hi_lo(s, hi, lo)
    nb = inexact(hi, s.to(F64)) if exact else int((bits(hi) != bits(s.to(dtype))).sum())
    if exact:
        nb += int((lo != 0).sum())
    s64 = s.to(F64)
    nb += int((~((hi.to(F64) + lo.to(F64) - s64).abs() <= E[dtype] ** 2 * s64.abs())).sum())
    return nb + stray(bh, bh0, hi) + stray(bl, bl0, lo)


TABLE_NORM_CAP = (4 * grid_cap("embed_table_norm_bwd")[1] + 3, 8)
TABLE_NORM_CASES = [(V, D, dt, pad) for dt in (BF16, F32) for (V, D, pad) in
                    ((41, 8, 0), (41, 520 if dt == BF16 else 264, 40), (7, 504 if dt == BF16 else 248, -1), (5, 1024, 2))]


def check_table_norm(be, V, D, dtype, pad, seed=0):
    g = gen(6000 + seed)
    t_hi = torch.randn((V, D), generator=g).to(dtype).to(be.dev)
    t_lo = (torch.randn((V, D), generator=g) * 2.0 ** -9).to(dtype).to(be.dev)
    e = torch.randn((V, D), generator=g).to(dtype).to(be.dev)
    rstd = (0.5 + torch.rand(V, generator=g)).to(be.dev)
    buf, acc = fenced((V, D), F32, be.dev)
    acc.copy_(torch.randn((V, D), generator=g))
    acc0 = acc.clone()
    buf0 = buf.clone()
    be.table_norm_bwd(t_hi, t_lo, e, rstd, acc, pad)
    Tt, e64, r2 = t_hi.to(F64) + t_lo.to(F64), e.to(F64), rstd.to(F64)[:, None] ** 2
    dotabs = (Tt * e64).abs().sum(-1, keepdim=True)
    cf = r2 * (Tt * e64).sum(-1, keepdim=True) / D
    ref = acc0.to(F64) + Tt - e64 * cf
    bound = 3 * U24 * (acc0.to(F64).abs() + Tt.abs() + (e64 * cf).abs()) + e64.abs() * (r2 / D) * (D + 6) * U24 * dotabs
    live = torch.ones(V, dtype=torch.bool, device=be.dev)
    nb = 0
    if pad >= 0:
        live[pad] = False
        nb += inexact(acc[pad], acc0[pad].to(F64))
    return nb + bad(acc[live], ref[live], 2 * bound[live]) + stray(buf, buf0, acc)


# --------------------------------------------------------------------------------------------------------------- token_segments
TOKSEG_CASES = [(1, 1, 1, "mixed"), (SEG_CH - 1, 1, 255, "mixed"), (SEG_CH, 1, 256, "mixed"), (SEG_CH + 1, 1, 257, "mixed"),
                (3 * SEG_CH, 1, 15999, "mixed"), (1, 7, 257, "mixed"), ((SEG_CH - 1) // 7, 7, 255, "mixed"),
                (SEG_CH // 7 + 1, 7, 1, "mixed"), (3 * SEG_CH // 7 + 1, 7, 15999, "mixed"), (SEG_CH + 1, 1, 257, "oneid"),
                (SEG_CH // 7 + 1, 7, 256, "oneid"), (300, 7, 255, "inrange")]


def check_token_segments(be, n_rows, n_cols, V, kind, seed=0):
    """seg_start against the bucket counts; src_rows a permutation of the occurrences through the affine row map, every
    position holding an occurrence of the bucket that owns it (ids outside [0, V) behind seg_start[V]); a repeat call gives
    the same seg_start"""
    g = gen(7000 + seed)
    n = n_rows * n_cols
    ids = torch.randint(0, V, (n_rows, n_cols), generator=g)
    if kind == "oneid":
        ids[:] = V // 2
    flat = ids.view(-1)
    flat[0] = V - 1
    if kind == "mixed" and n >= 4:
        k = max(1, n // 9)
        flat[torch.randperm(n, generator=g)[: 2 * k]] = torch.cat([torch.full((k,), -1 - seed), torch.full((k,), V + 5 * seed)])
        flat[1], flat[2], flat[-1] = V, -1, V - 1
    wide = torch.full((n_rows, n_cols + 3), V // 3, dtype=I64)   # an in-range id in the unused columns: it would be counted
    wide[:, :n_cols] = ids
    tok = wide.to(be.dev)[:, :n_cols]
    row_mul, col_mul, add = n_cols + 2, 1, 1
    bs, src = fenced((n,), I64, be.dev)
    bg, seg = fenced((V + 1,), I64, be.dev)
    bs0, bg0 = bs.clone(), bg.clone()
    be.token_segments(tok, V, row_mul, col_mul, add, src, seg)
    seg1 = seg.clone()
    bucket = torch.where((tok >= 0) & (tok < V), tok, torch.full_like(tok, V)).reshape(-1)
    counts = torch.bincount(bucket, minlength=V + 1)
    ref = torch.cumsum(counts, 0) - counts
    nb = int((seg != ref).sum())
    q = src - add
    r, j = torch.div(q, row_mul, rounding_mode="floor"), q % row_mul
    ok = (r >= 0) & (r < n_rows) & (j < n_cols)
    nb += int((~ok).sum())
    occ = torch.where(ok, r * n_cols + j, torch.zeros_like(q))
    nb += int((torch.sort(occ).values != torch.arange(n, device=be.dev)).sum())                  # a permutation
    owner = torch.searchsorted(torch.cat([ref, ref.new_tensor([n])]), torch.arange(n, device=be.dev), right=True) - 1
    nb += int((bucket[occ] != owner).sum())                                                     # grouped by bucket
    be.token_segments(tok, V, row_mul, col_mul, add, src, seg)
    nb += int((seg != seg1).sum())
    return nb + stray(bs, bs0, src) + stray(bg, bg0, seg)


# -------------------------------------------------------------------------------------------------------------------- transpose
TRANSPOSE_SHAPES = ((1, 1), (63, 65), (64, 64), (65, 63), (8, 130))
TRANSPOSE_VARIANTS = ("aligned", "ldi odd", "input offset", "output odd")


def check_transpose(be, R, C, dtype, variant, seed=0):
    g = gen(8000 + seed)
    nv = NVEC[dtype]
    up = lambda x: (x + nv - 1) // nv * nv
    ldi = up(C) + nv + (1 if variant == "ldi odd" else 0)
    ldo = (up(R) + nv) | 1 if variant == "output odd" else up(R) + nv
    ioff = 1 if variant == "input offset" else 0
    ibuf = torch.full((FENCE + ioff + R * ldi,), float("nan"), dtype=dtype)
    x = ibuf[FENCE + ioff:].view(R, ldi)[:, :C]
    x.copy_(ints((R, C), dtype, g, lim=100))
    ibuf = ibuf.to(be.dev)
    x = ibuf[FENCE + ioff:].view(R, ldi)[:, :C]
    buf, out = fenced((C, R), dtype, be.dev, ld=ldo, off=1 if variant == "output odd" else 0)
    buf0 = buf.clone()
    be.transpose(x, out)
    return inexact(out, x.T.to(F64)) + stray(buf, buf0, out)


# ---------------------------------------------------------------------------------------------------------------------- collate
ROW_SENTINEL = 31111       # int16 corpus rows outside every window


def collate_ref(tokens, win_start, win_len, L, pad_id):
    ar = torch.arange(L, device=tokens.device)
    valid = ar[None, :] < win_len[:, None]
    idx = (win_start[:, None] + ar[None, :]).clamp_(0, tokens.shape[0] - 1)
    return torch.where(valid[:, :, None], tokens[idx].to(I64), torch.full((), pad_id, dtype=I64, device=tokens.device))


# (T, B, L, windows (start, len) or None for random ones, pad id); starts are relative to the corpus of N_COLLATE events
N_COLLATE = 500
COLLATE_CASES = [(8, 4, 16, ((0, 16), (N_COLLATE - 16, 16), (40, 0), (77, 1)), -3),
                 (1, 3, 9, ((N_COLLATE - 9, 9), (100, 1), (200, 0)), 0),
                 (8, 1, 33, ((N_COLLATE - 5, 5),), -1),
                 (1, 1, 1, ((N_COLLATE - 1, 1),), 7)]
COLLATE_CAP = (8, (256 * grid_cap("collate_windows")[1] + 8) // 24, 3, None, -2)      # B L T = 256 x 16384 + 8


def check_collate(be, T, B, L, wins, pad_id, seed=0, slice_b=None):
    g = gen(9000 + seed)
    N, margin = N_COLLATE, 40
    tokens = torch.full((N + 2 * margin, T), ROW_SENTINEL, dtype=I16)      # the corpus is the middle N rows
    if wins is None:
        length = torch.randint(0, L + 1, (B,), generator=g)
        start = (torch.rand(B, generator=g) * (N - length + 1).double()).long().clamp_(max=N) + margin
        start[0], length[0] = margin + N - L, L
        if slice_b:
            start, length, B = start[:slice_b], length[:slice_b], slice_b
    else:
        start = torch.tensor([w[0] for w in wins]) + margin
        length = torch.tensor([w[1] for w in wins])
    used = torch.zeros(N + 2 * margin, dtype=torch.bool)
    ar = torch.arange(L)
    rows = (start[:, None] + ar[None, :])[ar[None, :] < length[:, None]]
    used[rows] = True
    assert int(rows.max()) == margin + N - 1 and not used[:margin].any()
    tokens[used] = torch.randint(-3000, 3000, (int(used.sum()), T), generator=g).to(I16)
    tokens, start, length = tokens.to(be.dev), start.to(be.dev), length.to(be.dev)
    buf, out = fenced((B, L, T), I64, be.dev)
    buf0 = buf.clone()
    be.collate(tokens[: margin + N], start, length, out, pad_id)    # n_events = the corpus's end: the last window ends on it
    return int((out != collate_ref(tokens, start, length, L, pad_id)).sum()) + int((out == ROW_SENTINEL).sum()) + stray(buf, buf0, out)


# ---------------------------------------------------------------------------------------------------------------------- augment
def tokenizer(ver):
    import midi_model_amd as mm
    return mm.MIDITokenizerV1() if ver == "v1" else mm.MIDITokenizerV2()


def aug_tab(tok):
    from midi_model_amd.tokenizer import augment_table
    return torch.tensor(augment_table(tok), dtype=I32)


def event(tok, name, **kw):
    return tok.event2tokens([name] + [kw.get(p, 0) for p in tok.events[name]])


def pieces_tensor(pieces, T):
    """-> (tokens int16 [N, T], piece_off int64 [P + 1])"""
    off = np.cumsum([0] + [len(p) for p in pieces])
    rows = [r for p in pieces for r in p]
    tokens = torch.tensor(rows, dtype=I64).reshape(-1, T).to(I16)
    return tokens, torch.from_numpy(off).to(I64)


def stats_pieces(tok):
    """pieces of 0, 1, 255, 256, 257 and 600 events; one with drum notes only, one without notes; tracks 0 and 127, channel 15"""
    def note(i, track=None, channel=None, pitch=None):
        return event(tok, "note", time1=i % 128, track=i % 5 if track is None else track, channel=i % 9 if channel is None else channel,
                     pitch=30 + i % 60 if pitch is None else pitch, velocity=1 + i % 127, duration=1 + i % 50)
    def other(i):
        return [event(tok, "control_change", track=i % 7, channel=i % 16, controller=i % 128, value=i % 128),
                event(tok, "set_tempo", bpm=1 + i % 200), event(tok, "patch_change", track=3, channel=15, patch=i % 128)][i % 3]
    def mixed(n, seed):
        return [note(i + seed) if (i * 7 + seed) % 4 else other(i) for i in range(n)]
    P = [[], [note(0, track=127, channel=15, pitch=0)], mixed(255, 1), mixed(256, 2), mixed(257, 3), mixed(600, 4)]
    P[5][599] = note(599, track=0, channel=15, pitch=127)
    P[5][300] = note(300, track=127, channel=9, pitch=1)
    P[3][255] = note(255, track=127, channel=0, pitch=5)
    P.append([note(i, channel=9, track=i % 3) if i % 2 else other(i) for i in range(40)])      # drum notes only: (128, -1)
    P.append([other(i) for i in range(30)])                                                     # no notes
    P.append([[tok.bos_id] + [tok.pad_id] * (tok.max_token_seq - 1)])
    return P


def piece_stats_ref(tokens, piece_off, tab, count_drums=False):
    """[P, 130] int32: lowest / highest pitch among the notes off channel 9 (128 / -1 without any), per ORIGINAL track the bit
    mask of its notes' ORIGINAL channels"""
    t = tab.tolist()
    dev = tokens.device
    P = piece_off.numel() - 1
    a = tokens.to(I64)
    piece = torch.searchsorted(piece_off, torch.arange(a.shape[0], device=dev), right=True) - 1
    note = a[:, 0] == t[1]
    pc, tr, ch, pitch = piece[note], a[note, t[7]] - t[26], a[note, t[13]] - t[28], a[note, t[19]] - t[30]
    off9 = (ch != 9) | count_drums           # (count_drums: the wrong kernel "rule (1) counting drum notes")
    lo = torch.full((P,), 128, dtype=I64, device=dev).scatter_reduce_(0, pc[off9], pitch[off9], "amin")
    hi = torch.full((P,), -1, dtype=I64, device=dev).scatter_reduce_(0, pc[off9], pitch[off9], "amax")
    flag = torch.zeros((P, 128, 32), dtype=I64, device=dev)
    flag[pc, tr, ch] = 1
    mask = (flag << torch.arange(32, device=dev)).sum(-1)
    return torch.cat([lo[:, None], hi[:, None], mask], 1).to(I32)


def check_piece_stats(be, tok):
    tab = aug_tab(tok)
    tokens, off = pieces_tensor(stats_pieces(tok), tok.max_token_seq)
    P = off.numel() - 1
    tokens, off, tab = tokens.to(be.dev), off.to(be.dev), tab.to(be.dev)
    buf, stats = fenced((P, 130), I32, be.dev)
    buf0 = buf.clone()
    be.piece_stats(tokens, off, tab, stats)
    ref = piece_stats_ref(tokens, off, tab)
    assert ref[6, :2].tolist() == [128, -1] and ref[7, :2].tolist() == [128, -1] and int(ref[7, 2:].abs().sum()) == 0
    assert int(ref[5, 2]) & (1 << 15) and int(ref[5, 2 + 127]) == 1 << 9
    return int((stats != ref).sum()) + stray(buf, buf0, stats)


def augment_ref(tokens, win_start, win_len, win_piece, shifts, stats, tab, L, pad_id, wrong=None):
    """mh_augment_collate_windows, row by row in whole-array form: [B, L, T] int64.  `wrong` names one of the wrong kernels that
    tests/test_index_bounds_host.py shows the checks to reject (AUGMENT_WRONG); None is the rule as the reference has it."""
    assert wrong is None or wrong in AUGMENT_WRONG
    mod = torch.fmod if wrong == "C-style % on negatives" else torch.remainder
    t = tab.tolist()
    dev = tokens.device
    B, T = win_start.numel(), tokens.shape[1]
    ar = torch.arange(L, device=dev)
    valid = (ar[None, :] < win_len[:, None]).reshape(-1)
    v = tokens[(win_start[:, None] + ar[None, :]).clamp_(0, tokens.shape[0] - 1).reshape(-1)].to(I64)
    sh = shifts.to(I64).repeat_interleave(L, 0)
    pc = win_piece.repeat_interleave(L)
    st = stats.to(I64)
    lo, hi = st[pc, 0], st[pc, 1]
    changed = ~((hi >= 0) & ((lo + sh[:, 0] < 0) | (hi + sh[:, 0] > 127)))
    out = v.clone()
    tr_new = torch.full_like(pc, -1)
    for e in range(6):
        if t[1 + e] < 0:
            continue
        m = changed & (v[:, 0] == t[1 + e])
        tcol, ccol = t[7 + e], t[13 + e]
        c0 = torch.full_like(pc, -1)
        if tcol:
            trn = mod(v[:, tcol] - t[26] + sh[:, 4], t[27])
            tr_new = torch.where(m, trn, tr_new)
            out[:, tcol] = torch.where(m, t[26] + trn, out[:, tcol])
        if ccol:
            c0 = v[:, ccol] - t[28]
            c = mod(c0 + sh[:, 5], t[29])
            again = c if wrong == "collision not re-shifted" else torch.where(c == 9, mod(9 + sh[:, 5], t[29]), c)
            c = again if wrong == "channel 9 shifted" else torch.where(c0 == 9, torch.full_like(c, 9), again)
            out[:, ccol] = torch.where(m, t[28] + c, out[:, ccol])
        if e == 0:
            out[:, t[19]] = torch.where(m & (c0 != 9), v[:, t[19]] + sh[:, 0], out[:, t[19]])
            out[:, t[20]] = torch.where(m, t[31] + (v[:, t[20]] - t[31] + sh[:, 1]).clamp(0 if wrong == "velocity clamp to 0" else 1, 127), out[:, t[20]])
        elif e == 2:
            ctrl = v[:, t[21]] - t[32]
            m = m & ((ctrl == 1) | (ctrl == 2) | (ctrl == 7) | (ctrl == 11))
            out[:, t[22]] = torch.where(m, t[33] + (v[:, t[22]] - t[33] + sh[:, 2]).clamp(1, 127), out[:, t[22]])
        elif e == 3:
            out[:, t[23]] = torch.where(m, t[34] + (v[:, t[23]] - t[34] + sh[:, 3]).clamp(1, t[35] - 1), out[:, t[23]])
        elif e == 5:
            sf, mi = v[:, t[24]] - t[36] - 7, v[:, t[25]] - t[37]
            sf = ((((sf * 7) % 12 + sh[:, 0]) % 12) * 7) % 12
            sf = torch.where((sf > 6) | ((mi == 1) & (sf >= 5)), sf - 12, sf) + 7
            look = (v[:, tcol] - t[26]) if wrong == "rule (2) looked up on the unshifted track" else tr_new
            drum = st[pc, 2 + look.clamp(0, 127)] == (1 << 9)
            out[:, t[24]] = torch.where(m, t[36] + torch.where(drum, torch.full_like(sf, 7), sf), out[:, t[24]])
    out = torch.where(valid[:, None], out, torch.full((), pad_id, dtype=I64, device=dev))
    return out.view(B, L, T)


AUGMENT_WRONG = ("channel 9 shifted", "collision not re-shifted", "velocity clamp to 0", "C-style % on negatives",
                 "rule (2) looked up on the unshifted track")


def augment_corpus(tok):
    """-> (pieces, shifts): a constructed corpus that reaches every branch of the rules (augment_census says which); shifts =
    (pitch, velocity, cc value, bpm, track, channel) per piece, negative track and channel shifts included"""
    v2 = "key_signature" in tok.events
    nbpm = tok.event_parameters["bpm"]

    def body(lowp, highp):
        ev = []
        for i in range(24):       # notes: velocities and pitches at both ends, every channel, tracks 0, 126, 127
            ev.append(event(tok, "note", time1=i, track=(0, 126, 127, 6, 8)[i % 5], channel=(i * 5) % 16 if (i * 5) % 16 != 9 else 10,
                            pitch=(lowp, highp)[i % 2], velocity=(1, 3, 64, 125, 127)[i % 5], duration=1 + i))
        ev += [event(tok, "note", track=5, channel=9, pitch=p, velocity=100, duration=2) for p in (0, 127, 35)]   # track 5: drums only
        ev += [event(tok, "note", track=6, channel=9, pitch=1, velocity=100, duration=2)]                         # track 6: mixed
        for c in (1, 2, 7, 11, 5, 0, 64):
            ev += [event(tok, "control_change", track=2, channel=(6, 12, 9, 3)[k % 4], controller=c, value=val) for k, val in enumerate((0, 2, 64, 126, 127))]
        ev += [event(tok, "set_tempo", track=1, bpm=b) for b in (0, 1, 5, 120, nbpm - 6, nbpm - 1)]
        ev += [event(tok, "patch_change", track=127, channel=c, patch=c) for c in range(16)]
        if v2:
            ev += [event(tok, "time_signature", track=126, nn=3, dd=2)]
            ev += [event(tok, "key_signature", track=3 + (i % 6), sf=i % 15, mi=i // 15) for i in range(30)]
        ev.append([tok.bos_id] + [tok.pad_id] * (tok.max_token_seq - 1))
        ev.append([tok.eos_id] + [tok.pad_id] * (tok.max_token_seq - 1))
        ev.append([tok.parameter_ids["pitch"][5]] + [tok.parameter_ids["track"][1]] * (tok.max_token_seq - 1))   # not an event id
        return ev
    low = [event(tok, "note", track=1, channel=0, pitch=2, velocity=9, duration=1)]
    high = [event(tok, "note", track=1, channel=15, pitch=126, velocity=9, duration=1)]
    pieces = [body(40, 80) + low, body(40, 80) + high, body(4, 123), body(3, 124), body(60, 61), body(20, 90)]
    shifts = [(-3, -5, 4, 2, 1, 3), (3, 5, -4, -2, 1, 3), (4, 10, 10, 10, 1, 3), (-3, -10, -10, -10, -2, -3), (0, 0, 0, 0, 0, 0), (-4, 7, -9, 300, 127, 16 - 7)]
    return pieces, shifts


CENSUS_COMMON = ["unchanged: a pitch below 0", "unchanged: a pitch above 127", "rule 1 spared: only a channel-9 pitch leaves the range",
                 "channel stays 9", "channel lands on 9 and is shifted again", "negative channel shift wraps", "negative track shift wraps",
                 "velocity clamped at 1", "velocity clamped at 127", "cc 1 clamped", "cc 2 clamped", "cc 7 clamped", "cc 11 clamped",
                 "cc clamped at 1", "cc clamped at 127", "another controller left alone", "bpm clamped at 1", "bpm clamped at its top",
                 "an id that is no event passes through", "padded tail"]
CENSUS_V2 = ["major key with sf 5..6 kept", "minor key with sf >= 5 folded", "sf > 6 folded", "rule 2 fires after the track shift",
             "rule 2 does not fire after the track shift"]


def augment_census(tok, pieces, shifts, win_len, L):
    """how often each rule branch is reached, from the inputs and the shifts alone"""
    c = collections.Counter()
    pid, npar = tok.parameter_ids, tok.event_parameters

    def col(name, pn):
        return 1 + tok.events[name].index(pn)
    for rows, (ps, vs, cs, bs, ts, chs) in zip(pieces, shifts):
        a = torch.tensor(rows, dtype=I64).reshape(-1, tok.max_token_seq)
        is_ev = {n: a[:, 0] == i for n, i in tok.event_ids.items()}
        note = a[is_ev["note"]]
        ch, p = note[:, col("note", "channel")] - pid["channel"][0], note[:, col("note", "pitch")] - pid["pitch"][0]
        tr = note[:, col("note", "track")] - pid["track"][0]
        low, high = bool((p[ch != 9] + ps < 0).any()), bool((p[ch != 9] + ps > 127).any())
        c["unchanged: a pitch below 0"] += low
        c["unchanged: a pitch above 127"] += high
        if low or high:
            continue
        c["rule 1 spared: only a channel-9 pitch leaves the range"] += bool(((p[ch == 9] + ps < 0) | (p[ch == 9] + ps > 127)).any())
        for n, m in is_ev.items():
            if "channel" in tok.events[n]:
                c0 = a[m, col(n, "channel")] - pid["channel"][0]
                c["channel stays 9"] += int((c0 == 9).sum()) * (chs % npar["channel"] != 0)
                c["channel lands on 9 and is shifted again"] += int(((c0 != 9) & ((c0 + chs) % npar["channel"] == 9)).sum())
                c["negative channel shift wraps"] += int((c0 + chs < 0).sum())
            c["negative track shift wraps"] += int((a[m, col(n, "track")] - pid["track"][0] + ts < 0).sum())
        vel = note[:, col("note", "velocity")] - pid["velocity"][0] + vs
        c["velocity clamped at 1"] += int((vel < 1).sum())
        c["velocity clamped at 127"] += int((vel > 127).sum())
        cc = a[is_ev["control_change"]]
        ctrl, val = cc[:, col("control_change", "controller")] - pid["controller"][0], cc[:, col("control_change", "value")] - pid["value"][0] + cs
        for k in (1, 2, 7, 11):
            c["cc %d clamped" % k] += int(((ctrl == k) & ((val < 1) | (val > 127))).sum())
        rule = (ctrl == 1) | (ctrl == 2) | (ctrl == 7) | (ctrl == 11)
        c["cc clamped at 1"] += int((rule & (val < 1)).sum())
        c["cc clamped at 127"] += int((rule & (val > 127)).sum())
        c["another controller left alone"] += int((~rule).sum()) * (cs != 0)
        bpm = a[is_ev["set_tempo"], col("set_tempo", "bpm")] - pid["bpm"][0] + bs
        c["bpm clamped at 1"] += int((bpm < 1).sum())
        c["bpm clamped at its top"] += int((bpm > npar["bpm"] - 1).sum())
        known = torch.zeros(a.shape[0], dtype=torch.bool)
        for m in is_ev.values():
            known |= m
        c["an id that is no event passes through"] += int((~known).sum())
        if "key_signature" in is_ev:
            ks = a[is_ev["key_signature"]]
            sf, mi = ks[:, col("key_signature", "sf")] - pid["sf"][0] - 7, ks[:, col("key_signature", "mi")] - pid["mi"][0]
            sf2 = ((((sf * 7) % 12 + ps) % 12) * 7) % 12
            c["major key with sf 5..6 kept"] += int(((mi == 0) & (sf2 >= 5) & (sf2 <= 6)).sum())
            c["minor key with sf >= 5 folded"] += int(((mi == 1) & (sf2 >= 5) & (sf2 <= 6)).sum())
            c["sf > 6 folded"] += int((sf2 > 6).sum())
            drum_only = torch.tensor([int(x) for x in tr.unique() if bool((ch[tr == x] == 9).all())], dtype=I64)
            k0 = ks[:, col("key_signature", "track")] - pid["track"][0]
            k1 = (k0 + ts) % npar["track"]
            d0, d1 = torch.isin(k0, drum_only), torch.isin(k1, drum_only)
            c["rule 2 fires after the track shift"] += int((d1 & ~d0 & (sf2 != 0)).sum())
            c["rule 2 does not fire after the track shift"] += int((d0 & ~d1 & (sf2 != 0)).sum())
    c["padded tail"] += int((torch.as_tensor(win_len) < L).sum())
    need = CENSUS_COMMON + (CENSUS_V2 if "key_signature" in tok.events else [])
    missing = [k for k in need if c[k] < 1]
    assert not missing, f"the constructed corpus does not reach: {missing}"
    return c


def augment_windows(pieces):
    """whole pieces, then cuts inside them: -> (piece, start inside the piece, length) lists, L"""
    wins = [(i, 0, len(p)) for i, p in enumerate(pieces)]
    wins += [(i, 7 + 3 * i, 50 + i) for i in range(len(pieces))] + [(0, 5, 0), (2, len(pieces[2]) - 1, 1)]
    return wins, max(w[2] for w in wins)


def check_augment(be, tok, orc):
    """the constructed corpus: census first, then every window against oracle.augment on the whole file, cut afterwards"""
    pieces, shifts = augment_corpus(tok)
    wins, L = augment_windows(pieces)
    augment_census(tok, pieces, shifts, [w[2] for w in wins], L)
    T = tok.max_token_seq
    margin = [[ROW_SENTINEL] * T] * 9
    tokens, off = pieces_tensor([margin] + pieces + [margin], T)
    whole = [orc.augment(tok, np.asarray(p, dtype=np.int16).reshape(-1, T), s) for p, s in zip(pieces, shifts)]
    want = torch.full((len(wins), L, T), tok.pad_id, dtype=I64)
    for b, (i, s, n) in enumerate(wins):
        want[b, :n] = torch.from_numpy(whole[i][s: s + n].astype(np.int64))
    assert sum(int((w != np.asarray(p).reshape(-1, T)).any()) for w, p in zip(whole, pieces)) == len(pieces) - 2
    start = torch.tensor([int(off[1 + i]) + s for i, s, _ in wins])
    length = torch.tensor([n for _, _, n in wins])
    piece = torch.tensor([1 + i for i, _, _ in wins])
    sh = torch.tensor([shifts[i] for i, _, _ in wins], dtype=I32)
    tab = aug_tab(tok)
    tokens, off, start, length, piece, sh, tab = (x.to(be.dev) for x in (tokens, off, start, length, piece, sh, tab))
    stats = torch.empty((off.numel() - 1, 130), dtype=I32, device=be.dev)
    be.piece_stats(tokens, off, tab, stats)
    nb = int((stats != piece_stats_ref(tokens, off, tab)).sum())
    buf, out = fenced((len(wins), L, T), I64, be.dev)
    buf0 = buf.clone()
    be.augment_collate(tokens, start, length, piece, sh, stats, tab, out, tok.pad_id)
    nb += int((out != want.to(be.dev)).sum()) + int((out == ROW_SENTINEL).sum())
    nb += int((augment_ref(tokens, start, length, piece, sh, stats, tab, L, tok.pad_id) != want.to(be.dev)).sum())   # the whole-array form itself
    return nb + stray(buf, buf0, out)


AUGMENT_CAP_ROWS = 256 * 16384 + 3      # = 13 x 322639: the launcher's cap of 16384 blocks of 256 rows, and three rows


def check_augment_cap(be, tok, L=13, slice_b=None, seed=0):
    """B L = 256 x 16384 + 3 rows of windows over the constructed corpus, against the whole-array form"""
    assert AUGMENT_CAP_ROWS % L == 0
    B = slice_b or AUGMENT_CAP_ROWS // L
    g = gen(9500 + seed)
    pieces, shifts = augment_corpus(tok)
    T = tok.max_token_seq
    tokens, off = pieces_tensor(pieces, T)
    piece = torch.randint(0, len(pieces), (B,), generator=g)
    length = torch.randint(0, L + 1, (B,), generator=g)
    plen = (off[1:] - off[:-1])[piece]
    start = off[piece] + (torch.rand(B, generator=g) * (plen - length + 1).double()).long().clamp_(min=0)
    alt = torch.tensor(shifts + [tuple(-x for x in s) for s in shifts], dtype=I32)
    sh = alt[(piece + len(pieces) * torch.randint(0, 2, (B,), generator=g))]
    tab = aug_tab(tok)
    tokens, off, start, length, piece, sh, tab = (x.to(be.dev) for x in (tokens, off, start, length, piece, sh, tab))
    stats = piece_stats_ref(tokens, off, tab)
    buf, out = fenced((B, L, T), I64, be.dev)
    buf0 = buf.clone()
    be.augment_collate(tokens, start, length, piece, sh, stats, tab, out, tok.pad_id)
    ref = augment_ref(tokens, start, length, piece, sh, stats, tab, L, tok.pad_id)
    assert int((ref != collate_ref(tokens, start, length, L, tok.pad_id)).any(-1).sum()) > B      # most rows do change
    return int((out != ref).sum()) + stray(buf, buf0, out)
