"""mh_sample_top_p_k_rows on the MI355X: the fused sampler with temperature, top-p, top-k and both masks per row, against the
uniform entry point launched once per row with that row's scalars and masks (the same-arithmetic contract: every row, no exclusion)
and against emu_ops.sample_top_p_k per row.  The cases are ref_streamers.sampler_case's, one per instantiation (range lengths
1...128, 129...512, 513...2048 at odd `lo`: a range clipped at V, a ban that leaves one candidate, the peaked rows), at token
position 1 and -- the same ranges restated as per-row first masks -- at position 0."""
import pytest
import torch

import emu_ops as emu
import ref_streamers as R
from ref_streamers import BF16, F32

pytestmark = pytest.mark.gpu

DTYPES = [F32, BF16]
PARAMS = [(0.5, 0.9, 20), (1.0, 0.98, 1), (1.7, 0.5, 64), (0.8, 1.0, 2),
          (1.0, 0.0, 20), (1.3, 0.98, 63), (0.6, 0.7, 5), (1.0, 0.98, 20)]
SENTINEL = -7


@pytest.fixture(scope="module")
def ops():
    import midi_model_amd.ops as real
    return real


def row_params(B):
    p = [PARAMS[b % 8] for b in range(B)]
    return ([float(x[0]) for x in p], [float(x[1]) for x in p], [int(x[2]) for x in p])


FIRST_LO = 37   # position 0: every row's first mask lies in [FIRST_LO, FIRST_LO + 64 * tmax), the span the host states


def position0(case, tmax):
    """the case restated for token position 0, where the host states ONE span for all rows: row b's FIRST MASK is a run of
    SAMPLER_LENGTHS[tmax][b] ids at an offset of its own inside the span (the longest run fills it: the instantiation is the
    case's), with every third id cleared at a phase of its own (rows differing in which ids are cleared); row b's BAN is the
    case's plus the last id of its run; row 2's ban leaves exactly one candidate.  -> (first [B, V], ban [B, V], span, row 2's id)"""
    B, V = case["B"], case["V"]
    lens, width = R.SAMPLER_LENGTHS[tmax], 64 * tmax
    assert max(lens) == width and FIRST_LO + width <= V
    first = torch.zeros((B, V), dtype=torch.uint8)
    ban = case["ban"][None, :].repeat(B, 1)
    only = None
    for b, n in enumerate(lens):
        l = FIRST_LO + min(1 + 5 * b, width - n)
        first[b, l:l + n] = 1
        if b == 2:
            only = l + n // 2
            ban[b] = 0
            ban[b, l:l + n] = 1
            ban[b, only] = 0
        elif n >= 8:
            first[b, l + 1 + b % 3:l + n - 1:3] = 0
            ban[b, l + n - 1] = 1   # (not the first: row 0's run starts at its peak, the only id of non-zero probability)
    assert bool(((first == 1) & (ban == 0)).any(1).all()), "a row without a candidate"
    return first, ban, (FIRST_LO, FIRST_LO + width), only


def launch_rows(ops, case, pos, temp, top_p, top_k, first, ban, span, fill_rest=0, rows=None):
    """one launch of the rows form over `rows` (default: all); -> the ids, the buffer around them checked for sentinels"""
    c = case
    sel = list(range(c["B"])) if rows is None else rows
    n = len(sel)
    buf = torch.full((n + 2, fill_rest + 1), SENTINEL, dtype=torch.int64, device="cuda")
    out_b = torch.full((n + 2,), SENTINEL, dtype=torch.int64, device="cuda")
    idx = torch.tensor(sel)
    pick = lambda m: m.cuda() if m.dim() == 1 else m[idx].contiguous().cuda()
    ops.sample_top_p_k_rows(c["logits"][idx].cuda(), pick(first), c["lo_tab"].cuda(), c["hi_tab"].cuda(), c["ev"][idx].cuda(), pos,
                            c["q"][idx].contiguous().cuda(), buf[1:1 + n, 0], c["V"],
                            torch.tensor([temp[b] for b in sel], dtype=torch.float32, device="cuda"),
                            torch.tensor([top_p[b] for b in sel], dtype=torch.float32, device="cuda"),
                            torch.tensor([top_k[b] for b in sel], dtype=torch.int32, device="cuda"), pick(ban),
                            out_b=out_b[1:1 + n], first_span=span, max_range=c["max_range"], fill_rest=fill_rest, fill_id=-3)
    torch.cuda.synchronize()
    assert bool((buf[0] == SENTINEL).all()) and bool((buf[-1] == SENTINEL).all()), "a write outside the rows of `out`"
    assert out_b[0].item() == SENTINEL and out_b[-1].item() == SENTINEL and torch.equal(out_b[1:1 + n], buf[1:1 + n, 0])
    assert bool((buf[1:1 + n, 1:] == -3).all()), "fill_rest entries not written"
    return buf[1:1 + n, 0].cpu()


def launch_uniform_row(ops, case, pos, b, temp, top_p, top_k, first_b, ban_b, span):
    c = case
    buf = torch.full((3,), SENTINEL, dtype=torch.int64, device="cuda")
    ops.sample_top_p_k(c["logits"][b:b + 1].cuda(), first_b.cuda(), c["lo_tab"].cuda(), c["hi_tab"].cuda(), c["ev"][b:b + 1].cuda(), pos,
                       c["q"][b:b + 1].contiguous().cuda(), buf[1:2], c["V"], temp, top_p, top_k, first_span=span,
                       max_range=c["max_range"], ban_mask=ban_b.cuda())
    torch.cuda.synchronize()
    assert buf[0].item() == SENTINEL and buf[2].item() == SENTINEL
    return int(buf[1])


def row_case(case, pos, b, temp, top_p, top_k, first_b, ban_b):
    """row b as a one-row case of ref_streamers.sampler_emulate / sampler_undecided (which sample at position 1 from the range
    tables: a table entry of -1 makes them read the first mask instead, which is position 0)"""
    c = dict(case, logits=case["logits"][b:b + 1], ev=case["ev"][b:b + 1], q=case["q"][b:b + 1], B=1, temp=temp, top_p=top_p,
             top_k=top_k, fm=first_b, ban=ban_b)
    if pos == 0:
        c["lo_tab"] = c["hi_tab"] = torch.full_like(case["lo_tab"], -1)
    return c


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("pos", [1, 0])
@pytest.mark.parametrize("tmax", [2, 8, 32])
def test_rows_equal_the_uniform_kernel_and_the_emulation(ops, tmax, pos, dtype):
    """(a) every row's id is mh_sample_top_p_k's for that row's scalars and masks on the same logits and q -- all rows compared;
    (b) it is emu_ops.sample_top_p_k's on the rows the emulation does not mark as decided by fp32 summation order, at most 2 % of
    the rows left out (test_streamer_bounds_host.py's cap; on the CPU the emulation marks none of these); (d) sentinels around
    `out` / `out_b` intact and, at position 0, the fill_rest entries written."""
    case = R.sampler_case(tmax, dtype, 100 + tmax)
    B, V = case["B"], case["V"]
    temp, top_p, top_k = row_params(B)
    if pos == 0:
        first, ban, span, only = position0(case, tmax)
    else:
        first, ban, span = case["fm"], case["ban"], (0, 0)
    got = launch_rows(ops, case, pos, temp, top_p, top_k, first, ban, span, fill_rest=7 if pos == 0 else 0)
    row = lambda m, b: m if m.dim() == 1 else m[b].contiguous()
    left_out = 0
    for b in range(B):
        fb, bb = row(first, b), row(ban, b)
        uni = launch_uniform_row(ops, case, pos, b, temp[b], top_p[b], top_k[b], fb, bb, span)
        assert int(got[b]) == uni, (b, PARAMS[b % 8], int(got[b]), uni)
        rc1 = row_case(case, pos, b, temp[b], top_p[b], top_k[b], fb, bb)
        if bool(R.sampler_undecided(rc1, emu)[0]):
            left_out += 1
            continue
        want = int(R.sampler_emulate(rc1, emu)[0])
        assert int(got[b]) == want, (b, PARAMS[b % 8], int(got[b]), want)
    assert left_out <= 0.02 * B, f"{left_out} of {B} rows decided by fp32 summation order"
    if pos == 0:
        assert bool((first.gather(1, got[:, None]) == 1).all()) and bool((ban.gather(1, got[:, None]) == 0).all()), \
            "an id outside the row's own masks"
        assert got[2].item() == only, "the one id row 2's ban leaves"
        assert got[0].item() == FIRST_LO + 1 == int(case["lo_tab"][0, 1]), "row 0's peak, the first id of its run"
        return
    lo, hi = case["lo_tab"][:, 1], case["hi_tab"][:, 1].clamp(max=V)
    assert bool(((got >= lo) & (got < hi)).all()), "an id outside the row's range"
    assert got[0].item() == int(lo[0]) and got[1].item() == int(hi[1]) - 1, "the peaked rows"
    assert got[2].item() == int(lo[2]) + R.SAMPLER_LENGTHS[tmax][2] // 2, "the one id the ban mask leaves"


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("tmax", [2, 8, 32])
def test_stride_zero_masks_and_equal_entries_give_the_uniform_launch(ops, tmax, dtype):
    """(c) [V] masks (stride 0) and arrays of equal entries: the ids of ONE uniform launch over all rows, at both positions (at
    position 0 the single first mask is the union of the rows' ranges)"""
    case = R.sampler_case(tmax, dtype, 100 + tmax)
    c, B, V = case, case["B"], case["V"]
    for pos in (1, 0):
        first = case["fm"].clone()
        span = (0, 0)
        if pos == 0:
            b = B - 2
            first[int(c["lo_tab"][b, 1]):int(c["hi_tab"][b, 1])] = 1
            span = (int(c["lo_tab"][b, 1]), int(c["hi_tab"][b, 1]))
        for t, p, k in ((0.5, 0.9, 20), (1.3, 0.98, 64)):
            buf = torch.full((B + 2,), SENTINEL, dtype=torch.int64, device="cuda")
            ops.sample_top_p_k(c["logits"].cuda(), first.cuda(), c["lo_tab"].cuda(), c["hi_tab"].cuda(), c["ev"].cuda(), pos,
                               c["q"].cuda(), buf[1:1 + B], V, t, p, k, first_span=span, max_range=c["max_range"],
                               ban_mask=c["ban"].cuda())
            torch.cuda.synchronize()
            got = launch_rows(ops, case, pos, [t] * B, [p] * B, [k] * B, first, case["ban"], span)
            assert torch.equal(got, buf[1:1 + B].cpu()), (pos, t, p, k)
            # ... and so do [B, V] masks whose rows are that one mask
            got2 = launch_rows(ops, case, pos, [t] * B, [p] * B, [k] * B, first[None].repeat(B, 1), case["ban"][None].repeat(B, 1), span)
            assert torch.equal(got2, got), (pos, t, p, k)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("tmax", [2, 8, 32])
def test_one_row(ops, tmax, dtype):
    """(e) B = 1: the last row of the case (the range clipped at V) alone, with each parameter set"""
    case = R.sampler_case(tmax, dtype, 100 + tmax)
    b = case["B"] - 1
    for t, p, k in PARAMS[:4]:
        got = launch_rows(ops, case, 1, {b: t}, {b: p}, {b: k}, case["fm"], case["ban"], (0, 0), rows=[b])
        assert int(got[0]) == launch_uniform_row(ops, case, 1, b, t, p, k, case["fm"], case["ban"], (0, 0)), (t, p, k)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("tmax", [2, 8, 32])
def test_top_k_outside_its_range_is_clamped(ops, tmax, dtype):
    """(f) the host API refuses such values; the kernel still clamps top_k[b] into [1, 64] before any use, so an array holding 0
    and 1000 behaves as one holding 1 and 64: ids inside the rows' ranges, nothing else touched (launch_rows checks the
    sentinels)"""
    case = R.sampler_case(tmax, dtype, 100 + tmax)
    B, V = case["B"], case["V"]
    temp, top_p, _ = row_params(B)
    wild = [0 if b % 2 == 0 else 1000 for b in range(B)]
    got = launch_rows(ops, case, 1, temp, top_p, wild, case["fm"], case["ban"], (0, 0))
    want = launch_rows(ops, case, 1, temp, top_p, [1 if k == 0 else 64 for k in wild], case["fm"], case["ban"], (0, 0))
    assert torch.equal(got, want)
    lo, hi = case["lo_tab"][:, 1], case["hi_tab"][:, 1].clamp(max=V)
    assert bool(((got >= lo) & (got < hi)).all()), "an id outside the row's range"


def test_wrapper_and_entry_point_refuse_bad_arguments(ops):
    from midi_model_amd.lib import lib
    case = R.sampler_case(2, F32, 102)
    B, V = case["B"], case["V"]
    temp, top_p, top_k = row_params(B)
    dev = lambda v, ty: torch.tensor(v, dtype=ty, device="cuda")
    base = dict(logits=case["logits"].cuda(), lo=case["lo_tab"].cuda(), hi=case["hi_tab"].cuda(), ev=case["ev"].cuda(), q=case["q"].cuda(),
                out=torch.zeros(B, dtype=torch.int64, device="cuda"), fm=case["fm"].cuda(), ban=case["ban"].cuda())

    def call(t, p, k, fm=base["fm"], ban=base["ban"], span=(0, 0), max_range=case["max_range"]):
        return ops.sample_top_p_k_rows(base["logits"], fm, base["lo"], base["hi"], base["ev"], 1, base["q"], base["out"], V, t, p, k,
                                       ban, first_span=span, max_range=max_range)

    T, P, K = dev(temp, torch.float32), dev(top_p, torch.float32), dev(top_k, torch.int32)
    with pytest.raises(AssertionError, match="rows: temp must"):
        call(T.double(), P, K)
    with pytest.raises(AssertionError, match="rows: top_k must"):
        call(T, P, K.long())
    with pytest.raises(AssertionError, match="rows: top_p must"):
        call(T, P[:-1], K)
    with pytest.raises(AssertionError, match="first_mask"):
        call(T, P, K, fm=base["fm"][None].repeat(B + 1, 1))
    with pytest.raises(AssertionError, match="ban_mask"):
        call(T, P, K, ban=base["ban"].bool())
    with pytest.raises(RuntimeError, match="spans more than"):
        call(T, P, K, max_range=2049)
    # the C entry point itself: NULL arrays are MH_ERR_ARG
    from midi_model_amd.lib import MH_F32
    args = [base["logits"].data_ptr(), base["logits"].stride(0), base["fm"].data_ptr(), 0, base["ban"].data_ptr(), 0, 0, 0,
            base["lo"].data_ptr(), base["hi"].data_ptr(), 2, case["max_range"], base["ev"].data_ptr(), 1, base["q"].data_ptr(),
            base["out"].data_ptr(), 1, 0, 0, B, V, T.data_ptr(), P.data_ptr(), K.data_ptr(), 0, 0, MH_F32,
            torch.cuda.current_stream().cuda_stream]
    lib().call("mh_sample_top_p_k_rows", *args)
    torch.cuda.synchronize()
    for null_at in (21, 22, 23, 2, 4, 14):
        bad = list(args)
        bad[null_at] = 0
        with pytest.raises(RuntimeError):
            lib().call("mh_sample_top_p_k_rows", *bad)
