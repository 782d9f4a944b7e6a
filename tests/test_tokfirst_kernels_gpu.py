"""The kernels of the per-vocabulary first token-level block (midi_model_amd/tokfirst.py) at their boundaries:
  * row-indirect token attention (mh_tokattn_fwd_rows / mh_tokattn_bwd_rows) against the dense kernels on the materialised
    rows, bit for bit;
  * the wide segment sum (mh_embed_segment_sum) and its two-term bf16 form (mh_embed_split_hi_lo) against fp64;
  * the folded norm's backward on table rows (mh_embed_table_norm_bwd) against the fp64 formula.
"""
import pytest
import torch

from midi_model_amd import engine, ops, tokfirst

pytestmark = pytest.mark.gpu

DEV = "cuda"


def bits(t):
    return t.contiguous().view(torch.int16)


def test_row_indirect_token_attention_equals_dense_bit_for_bit():
    """N = 37 sequences x H = 4 heads: 148 (sequence, head) pairs, not a multiple of the 4 waves of a workgroup, 37 workgroups;
    table of 41 rows behind 3 unused rows (tab0 = 40 > N); ids hold the pad id 0, V - 1 and repeats inside a sequence."""
    N, H, T, V = 37, 4, 8, 41
    D, tab0 = H * 256, 40
    g = torch.Generator().manual_seed(11)
    zc = (torch.randn((tab0 + V, 3 * D), generator=g) * 0.7).to(torch.bfloat16).to(DEV)
    tokm = torch.randint(0, V, (N, T), generator=g)
    tokm[0, :7] = torch.tensor([0, V - 1, 5, 5, 0, V - 1, 5])
    tokm[36, :7] = V - 1
    tokm[17, :7] = 0
    tokm = tokm.to(DEV)
    ids = tokm[:, : T - 1]                                   # a column slice: row stride 8
    rs_c = (0.5 + torch.rand(tab0 + V, generator=g)).to(DEV)
    rows = torch.cat([torch.arange(N, device=DEV)[:, None], tab0 + ids], dim=1).reshape(-1)   # row of zc per (n, p)
    qkv = zc[rows].contiguous()
    rs = rs_c[rows].contiguous()
    dout = torch.randn((N * T, D), generator=g).to(torch.bfloat16).to(DEV)
    rope = engine.RopeTable(256, 10000.0, DEV, T)
    scale = 256 ** -0.5

    o_ref = torch.empty((N * T, D), dtype=torch.bfloat16, device=DEV)
    ops.tokattn_fwd(qkv, o_ref, N, T, H, scale, rope.cos, rope.sin)
    o = torch.full_like(o_ref, float("nan"))
    tokfirst.tokattn_fwd_rows(zc, ids, tab0, V, o, N, H, scale, rope.cos, rope.sin)
    assert torch.equal(bits(o), bits(o_ref))

    dz_ref = torch.empty((N * T, 3 * D), dtype=torch.bfloat16, device=DEV)
    ops.tokattn_bwd(qkv, dout, dz_ref, N, T, H, scale, rope.cos, rope.sin, rowscale=rs)
    assert float(dz_ref.float().abs().max()) > 0
    # every row in place
    dz = torch.full_like(dz_ref, float("nan"))
    tokfirst.tokattn_bwd_rows(zc, ids, tab0, V, dout, dz, None, rs_c, N, H, scale, rope.cos, rope.sin)
    assert torch.equal(bits(dz), bits(dz_ref))
    # position 0's rows to the compact buffer, rows 8n of dz untouched
    dz = torch.full_like(dz_ref, float("nan"))
    dzh = torch.full((N, 3 * D), float("nan"), dtype=torch.bfloat16, device=DEV)
    tokfirst.tokattn_bwd_rows(zc, ids, tab0, V, dout, dz, dzh, rs_c, N, H, scale, rope.cos, rope.sin)
    d3 = dz.view(N, T, 3 * D)
    assert torch.equal(bits(d3[:, 1:]), bits(dz_ref.view(N, T, 3 * D)[:, 1:]))
    assert torch.equal(bits(dzh), bits(dz_ref.view(N, T, 3 * D)[:, 0]))
    assert torch.isnan(d3[:, 0].float()).all()
    # without a row scale as well
    ops.tokattn_bwd(qkv, dout, dz_ref, N, T, H, scale, rope.cos, rope.sin)
    tokfirst.tokattn_bwd_rows(zc, ids, tab0, V, dout, dz, None, None, N, H, scale, rope.cos, rope.sin)
    assert torch.equal(bits(dz), bits(dz_ref))


@pytest.fixture(scope="module")
def occurrences():
    """2,800 occurrences over V = 700 ids: id 9 with 1,500 (> SEG_OWN = 1024: the atomic path), the pad id 0 with 3, ids with 1-5
    each until the total is reached, the rest absent; shuffled."""
    V, total = 700, 2800
    g = torch.Generator().manual_seed(5)
    counts = torch.zeros(V, dtype=torch.long)
    counts[9] = 1500
    counts[0] = 3
    left = total - 1503
    for v in torch.randperm(V, generator=g).tolist():
        if v in (0, 9) or left == 0:
            continue
        c = min(left, int(torch.randint(1, 6, (1,), generator=g)))
        counts[v] = c
        left -= c
    assert left == 0 and int((counts == 0).sum()) > 10 and int(counts.sum()) == total
    tokv = torch.repeat_interleave(torch.arange(V), counts)
    tokv = tokv[torch.randperm(total, generator=g)]
    return V, tokv, counts


@pytest.mark.parametrize("width", [768, 3072])
def test_wide_segment_sum_against_fp64(occurrences, width):
    V, tokv, counts = occurrences
    n = tokv.numel()
    g = torch.Generator().manual_seed(width)
    ld = width + 64                                          # rows wider than what is summed
    x = torch.randn((n, ld), generator=g).to(torch.bfloat16)
    ref = torch.zeros((V, width), dtype=torch.float64).index_add_(0, tokv, x[:, :width].double())
    mag = torch.zeros((V, width), dtype=torch.float64).index_add_(0, tokv, x[:, :width].double().abs())
    xd, tokd = x.to(DEV), tokv.to(DEV)
    src, seg = ops.token_segments(tokd, V)
    S = torch.zeros((V, width), dtype=torch.float32, device=DEV)
    tokfirst.segment_sum(src, seg, xd[:, :width], S)
    err = (S.double().cpu() - ref).abs()
    bound = counts.double()[:, None] * 2.0 ** -23 * mag      # a plain fp32 summation bound
    worst = float((err - bound).max())
    print(f"segment sum width {width}: max |err| {float(err.max()):.3e}, max (err - bound) {worst:.3e}")
    assert (err <= bound).all()
    assert float(S[0].abs().max()) > 0, "the pad id is part of this sum"
    assert float(S[counts.to(DEV) == 0].abs().max()) == 0
    hi = torch.empty((V, width), dtype=torch.bfloat16, device=DEV)
    lo = torch.empty_like(hi)
    tokfirst.split_hi_lo(S, hi, lo)
    back = hi.double() + lo.double()
    assert ((back - S.double()).abs() <= 2.0 ** -16 * S.double().abs()).all()
    assert torch.equal(hi, S.to(torch.bfloat16))


@pytest.mark.parametrize("D", [256, 1024])
def test_table_norm_backward_against_fp64(D):
    """acc32[v] += T_v - e_v (rstd_v^2 / D) rowdot(T_v, e_v), T = t_hi + t_lo, every row but the pad id's.  Bound, with u = 2^-24
    (fp32 unit roundoff; the bf16 inputs are exact in fp32): T carries 1 rounding, the dot product D products and D additions
    in some order (<= (D + 1) u sum|T_k e_k| on top of T's), cf = r r dot / D three more, and each output element e cf, T - e cf
    and acc + (.) one each -- |err| <= 3 u (|acc| + |T| + |e cf|) + |e| (r^2 / D) (D + 6) u sum|T_k e_k|; asserted at twice
    that to leave room for second-order terms."""
    V, pad = 41, 0
    g = torch.Generator().manual_seed(D)
    t_hi = torch.randn((V, D), generator=g).to(torch.bfloat16)
    t_lo = (torch.randn((V, D), generator=g) * 2.0 ** -9).to(torch.bfloat16)
    e = torch.randn((V, D), generator=g).to(torch.bfloat16)
    rstd = (0.5 + torch.rand(V, generator=g)).float()
    acc0 = torch.randn((V, D), generator=g).float()
    Tt = t_hi.double() + t_lo.double()
    dotabs = (Tt * e.double()).abs().sum(-1, keepdim=True)
    cf = rstd.double()[:, None] ** 2 * (Tt * e.double()).sum(-1, keepdim=True) / D
    ref = acc0.double() + Tt - e.double() * cf
    ref[pad] = acc0[pad].double()
    u = 2.0 ** -24
    bound = 3 * u * (acc0.double().abs() + Tt.abs() + (e.double() * cf).abs()) \
        + e.double().abs() * (rstd.double()[:, None] ** 2 / D) * (D + 6) * u * dotabs
    acc = acc0.to(DEV).clone()
    tokfirst.table_norm_bwd(t_hi.to(DEV), t_lo.to(DEV), e.to(DEV), rstd.to(DEV), acc, pad)
    err = (acc.double().cpu() - ref).abs()
    print(f"table norm backward D {D}: max |err| {float(err.max()):.3e}, max err / bound {float((err / bound)[1:].max()):.3f}")
    assert torch.equal(acc[pad].cpu(), acc0[pad])
    assert (err <= 2 * bound).all()


def test_fixed_order_segment_sum(occurrences):
    """tokfirst.occurrence_lists + segment_sum_fixed_order (the form the training step uses: no segment longer than SEG_OWN
    reaches the kernel, an id's pieces are added in ascending order): the fp32 summation bound against fp64, the lists agree with
    mh_token_segments up to the order inside an id, and a repeat gives the same bits."""
    V, tokv, counts = occurrences
    N, C, T, width = 400, 7, 8, 3072
    ids = tokv.view(N, C).to(DEV)
    g = torch.Generator().manual_seed(3)
    x = torch.randn((N * T, width), generator=g).to(torch.bfloat16)
    rows = (torch.arange(N)[:, None] * T + torch.arange(C)[None, :] + 1).reshape(-1)
    ref = torch.zeros((V, width), dtype=torch.float64).index_add_(0, tokv, x[rows].double())
    mag = torch.zeros((V, width), dtype=torch.float64).index_add_(0, tokv, x[rows].double().abs())
    src, seg, vseg, vstart = tokfirst.occurrence_lists(ids, V, T, 1)
    src_k, seg_k = ops.token_segments(ids, V, row_mul=T, col_mul=1, add=1)
    assert torch.equal(seg, seg_k)
    assert int((vseg[1:] - vseg[:-1]).max()) <= tokfirst.SEG_OWN and int(vseg[-1]) == N * C
    assert int(vstart[10] - vstart[9]) == 2, "1,500 occurrences are two pieces"
    for v in (0, 9, int(torch.nonzero(counts == 5)[0])):
        a, b = int(seg[v]), int(seg[v + 1])
        assert src[a:b].tolist() == sorted(src_k[a:b].tolist())
    xd = x.to(DEV)
    S = torch.full((V, width), float("nan"), dtype=torch.float32, device=DEV)
    tokfirst.segment_sum_fixed_order(src, vseg, vstart, xd, S)
    err = (S.double().cpu() - ref).abs()
    assert (err <= counts.double()[:, None] * 2.0 ** -23 * mag).all()
    S2 = torch.empty_like(S)
    tokfirst.segment_sum_fixed_order(src, vseg, vstart, xd, S2)
    assert torch.equal(S, S2)
