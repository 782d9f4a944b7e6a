"""The first block of the token-level stack, per vocabulary entry instead of per row (training, folded norms).

The token-level stack runs over R = N * 8 rows of which row 8n is the event's hidden state and rows 8n+1 .. 8n+7 are
``embed[y[n, p-1]]`` (midi_model.py forward_token): in the FIRST block seven of every eight inputs of the RMSNorm and of the
q|k|v projection are one of the V rows of the embedding table, and RoPE is applied inside the attention kernel, so the
projection of such a row depends on its token id alone.  engine.tok_first_forward / tok_first_backward project the table once
and sum the output gradient per id before the dgrad, the weight gradient and the norm's backward; this module holds the
C-ABI wrappers those two need (row-indirect token attention, the wide segment sum, the table's norm backward) and the one
question whether that form runs.
"""
from __future__ import annotations

import os
from typing import NamedTuple, Optional

import torch

from .lib import lib
from .ops import _p, _rowmajor, _stream, dt

TN = 8  # tokens per sequence the row-indirect attention kernels are built for


class TokFirst(NamedTuple):
    """the inputs of the token-level stack before they are laid out as rows"""
    hidden: torch.Tensor    # [N, D] event hidden states (position 0 of every sequence)
    ids: torch.Tensor       # [N, >= 7] int64, unit column stride: the token ids of positions 1..7
    table: torch.Tensor     # [V, D] the token-level embedding table
    pad_id: int


def table_first_ok(spec, first: Optional[TokFirst], slen: int) -> bool:
    """whether the first block of stack ``spec`` takes the per-vocabulary form in the folded training step: device tensors (the
    CPU stand-in runs of the tests keep the dense schedule), bf16, octets, and MH_TOK_TABLE != 0 in the environment"""
    return (first is not None and spec.kind == "token" and slen == TN and first.hidden.is_cuda
            and first.hidden.dtype == torch.bfloat16 and first.table.shape[0] >= 4 and os.environ.get("MH_TOK_TABLE", "1") != "0")


def tokattn_fwd_rows(zc, ids, tab0: int, V: int, o, N: int, H: int, scale: float, cos_t, sin_t):
    """tokattn_fwd at T = 8 on rows taken through the indirection: position 0 of sequence n = row n of ``zc``, position p >= 1 =
    row tab0 + ids[n, p - 1]; o [N * 8, D] as the dense kernel writes it"""
    assert ids.dtype == torch.int64 and ids.stride(1) == 1 and ids.shape[1] >= TN - 1 and zc.shape[0] >= tab0 + V
    lib().call("mh_tokattn_fwd_rows", _p(zc), _p(ids), ids.stride(0), tab0, V, _p(o), N, H, scale, _p(cos_t), _p(sin_t), dt(zc),
               _stream())
    return o


def tokattn_bwd_rows(zc, ids, tab0: int, V: int, dout, dz, dz_hid, rowscale, N: int, H: int, scale: float, cos_t, sin_t):
    """tokattn_bwd at T = 8 through the same indirection (``rowscale`` indexed like the rows of zc): dz [N * 8, 3D] as the dense
    kernel writes it, except that position 0's rows go to ``dz_hid`` [N, 3D] when that is given"""
    assert ids.dtype == torch.int64 and ids.stride(1) == 1 and ids.shape[1] >= TN - 1 and zc.shape[0] >= tab0 + V
    assert dz.is_contiguous() and (dz_hid is None or dz_hid.is_contiguous())
    assert rowscale is None or (rowscale.dtype == torch.float32 and rowscale.is_contiguous() and rowscale.numel() >= tab0 + V)
    lib().call("mh_tokattn_bwd_rows", _p(zc), _p(ids), ids.stride(0), tab0, V, _p(dout), _p(dz), _p(dz_hid), _p(rowscale), N, H, scale,
               _p(cos_t), _p(sin_t), dt(zc), _stream())
    return dz


def segment_sum(src_rows, seg_start, rows, out_f32):
    """out_f32[v] += the rows ``rows[src_rows[i]]``, i in [seg_start[v], seg_start[v + 1]) -- every id, the pad id included"""
    V, D = out_f32.shape
    assert src_rows.dtype == torch.int64 and seg_start.dtype == torch.int64 and seg_start.numel() == V + 1 and src_rows.is_contiguous()
    assert out_f32.dtype == torch.float32 and rows.shape[1] == D
    lib().call("mh_embed_segment_sum", _p(src_rows), _p(seg_start), _p(rows), _rowmajor(rows), _p(out_f32), _rowmajor(out_f32), V, D,
               src_rows.numel(), dt(rows), _stream())
    return out_f32


SEG_OWN = 1024  # the longest segment mh_embed_segment_sum adds with plain loads and stores (elementwise.hip); longer ones meet in atomics


def occurrence_lists(ids: torch.Tensor, V: int, row_mul: int, add: int):
    """The occurrence lists of the id matrix ``ids`` [N, C] in an order that does not vary from run to run (index arithmetic only):
    occurrence (n, j) reads row n * row_mul + j + add.  -> (src, seg, vseg, vstart):
      src [N * C]     the rows grouped by id, ascending inside an id (ops.token_segments leaves that order to its atomics);
      seg [V + 1]     seg[v] = occurrences with id < v, as ops.token_segments gives it;
      vseg [Vb + 1]   the same list cut into pieces of at most SEG_OWN occurrences, every id at least one piece, so that
                      segment_sum(src, vseg, ...) never takes the atomic path (Vb = V + ceil(N C / SEG_OWN) bounds the pieces);
      vstart [V + 1]  vstart[v] = the first piece of id v: segment_sum(arange(Vb), vstart, pieces, ...) adds an id's pieces
                      in ascending order.
    A sum made this way is the same bits every time -- it feeds weight gradients, which the data-parallel tests compare exactly."""
    N, C = ids.shape
    dev = ids.device
    R = N * row_mul
    rows = torch.arange(N, device=dev)[:, None] * row_mul + torch.arange(C, device=dev)[None, :] + add
    key, _ = torch.sort((ids * R + rows).reshape(-1))
    src = key % R
    seg = torch.searchsorted(key, torch.arange(V + 1, device=dev) * R)
    n = N * C
    Vb = V + (n + SEG_OWN - 1) // SEG_OWN
    pieces = torch.clamp((seg[1:] - seg[:-1] + SEG_OWN - 1) // SEG_OWN, min=1)
    vstart = torch.zeros(V + 1, dtype=torch.int64, device=dev)
    vstart[1:] = torch.cumsum(pieces, 0)
    j = torch.arange(Vb + 1, device=dev)
    v = torch.clamp(torch.searchsorted(vstart, j, right=True) - 1, max=V - 1)
    vseg = torch.minimum(seg[v] + (j - vstart[v]) * SEG_OWN, seg[v + 1])
    return src.contiguous(), seg.contiguous(), vseg.contiguous(), vstart


def segment_sum_fixed_order(src, vseg, vstart, rows, out_f32):
    """out_f32[v] = the sum of an id's rows in an order fixed by occurrence_lists: pieces first, then the pieces of an id"""
    V, D = out_f32.shape
    Vb = vseg.numel() - 1
    part = torch.zeros((Vb, D), dtype=torch.float32, device=rows.device)
    segment_sum(src, vseg, rows, part)
    out_f32.zero_()
    return segment_sum(torch.arange(Vb, device=rows.device), vstart, part, out_f32)


def split_hi_lo(s_f32, hi, lo):
    """hi = round(s), lo = round(s - hi) in the dtype of hi / lo (contiguous, same shape as s)"""
    assert s_f32.dtype == torch.float32 and s_f32.is_contiguous() and hi.is_contiguous() and lo.is_contiguous()
    assert hi.shape == s_f32.shape == lo.shape and hi.dtype == lo.dtype
    lib().call("mh_embed_split_hi_lo", _p(s_f32), _p(hi), _p(lo), s_f32.numel(), dt(hi), _stream())


def table_norm_bwd(t_hi, t_lo, table, rstd, acc32, pad_id: int):
    """acc32[v] += T_v - e_v (rstd_v^2 / D) rowdot(T_v, e_v) with T = t_hi + t_lo, for every table row but ``pad_id``"""
    V, D = table.shape
    assert t_hi.shape == t_lo.shape == (V, D) and acc32.shape == (V, D) and acc32.dtype == torch.float32 and rstd.shape == (V,)
    assert t_hi.is_contiguous() and t_lo.is_contiguous() and table.is_contiguous() and acc32.is_contiguous() and rstd.is_contiguous()
    lib().call("mh_embed_table_norm_bwd", _p(t_hi), _p(t_lo), _p(table), _p(rstd), _p(acc32), V, D, pad_id, dt(table), _stream())
    return acc32
