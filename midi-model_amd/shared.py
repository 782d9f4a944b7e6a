"""Decode over a prompt that every row of the batch shares (``MIDIModel.generate(share_prompt=True)``).

Every caller of the reference generates B continuations of ONE prompt (app.py builds ``[mid] * OUTPUT_BATCH_SIZE``;
midi_model.py:171-188 broadcasts a 2-D prompt).  The plain path treats the B rows as unrelated: B prefills, B copies of the
prompt's K/V, and every decoded event streams all B copies.  Here the prompt's K/V are cached once per layer, [H, Pmax, 64], and
the per-row cache holds only the generated suffix.  One decode attention becomes two launches:

  attn_prefix_partial        one workgroup per (head, chunk of CHUNK prefix keys) reads the chunk's K/V once and runs all B query
                             rows against it on the matrix cores; per (b, h, chunk) an unnormalised fp32 acc[64], m, l
  attn_decode_append_shared  attn_decode_append over the row's suffix cache, then the merge of the row's partials in chunk order

The two wrappers live here, not in ``ops.py`` (as mixed.py's do).
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from .lib import lib
from .ops import _p, _stream, dt

CHUNK = 256  # MH_ATTN_PREFIX_CHUNK (include/midihip.h); mh_attn_prefix_chunk() reports the library's value


class SharedPrefix(NamedTuple):
    """what ``engine.stack_decode(shared=...)`` needs: the prompt's cache (a KVState of ONE sequence; ``kvp.len`` = prompt
    length), the prompt length in device memory (int32[1], read by a captured graph; None = take ``kvp.len``) and the fp32
    partials workspace, reused by every layer"""
    kvp: object
    pre_len_dev: object
    workspace: torch.Tensor


def workspace_floats(B: int, H: int, Pmax: int) -> int:
    """acc [B, H, nch, 64] + (m, l) [B, H, nch, 2], nch = ceil(Pmax / CHUNK)"""
    return 66 * B * H * ((Pmax + CHUNK - 1) // CHUNK)


def attn_prefix_partial(qkv, cos_t, sin_t, kpre, vpre, ws, B: int, H: int, hd: int, Pmax: int, pre_len: int, pos: int,
                        scale: float, pre_len_dev=None, pos_dev=None):
    """partials of the B rotated query rows against prefix rows [0, pre_len) of kpre / vpre [H, Pmax, hd] -> ws"""
    lib().call("mh_attn_prefix_partial", _p(qkv), _p(cos_t), _p(sin_t), _p(kpre), _p(vpre), _p(ws), ws.numel(), B, H, hd, Pmax,
               pre_len, pos, scale, _p(pre_len_dev), _p(pos_dev), dt(qkv), _stream())
    return ws


def attn_decode_append_shared(qkv, cos_t, sin_t, ksuf, vsuf, ws, o, B: int, H: int, hd: int, Lsuf: int, Pmax: int, pre_len: int,
                              pos: int, scale: float, pre_len_dev=None, pos_dev=None):
    """attn_decode_append over the suffix cache [B, H, Lsuf, hd] (new row at pos - pre_len) + the merge of the partials in ws"""
    lib().call("mh_attn_decode_append_shared", _p(qkv), _p(cos_t), _p(sin_t), _p(ksuf), _p(vsuf), _p(ws), ws.numel(), _p(o), B,
               H, hd, Lsuf, Pmax, pre_len, pos, scale, _p(pre_len_dev), _p(pos_dev), dt(qkv), _stream())
    return o


def check_equal_rows(prompt) -> None:
    """share_prompt=True accepts a (L, T'), a (1, L, T') or a (B, L, T') prompt whose rows are all equal; checked on the host,
    before any launch"""
    import numpy as np
    p = np.asarray(prompt)
    if p.ndim == 3 and p.shape[0] > 1:
        differs = (p != p[:1]).reshape(p.shape[0], -1).any(axis=1)
        if differs.any():
            raise ValueError(f"share_prompt=True needs a prompt whose rows are all equal: row {int(np.argmax(differs))} differs "
                             "from row 0 (rows with different prompts take the plain path, share_prompt=False)")
