"""CPU stand-ins for the two prefix-slot entry points (ops.attn_prefix_partial_slots, ops.attn_decode_append_rows_shared), layered on
emu_fork.py in the style of emu_fork itself.  The EXACT emulation: the prefix half leaves the workspace alone and the decode half
attends, in emu_ragged's own float64 ``_attend``, to the slot's rows [0, pre_b) laid in front of the row's own cache rows
[0, row_pos[b] - pre_b] -- the same keys in the same order as a row that owns a copy of its prompt, so a sharing request equals the
same request unshared, which is what lets the host tests compare the two.  (The kernels' split into chunk partials is what
tests/test_poolshare_kernels_gpu.py checks, against ``reference`` below.)  ``install()`` is emu_fork.install() with the two patched on
top; it yields the same CALL LOG.  Test infrastructure only."""
from __future__ import annotations

import contextlib

import torch

import emu_fork
import emu_ragged
from emu_shared import rotated

CHUNK = 256


def _check(name, qkv, hd, B, G, Pmax, slot_len, row_slot, row_pos):
    if hd != 64:
        raise RuntimeError(f"{name}: head_dim {hd} unsupported (64)")
    if G < 1:
        raise RuntimeError(f"{name}: {G} slots")
    for t, n in ((slot_len, G), (row_slot, B), (row_pos, B)):
        if t is None:
            raise RuntimeError(f"{name}: a NULL array")
        assert t.dtype == torch.int32 and t.shape == (n,)
    lens = [min(max(int(x), 0), Pmax) for x in slot_len.tolist()]
    pre = [lens[g] if 0 <= g < G else 0 for g in row_slot.tolist()]
    return pre, [int(p) for p in row_pos.tolist()]


def attn_prefix_partial_slots(qkv, cos_t, sin_t, kpre, vpre, slot_len, row_slot, row_pos, ws, B, H, hd, G, Pmax, scale):
    _check("attn_prefix_partial_slots", qkv, hd, B, G, Pmax, slot_len, row_slot, row_pos)
    assert kpre.shape == (G, H, Pmax, hd) and vpre.shape == kpre.shape
    assert ws.dtype == torch.float32 and ws.numel() >= 66 * B * H * ((Pmax + CHUNK - 1) // CHUNK)
    return ws


# (the decode half needs the slot caches, which the entry point does not take: the prefix half runs right before it on the same
#  layer, so the stand-in remembers that call's)
_last_slots: list = [None, None]


def _prefix_then(fn):
    def f(qkv, cos_t, sin_t, kpre, vpre, *a, **k):
        _last_slots[:] = [kpre, vpre]
        return fn(qkv, cos_t, sin_t, kpre, vpre, *a, **k)
    return f


def attn_decode_append_rows_shared(qkv, cos_t, sin_t, ksuf, vsuf, ws, o, B, H, hd, Lsuf, G, Pmax, scale, slot_len, row_slot, row_pos):
    pre, pos = _check("attn_decode_append_rows_shared", qkv, hd, B, G, Pmax, slot_len, row_slot, row_pos)
    kpre, vpre = _last_slots
    assert kpre is not None and kpre.shape[0] == G and kpre.shape[2] == Pmax, "no prefix call of this layer came before"
    _last_slots[:] = [None, None]   # (strictly in pairs: the next layer's prefix call sets its own)
    slots = row_slot.tolist()
    for b in range(B):
        p = max(pos[b], 0)
        row = min(max(p - pre[b], 0), Lsuf - 1)
        q, k, v = rotated(qkv[b:b + 1], cos_t, sin_t, p, H, hd)
        ksuf[b, :, row] = k[0]
        vsuf[b, :, row] = v[0]
        if pre[b] == 0:
            o[b] = emu_ragged._attend(q[0], ksuf[b], vsuf[b], row + 1, scale, o.dtype)
            continue
        g = slots[b]
        kk = torch.cat([kpre[g, :, :pre[b]], ksuf[b, :, :row + 1]], 1)
        vv = torch.cat([vpre[g, :, :pre[b]], vsuf[b, :, :row + 1]], 1)
        o[b] = emu_ragged._attend(q[0], kk, vv, pre[b] + row + 1, scale, o.dtype)
    return o


def reference(qkv, cos_t, sin_t, kpre, vpre, ksuf, vsuf, H, slot_len, row_slot, row_pos, scale):
    """float64 softmax attention of every row over its slot's rows [0, pre_b), its own cache rows [0, row_pos[b] - pre_b) and the
    new key, from the values the kernels read (ksuf / vsuf BEFORE the append).  -> o64 [B, H * 64]"""
    B, hd = qkv.shape[0], 64
    G, Pmax = kpre.shape[0], kpre.shape[2]
    out = torch.zeros((B, H * hd), dtype=torch.float64)
    for b in range(B):
        g, pos = int(row_slot[b]), int(row_pos[b])
        pre = min(int(slot_len[g]), Pmax) if 0 <= g < G else 0
        q, k, v = rotated(qkv[b:b + 1], cos_t, sin_t, pos, H, hd)
        row = pos - pre
        keys = torch.cat([kpre[g, :, :pre].double() if pre else ksuf[b, :, :0].double(), ksuf[b, :, :row].double(),
                          k[0].double()[:, None]], 1)
        vals = torch.cat([vpre[g, :, :pre].double() if pre else vsuf[b, :, :0].double(), vsuf[b, :, :row].double(),
                          v[0].double()[:, None]], 1)
        s = torch.einsum("hd,hkd->hk", q[0].double() * scale, keys)
        out[b] = torch.einsum("hk,hkd->hd", torch.softmax(s, -1), vals).reshape(-1)
    return out


_NAMES = ("attn_prefix_partial_slots", "attn_decode_append_rows_shared")


@contextlib.contextmanager
def install():
    """emu_fork.install() + the two stand-ins above (logged like every other op); yields the call log"""
    import midi_model_amd.ops as real
    with emu_fork.install() as log:
        _last_slots[:] = [None, None]
        try:
            setattr(real, _NAMES[0], emu_ragged._logged(_NAMES[0], _prefix_then(attn_prefix_partial_slots), log))
            setattr(real, _NAMES[1], emu_ragged._logged(_NAMES[1], attn_decode_append_rows_shared, log))
            yield log
        finally:
            for n in _NAMES:
                delattr(real, n)
