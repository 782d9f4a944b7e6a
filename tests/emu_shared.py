"""CPU stand-ins for the two wrappers of ``midi_model_amd.shared`` (mh_attn_prefix_partial, mh_attn_decode_append_shared) in
float64, with the argument checks of the entry points, and ``install()``: emu_ops.install() with ``midi_model_amd.shared``
patched on top (the way tests/emu_mixed.py does it), so that the shared-prompt host logic of engine.py / decode.py / model.py
runs on CPU tensors.  Also the float64 reference of the GPU kernel tests.  Test infrastructure only."""
from __future__ import annotations

import contextlib

import torch

import emu_ops

CHUNK = 256


def _value(host, dev):
    return int(dev.item()) if dev is not None else int(host)


def _check(name, hd, Pmax, pre_len, pos, pre_len_dev, pos_dev, Lsuf=None):
    if hd != 64:
        raise RuntimeError(f"{name}: head_dim {hd} unsupported (64)")
    if pre_len_dev is None and not 1 <= pre_len <= Pmax:
        raise RuntimeError(f"{name}: bad args pre_len={pre_len} Pmax={Pmax}")
    if pre_len_dev is None and pos_dev is None:
        if pos < pre_len or (Lsuf is not None and pos - pre_len >= Lsuf):
            raise RuntimeError(f"{name}: bad args pos={pos} pre_len={pre_len} Lsuf={Lsuf}")


def rotated(qkv, cos_t, sin_t, pos, H, hd):
    """(q, k, v) [B, H, hd] of position ``pos`` as mh_kv_append leaves them: cos / sin rounded to the dtype, results rounded"""
    T = qkv.dtype
    B, D, half = qkv.shape[0], H * hd, hd // 2
    c, s = cos_t[pos].to(T).float(), sin_t[pos].to(T).float()
    out = []
    for j in range(2):
        x = qkv[:, j * D:(j + 1) * D].float().view(B, H, hd)
        x1, x2 = x[..., :half], x[..., half:]
        out.append(torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1).to(T))
    out.append(qkv[:, 2 * D:].reshape(B, H, hd).clone())
    return out


def attn_prefix_partial(qkv, cos_t, sin_t, kpre, vpre, ws, B, H, hd, Pmax, pre_len, pos, scale, pre_len_dev=None, pos_dev=None):
    _check("attn_prefix_partial", hd, Pmax, pre_len, pos, pre_len_dev, pos_dev)
    pre, pos = min(_value(pre_len, pre_len_dev), Pmax), _value(pos, pos_dev)
    nch = (Pmax + CHUNK - 1) // CHUNK
    assert ws.numel() >= 66 * B * H * nch and ws.dtype == torch.float32
    kpre, vpre = kpre.reshape(H, Pmax, hd), vpre.reshape(H, Pmax, hd)
    q = rotated(qkv, cos_t, sin_t, pos, H, hd)[0].double() * scale
    acc = ws[: B * H * nch * 64].view(B, H, nch, 64)
    ml = ws[B * H * nch * 64: B * H * nch * 66].view(B, H, nch, 2)
    for c in range((pre + CHUNK - 1) // CHUNK):
        lo, hi = c * CHUNK, min(pre, (c + 1) * CHUNK)
        s = torch.einsum("bhd,hkd->bhk", q, kpre[:, lo:hi].double())
        m = s.max(-1).values
        p = (s - m[..., None]).exp()
        acc[:, :, c] = torch.einsum("bhk,hkd->bhd", p, vpre[:, lo:hi].double()).float()
        ml[:, :, c, 0] = m.float()
        ml[:, :, c, 1] = p.sum(-1).float()
    return ws


def attn_decode_append_shared(qkv, cos_t, sin_t, ksuf, vsuf, ws, o, B, H, hd, Lsuf, Pmax, pre_len, pos, scale, pre_len_dev=None,
                              pos_dev=None):
    _check("attn_decode_append_shared", hd, Pmax, pre_len, pos, pre_len_dev, pos_dev, Lsuf)
    pre, pos = _value(pre_len, pre_len_dev), _value(pos, pos_dev)
    row = min(max(pos - pre, 0), Lsuf - 1)
    nch = (Pmax + CHUNK - 1) // CHUNK
    q, k, v = rotated(qkv, cos_t, sin_t, pos, H, hd)
    ksuf[:, :, row] = k
    vsuf[:, :, row] = v
    q = q.double() * scale
    s = torch.einsum("bhd,bhkd->bhk", q, ksuf[:, :, : row + 1].double())
    acc = ws[: B * H * nch * 64].view(B, H, nch, 64).double()
    ml = ws[B * H * nch * 64: B * H * nch * 66].view(B, H, nch, 2).double()
    n = min((pre + CHUNK - 1) // CHUNK, nch)
    m = torch.maximum(s.max(-1).values, ml[:, :, :n, 0].max(-1).values) if n else s.max(-1).values
    p = (s - m[..., None]).exp()
    num = torch.einsum("bhk,bhkd->bhd", p, vsuf[:, :, : row + 1].double())
    den = p.sum(-1)
    for c in range(n):
        f = (ml[:, :, c, 0] - m).exp()
        num = num + acc[:, :, c] * f[..., None]
        den = den + ml[:, :, c, 1] * f
    o.copy_((num / den[..., None]).reshape(B, H * hd).to(o.dtype))
    return o


def reference(qkv, cos_t, sin_t, kpre, vpre, ksuf, vsuf, B, H, pre_len, pos, scale):
    """float64 attention over the exact values read: prefix rows [0, pre_len), suffix rows [0, pos - pre_len) and the new key
    concatenated per (b, h), the rotated q of kv_append.  -> (o64 [B, H*64], q, k_new, v_new, scores [B, H, n])"""
    hd = 64
    q, k, v = rotated(qkv, cos_t, sin_t, pos, H, hd)
    row = pos - pre_len
    keys = torch.cat([kpre.reshape(H, -1, hd)[None, :, :pre_len].expand(B, -1, -1, -1).double(), ksuf[:, :, :row].double(),
                      k.double()[:, :, None]], 2)
    vals = torch.cat([vpre.reshape(H, -1, hd)[None, :, :pre_len].expand(B, -1, -1, -1).double(), vsuf[:, :, :row].double(),
                      v.double()[:, :, None]], 2)
    s = torch.einsum("bhd,bhkd->bhk", q.double() * scale, keys)
    o = torch.einsum("bhk,bhkd->bhd", torch.softmax(s, -1), vals)
    return o.reshape(B, H * hd), q, k, v, s


_NAMES = ("attn_prefix_partial", "attn_decode_append_shared")


@contextlib.contextmanager
def install():
    """emu_ops.install() + the stand-ins above in place of midi_model_amd.shared's wrappers"""
    import midi_model_amd.shared as real
    saved = {n: getattr(real, n) for n in _NAMES}
    with emu_ops.install():
        try:
            for n in _NAMES:
                setattr(real, n, globals()[n])
            yield
        finally:
            for n, fn in saved.items():
                setattr(real, n, fn)
