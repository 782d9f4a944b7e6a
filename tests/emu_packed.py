"""CPU stand-ins for the packed-batch entry points (mh_rope_pos, mh_attn_fwd_seqs, mh_attn_bwd_seqs), in the style of emu_shared.py:
float64 restatements written from the definitions -- every sequence on its own, causal within itself, positions restarting at its
first row -- that do not go through the uniform stand-ins of emu_ops.py.  ``install()`` puts them over ``emu_ops.install()``, so a
whole training step on a PackedBatch runs on the CPU.  Results are rounded ONCE, to the output's dtype."""
from __future__ import annotations

import contextlib

import torch

import emu_ops


def _starts(plan):
    seq_start = plan.host_views()[0].tolist()
    return list(zip(seq_start[:-1], seq_start[1:]))


def rope_pos_(qkv, cos_t, sin_t, pos, H, hd, direction=1):
    M, D = qkv.shape[0], H * hd
    pos = pos.long().cpu()
    c = cos_t.cpu()[pos].to(qkv.dtype).double()[:, None, :]   # (the tables are rounded to the activation dtype before use)
    s = direction * sin_t.cpu()[pos].to(qkv.dtype).double()[:, None, :]
    for part in range(2):
        v = qkv[:, part * D:(part + 1) * D].double().view(M, H, hd)
        x1, x2 = v[..., : hd // 2], v[..., hd // 2:]
        qkv[:, part * D:(part + 1) * D] = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1).reshape(M, D).to(qkv.dtype)
    return qkv


def _seq_qkv(qkv, a, b, H):
    D = H * 64
    return tuple(qkv[a:b, i * D:(i + 1) * D].double().view(b - a, H, 64).transpose(0, 1) for i in range(3))  # [H, S, 64]


def _scores(q, k, scale):
    S = q.shape[-2]
    s = (q @ k.transpose(-1, -2)) * scale
    return s.masked_fill(torch.triu(torch.ones(S, S, dtype=torch.bool), 1), float("-inf"))


def attn_fwd_seqs(qkv, o, lse, plan, H, scale):
    M = plan.M
    lse_v = lse.view(-1)[:H * M].view(H, M)
    for a, b in _starts(plan):
        q, k, v = _seq_qkv(qkv, a, b, H)
        s = _scores(q, k, scale)
        o[a:b] = (torch.softmax(s, -1) @ v).transpose(0, 1).reshape(b - a, H * 64).to(o.dtype)
        lse_v[:, a:b] = torch.logsumexp(s, -1).to(lse.dtype)
    return o


def attn_bwd_seqs(qkv, o, dout, lse, dqkv, plan, H, scale, cos_t=None, sin_t=None, rowscale=None):
    D = H * 64
    for a, b in _starts(plan):
        q, k, v = _seq_qkv(qkv, a, b, H)
        do = dout[a:b].double().view(b - a, H, 64).transpose(0, 1)
        p = torch.softmax(_scores(q, k, scale), -1)
        dv = p.transpose(-1, -2) @ do
        dp = do @ v.transpose(-1, -2)
        ds = p * (dp - (p * dp).sum(-1, keepdim=True)) * scale
        for i, t in enumerate((ds @ k, ds.transpose(-1, -2) @ q, dv)):
            t = t.transpose(0, 1).reshape(b - a, D)
            if rowscale is not None:  # (the kernels scale the fp32 accumulators before the store's rounding)
                t = t * rowscale[a:b].double().cpu()[:, None]
            dqkv[a:b, i * D:(i + 1) * D] = t.to(dqkv.dtype)
    if cos_t is not None:  # (the rotation back works on the stored gradient, as mh_rope(dir = -1) would)
        rope_pos_(dqkv, cos_t, sin_t, plan.host_views()[1], H, 64, -1)
    return dqkv


_NAMES = ("rope_pos_", "attn_fwd_seqs", "attn_bwd_seqs")


@contextlib.contextmanager
def install():
    """emu_ops.install() plus the three packed entry points (attn_seq_plan is host code and stays the real one)"""
    import midi_model_amd.ops as real
    with emu_ops.install():
        try:
            for n in _NAMES:
                setattr(real, n, globals()[n])
            yield
        finally:
            for n in _NAMES:
                delattr(real, n)


@contextlib.contextmanager
def float64_arithmetic():
    """The emulated step entirely in float64 (for models moved ``.to(torch.float64)``): the stand-ins of emu_ops.py compute on
    ``x.float()`` and the step keeps its statistics, losses and accumulators in explicit float32 buffers, so inside this block
    ``Tensor.float()`` widens to float64 and every float32 buffer the engine / the step allocates becomes a float64 one.  Two
    schedules that differ only in the ORDER of sums over rows (padded against packed) then agree to float64 rounding instead of
    float32's.  Test-only; nothing of the package is changed outside the block."""
    from midi_model_amd import engine
    saved = (torch.Tensor.float, torch.empty, torch.zeros, engine._empty)

    def widen(fn):
        def f(*a, **k):
            if k.get("dtype") is torch.float32:
                k["dtype"] = torch.float64
            return fn(*a, **k)
        return f

    def _empty(shape, like, dtype=None):
        return saved[1](shape, dtype=torch.float64 if dtype in (None, torch.float32) else dtype, device=like.device)

    try:
        torch.Tensor.float = lambda self, *a, **k: self.double()
        torch.empty, torch.zeros, engine._empty = widen(saved[1]), widen(saved[2]), _empty
        yield
    finally:
        torch.Tensor.float, torch.empty, torch.zeros, engine._empty = saved
