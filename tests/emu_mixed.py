"""CPU stand-ins for the two wrappers of ``midi_model_amd.mixed`` (mh_grad_fold_f32, mh_adamw_master), in the style of
tests/emu_ops.py, and ``install()``: emu_ops.install() with ``midi_model_amd.mixed`` patched on top, so that the mixed-precision
host logic of train.py runs on CPU tensors.  Test infrastructure only."""
from __future__ import annotations

import contextlib

import torch

import emu_ops


def grad_fold(src, dst, accumulate):
    assert dst.dtype == torch.float32 and src.numel() == dst.numel()
    if accumulate:
        dst.add_(src.float())
    else:
        dst.copy_(src.float())


def adamw_master(p32, p_lo, g32, m, v, lr, b1, b2, eps, wd, bc1, bc2, coef_dev):
    """the kernel's operations in its order, each an fp32 operation (the scalars are formed in fp32 as the kernel forms them)"""
    f = lambda x: torch.tensor(x, dtype=torch.float32)
    coef = coef_dev[0] if coef_dev is not None else f(1.0)
    step, sq2, decay = f(lr) / f(bc1), f(bc2).sqrt(), f(1.0) - f(lr) * f(wd)
    omb1, omb2 = f(1.0) - f(b1), f(1.0) - f(b2)
    g = g32 * coef
    p = p32 * decay
    me = m + (g - m) * omb1
    ve = v * f(b2) + omb2 * g * g
    den = ve.sqrt() / sq2 + f(eps)
    p = p - step * (me / den)
    p32.copy_(p)
    m.copy_(me)
    v.copy_(ve)
    p_lo.copy_(p.to(p_lo.dtype))


_NAMES = ("grad_fold", "adamw_master")


@contextlib.contextmanager
def install():
    """emu_ops.install() + the stand-ins above in place of midi_model_amd.mixed's wrappers"""
    import midi_model_amd.mixed as real
    saved = {n: getattr(real, n) for n in _NAMES}
    with emu_ops.install():
        try:
            for n in _NAMES:
                setattr(real, n, globals()[n])
            yield
        finally:
            for n, fn in saved.items():
                setattr(real, n, fn)
