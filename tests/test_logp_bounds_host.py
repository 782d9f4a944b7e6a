"""The bound of the sampler's log-probability output (tests/ref_logp.py) on the CPU: it accepts the fp32 restatement of the
kernel's operation order on every row kind, size and choice of id, and it rejects each named wrong kernel by at least ten bounds on
inputs chosen to show that mistake.  No device, no emulation."""
import math

import pytest
import torch

import ref_logp as rl


@pytest.mark.parametrize("V", rl.SIZES)
def test_bound_accepts_the_restatement(V):
    worst = 0.0
    for kind in rl.ROW_KINDS:
        z = rl.make_row(kind, V, seed=1)
        for how in rl.CHOICES:
            c = rl.choose(z, how)
            got = rl.kernel_order(z, c, V).double()
            err = float((got - rl.logp64(z, c, V)).abs())
            frac = err / float(rl.bound(z, c, V))
            worst = max(worst, frac)
            assert frac < 1.0, (kind, V, how, err, float(rl.bound(z, c, V)))
    print(f"V={V}: worst error {worst:.2f} of the bound")


def test_restatement_in_float64_is_the_definition():
    """with its flags at their defaults and float64 arithmetic the restatement IS logp64 (so a flag is the only thing a wrong kernel
    differs by)"""
    for V in rl.SIZES:
        z = rl.make_row("gauss3", V, seed=2)
        c = rl.choose(z, "last")
        assert abs(float(rl.kernel_order(z, c, V, dtype=torch.float64) - rl.logp64(z, c, V))) < 1e-12


def _far(name, z, c, V, ctx):
    ref = rl.logp64(z, c, V)
    err = float((rl.WRONG[name](z, c, V, ctx) - ref).abs())
    b = float(rl.bound(z, c, V))
    assert err >= 10 * b, (name, err, b)
    # ... while the restatement itself stays inside on the same input
    assert float((rl.kernel_order(z, c, V).double() - ref).abs()) < b, name


def test_bound_rejects_the_named_wrong_kernels():
    V, ldl = 3406, 3408
    z = torch.full((ldl,), float("nan"))
    z[:V] = rl.make_row("gauss3", V, seed=3)
    mask = torch.zeros(V, dtype=torch.bool)
    mask[100:228] = True
    c = 100 + int(z[100:228].argmax())
    ctx = {"mask": mask, "temp": 0.7}
    _far("lse_candidates", z, c, V, ctx)
    _far("stats_on_temp", z, c, V, ctx)
    _far("temp_distribution", z, c, V, ctx)
    away = 100 + int(z[100:228].argmin())  # (an id away from the row's argmax)
    _far("argmax_logit", z, away, V, ctx)
    # padding filled with large values
    zp = z.clone()
    zp[V:] = 40.0
    _far("padding_included", zp, c, V, ctx)
    # the second batch of 3584 ids carries the mass
    for V2 in (3585, 7169):
        z2 = rl.make_row("gauss3", V2, seed=4)
        z2[3584:] += 12.0
        z2 = z2.bfloat16().float()
        _far("second_batch_dropped", z2, 5, V2, ctx)
    # ascending maxima across batches
    z3 = rl.make_row("gauss3", 7169, seed=5)
    z3[3584:] += 20.0
    z3[7168] += 20.0
    z3 = z3.bfloat16().float()
    _far("maxima_not_rescaled", z3, 7, 7169, ctx)
    assert set(rl.WRONG) == {"lse_candidates", "stats_on_temp", "temp_distribution", "padding_included", "second_batch_dropped",
                             "maxima_not_rescaled", "argmax_logit"}


def test_event_ll_counts_positions_zero_to_arity():
    arity = [0, 3, 0, 1]
    v = [-1.0, -2.0, -4.0, -8.0, -16.0, -32.0, -64.0, -128.0]
    assert rl.event_ll(v, [1, 9, 9, 9, 0, 0, 0, 0], arity, eos_id=2) == -15.0
    assert rl.event_ll(v, [3, 9, 0, 0, 0, 0, 0, 0], arity, eos_id=2) == -3.0
    assert rl.event_ll(v, [2, 0, 0, 0, 0, 0, 0, 0], arity, eos_id=2) == -1.0  # EOS: position 0 alone
    assert math.isclose(float(rl.bound(torch.zeros(64), 0)), rl.U * (1.5 * (math.log(64) + 2) + 24 + 4 * (1 + math.log(64))))
