"""Every training-block schedule of engine.py on the MI355X, slice by slice, against float64 (reference, stand-in yardstick and
measure: tests/ref_block.py; the CPU half and the proof that the measure bites: tests/test_block_bounds_host.py).

Each case builds LayerTensors from seeded bf16 tensors (weights std 0.02 .. 0.04, norm weights 1 +- 0.1, x std 1, dy std 1/64)
between NaN guard rows, NaN-filled gradient buffers, calls the engine's block functions directly, and holds the block output x3,
rstd1, rstd2, dx and the six parameter gradients to ``block_fp64`` on the same values: the whole-tensor, worst-row and
worst-column relative L2 distance (vectors: whole and max) of the device run is at most MARGIN = 1.5 x the same distance of the
SAME schedule run on the CPU through the stand-ins -- never another device schedule.  The stand-in run comes first, so a wrong
shape or argument shows before anything is launched.  Each case asserts the path it is there for, by the C-ABI entry points the
run called (lib.call is counted), the problems per grouped launch and ops.wgrad_grouped_launches.

Shapes (the smallest that reach each path):
  event D 256, H 4, I 1024, 2 x 100 rows   S no multiple of 64, M no multiple of 256; folded: one-problem grouped wgrads (M < 1024)
  event 2 x 516 rows (M = 1032)            wgrad_folded in 2 slices: mh_gemm_splitk_reduce_fold + mh_colsum, no grouped launch
  event D 1024, H 16, I 4096, 2 x 132      the four weight gradients as ONE grouped launch of 256 tiles; again with MH_WGRAD_GROUPED=0
  two chained folded blocks, 2 x 100       the second block's rstd1 from the first block's down-projection statistics
  packed (33, 200, 7, 128, 129, 3)         M = 500: the sequence-table attention, gemm_nt_scaled, RoPE per row position
  token D 512, H 2, I 1024, 52 x 8 rows    tokattn_* with the row scale
  token first block N = 300, V = 200       id 5 occurs >= 1100 times (> SEG_OWN), the pad id 3 times (once mid-sequence), 15 ids never
  event folded "spread"                    added to the cases above: rows of x at scales 0.5 .. 2, so that rstd is far from 1 -- with
                                           x std 1 in every row rstd = 1 +- 0.04 and a row scale missed in a 4-row group of the
                                           attention backward stays under every margin (test_block_bounds_host.py shows both)

MEASURED on the MI355X (profiles/block_schedules_gpu.txt), d(device) / d(stand-in), the worst tensor per slice kind:
  case                         whole          worst row      worst column   max (vectors)
  event plain                  1.006 dn1      1.019 dWd      1.009 dWd      1.000
  event folded                 1.013 dn2      1.009 dWo      1.002 dx       1.000
  event folded spread          1.070 dn2      1.000 x3       1.024 dx       1.177 dn1
  event folded splitk          1.004 dWo      1.008 dx       1.026 dx       1.002 rstd2
  event folded grouped         1.007 dn1      1.014 dx       1.028 x3       1.039 rstd2  (MH_WGRAD_GROUPED=0: the same to 3 digits)
  event folded chain           1.044 1.dn2    1.058 0.dWgu   1.118 1.dWd    1.030 1.rstd2
  event plain accumulate       1.003 dn2      1.029 dWd      1.042 dWo      1.041 dn2
  event folded accumulate      1.014 dn2      1.010 dWgu     1.015 dWqkv    1.180 dn1
  event plain / folded lean    as event plain / folded (same bits)
  packed plain                 1.052 dWqkv    1.095 dWqkv    1.057 dWqkv    0.998
  packed folded                1.130 dn1      1.100 dWo      1.096 dWqkv    1.262 dn1
  token plain                  1.018 dn2      1.001 dWgu     1.007 dWgu     1.193 dn2
  token folded                 1.001 dWgu     1.005 x3       1.013 dWd      1.091 dn1
  token first                  1.011 dn1      1.004 dWd      1.036 dhidden  1.278 dn1
  event plain fp32             1.427 dn2      1.420 dWgu     1.523 dWd      1.513 dn2    <- over 1.5: xfail(strict), see below
  token plain fp32             1.605 dWd      1.963 dWgu     1.977 dWd      1.426 dn2    <- over 1.5: xfail(strict), see below
The bf16 distances are 0.002 .. 0.019 on both sides (rstd2: 2e-4 .. 6e-4; rstd1, fp32 from exact inputs: 1e-7).  MARGIN = 1.5 holds
for every bf16 case and no case has a margin of its own.

The stand-in and the MFMA attention.  With emu_ops' attention (P, dS and delta in fp32) the uniform event-level cases stood at up to
1.15 x in a 2-D slice and dn1 of the "spread" case at 1.83 x in ONE element of 256 (whole vector 1.08; 0.77 .. 1.83 over eight seeds):
an excess in one slice.  Its cause was tested, not supposed: ref_block.attn_fwd_event / attn_bwd_event restate the kernels' rounding
points (attention_mfma3.hip: P into P @ V and P^T dO as bf16, delta from the stored bf16 O, the unscaled dS = P (dP - delta) as bf16),
and with them in the stand-in the same element stands at 1.18 x, eight seeds of the case at 1.00 .. 1.25, and every uniform
event-level case within 1.18 x (table above).  The packed and token-level cases run emu_packed / emu_ops as they are.

fp32 (the unfused verification schedule; distances 1e-7 .. 1e-6 on both sides): the device is 1.25 .. 1.98 x further from float64
than the fp32 stand-in, over the margin in event dWd (col 1.523) and dn2 (max 1.513) and in token dWd (1.605 / 1.617 / 1.977), dWgu
(1.552 / 1.963 / 1.557), dWo (col 1.557), dn2 (all 1.518) and x3 (1.553 / 1.330 / 1.592).  Over three seeds the 50 % and 90 %
quantiles of the per-row and per-column distances carry the whole-tensor ratio to +-0.07 and the maximum over the slices scatters
(1.15 .. 1.98): spread over all slices, no row or column stands out.  The cause is NOT found.  One supposition was tested and
refuted: a stand-in GEMM that adds every element in one fp32 chain over K, four k per step and per split-K slice, as the kernel's
v_mfma_f32_16x16x4_f32 loop does, came out CLOSER to float64 than the CPU BLAS (ratios 1.5 .. 2.2 over four seeds), so the
summation order is not what separates the device.  Not yet looked at: the rounding inside the fp32 MFMA, fast_exp2 / rsqrt in the
fp32 attention, SwiGLU and norm kernels.  Without a named rounding point there is no margin to set: both fp32 cases are
xfail(strict=True) with these figures, and every bf16 case is unaffected.

Time on the MI355X: the module's 18 tests in 5.6 s (the slowest 1.3 s), stand-in runs and float64 references included.
"""
import pytest
import torch

import ref_block as R
from midi_model_amd import lib as lib_mod
from midi_model_amd import ops, ops_grouped

pytestmark = pytest.mark.gpu

# the fp32 cases miss MARGIN and the cause is not found (module docstring): the measured slices, d(device) / d(stand-in)
XFAIL = {
    "event plain fp32": "fp32 device run 1.25 .. 1.52 x the fp32 stand-in's distance to float64, spread over all slices; over 1.5: dWd col "
                        "1.523 (whole 1.370), dn2 max 1.513 (whole 1.427); cause not found (a one-chain fp32 GEMM stand-in refuted)",
    "token plain fp32": "fp32 device run 1.33 .. 1.98 x the fp32 stand-in's distance to float64, spread over all slices; over 1.5: dWd "
                        "1.605 / row 1.617 / col 1.977, dWgu 1.552 / 1.963 / 1.557, dWo col 1.557, dn2 all 1.518, x3 1.553 / 1.330 / "
                        "1.592; cause not found (a one-chain fp32 GEMM stand-in refuted)",
}

F_EVENT = {"mh_row_rstd": 2, "mh_gemm_rope_scaled": 1, "mh_gemm_rowss": 2, "mh_gemm_swiglu_scaled": 1, "mh_gemm_dswiglu_scaled": 1,
           "mh_attn_fwd": 1, "mh_attn_bwd_o_scaled": 1, "mh_rmsnorm_bwd_folded": 2, "mh_colsum": 2,
           "mh_rmsnorm_fwd": 0, "mh_rmsnorm_bwd": 0, "mh_gemm_rope": 0, "mh_gemm_swiglu": 0, "mh_gemm_dswiglu": 0, "mh_swiglu_fwd": 0}
P_EVENT = {"mh_rmsnorm_fwd": 2, "mh_gemm_rope": 1, "mh_attn_fwd": 1, "mh_gemm_swiglu": 1, "mh_gemm_dswiglu": 1, "mh_attn_bwd_o": 1,
           "mh_rmsnorm_bwd": 2, "mh_colsum": 2, "mh_gemm_wgrad_grouped": 0, "mh_row_rstd": 0, "mh_gemm_rowss": 0, "mh_rope": 0,
           "mh_swiglu_fwd": 0, "mh_swiglu_bwd": 0, "mh_gemm_splitk_reduce_fold": 0}
ONE_PROBLEM = {"mh_gemm_wgrad_grouped": 2, "mh_gemm_splitk_reduce_fold": 0}
BACKWARD = ("mh_gemm_dswiglu", "mh_gemm_dswiglu_scaled", "mh_attn_bwd_o", "mh_attn_bwd_o_scaled", "mh_rmsnorm_bwd", "mh_rmsnorm_bwd_folded",
            "mh_colsum", "mh_gemm_wgrad_grouped")


def twice(expect, names=BACKWARD):
    return {k: v * (2 if k in names else 1) for k, v in expect.items()}


# case -> (entry point -> exact number of calls, problems per grouped launch, ops.wgrad_grouped_launches)
PATHS = {
    "event plain": (P_EVENT, [], 0),
    "event folded": ({**F_EVENT, **ONE_PROBLEM}, [1, 1], 2),
    "event folded spread": ({**F_EVENT, **ONE_PROBLEM}, [1, 1], 2),
    "event folded splitk": ({**F_EVENT, "mh_gemm_wgrad_grouped": 0, "mh_gemm_splitk_reduce_fold": 2}, [], 0),
    "event folded grouped": ({**F_EVENT, "mh_gemm_wgrad_grouped": 1, "mh_gemm_splitk_reduce_fold": 0}, [4], 1),
    "event folded chain": ({k: 2 * v for k, v in {**F_EVENT, **ONE_PROBLEM}.items()}, [1, 1, 1, 1], 4),
    "event plain accumulate": (twice(P_EVENT), [], 0),
    "event folded accumulate": (twice({**F_EVENT, **ONE_PROBLEM}), [1, 1, 1, 1], 4),
    "event plain lean": ({**P_EVENT, "mh_swiglu_fwd": 1}, [], 0),
    "event folded lean": ({**F_EVENT, **ONE_PROBLEM, "mh_swiglu_fwd": 1}, [1, 1], 2),
    "packed plain": ({**P_EVENT, "mh_gemm_rope": 0, "mh_attn_fwd": 0, "mh_attn_bwd_o": 0, "mh_rope_pos": 1, "mh_attn_fwd_seqs": 1,
                      "mh_attn_bwd_seqs": 1, "mh_gemm_nt_scaled": 0}, [], 0),
    "packed folded": ({**F_EVENT, **ONE_PROBLEM, "mh_gemm_rope_scaled": 0, "mh_attn_fwd": 0, "mh_attn_bwd_o_scaled": 0, "mh_gemm_nt_scaled": 1,
                       "mh_rope_pos": 1, "mh_attn_fwd_seqs": 1, "mh_attn_bwd_seqs": 1}, [1, 1], 2),
    "token plain": ({**P_EVENT, "mh_gemm_rope": 0, "mh_attn_fwd": 0, "mh_attn_bwd_o": 0, "mh_tokattn_fwd": 1, "mh_tokattn_bwd": 1,
                     "mh_tokattn_bwd_scaled": 0}, [], 0),
    "token folded": ({**F_EVENT, **ONE_PROBLEM, "mh_gemm_rope_scaled": 0, "mh_attn_fwd": 0, "mh_attn_bwd_o_scaled": 0, "mh_gemm_nt_scaled": 1,
                      "mh_tokattn_fwd": 1, "mh_tokattn_bwd_scaled": 1, "mh_tokattn_bwd": 0}, [1, 1], 2),
    # (the q|k|v gradient contracts N + 2 V = 700 rows: one-problem grouped; gate|up contracts 2400 rows: split-K with the fold)
    "token first": ({"mh_tokattn_fwd_rows": 1, "mh_tokattn_bwd_rows": 1, "mh_tokattn_fwd": 0, "mh_tokattn_bwd": 0, "mh_tokattn_bwd_scaled": 0,
                     "mh_embed_segment_sum": 2, "mh_embed_split_hi_lo": 1, "mh_embed_table_norm_bwd": 1, "mh_embed_segment_bwd": 1,
                     "mh_gemm_nt_scaled": 1, "mh_gemm_wgrad_grouped": 1, "mh_gemm_splitk_reduce_fold": 1, "mh_rmsnorm_bwd_folded": 2,
                     "mh_rmsnorm_fwd": 0, "mh_rmsnorm_bwd": 0}, [1], 1),
    "event plain fp32": ({"mh_rmsnorm_fwd": 2, "mh_rmsnorm_bwd": 2, "mh_rope": 1, "mh_attn_fwd": 1, "mh_attn_prep_bwd": 1, "mh_attn_bwd": 1,
                          "mh_swiglu_fwd": 1, "mh_swiglu_bwd": 1, "mh_gemm_rope": 0, "mh_gemm_swiglu": 0, "mh_gemm_dswiglu": 0,
                          "mh_attn_bwd_o": 0, "mh_gemm_wgrad_grouped": 0}, [], 0),
    "token plain fp32": ({"mh_rmsnorm_fwd": 2, "mh_rmsnorm_bwd": 2, "mh_rope": 0, "mh_tokattn_fwd": 1, "mh_tokattn_bwd": 1,
                          "mh_swiglu_fwd": 1, "mh_swiglu_bwd": 1, "mh_gemm_swiglu": 0, "mh_gemm_dswiglu": 0, "mh_gemm_wgrad_grouped": 0}, [], 0),
}
assert set(PATHS) == set(R.CASES)


class MarginMissed(AssertionError):
    """a distance over its margin (the one failure an xfail case may show: its path assertions must still hold)"""


def device_run(case, monkeypatch):
    """R.run_case on the device -> (tensors, entry point -> calls, problems per grouped launch, grouped launches)"""
    calls, groups = {}, []
    real_call, real_grouped = lib_mod._Lib.call, ops_grouped.wgrad_grouped

    def call(self, name, *a):
        calls[name] = calls.get(name, 0) + 1
        return real_call(self, name, *a)

    def grouped(problems, accumulate):
        groups.append(len(problems))
        return real_grouped(problems, accumulate)
    before = ops.wgrad_grouped_launches
    with monkeypatch.context() as m:
        m.setattr(lib_mod._Lib, "call", call)
        m.setattr(ops_grouped, "wgrad_grouped", grouped)     # (ops.wgrad_grouped and ops.wgrad_folded both resolve it there)
        got = R.run_case(case, "cuda")
    return got, calls, groups, ops.wgrad_grouped_launches - before


def assert_path(name, calls, groups, launches, path=None):
    expect, want_groups, want_launches = path or PATHS[name]
    seen = {k: calls.get(k, 0) for k in expect}
    assert seen == expect, f"{name}: entry points called {seen}, expected {expect}"
    assert groups == want_groups and launches == want_launches, (name, groups, launches)


def hold(name, monkeypatch, path=None, tag=None):
    case = R.CASES[name]
    zero = {"dtable": R.inputs(case)["zero_rows"]} if case.first else None
    ref, standin = R.reference(case), R.standin_run(case)    # CPU first
    got, calls, groups, launches = device_run(case, monkeypatch)
    rows = R.check(got, standin, ref, R.MARGIN, zero, tag=tag or name, raise_on_fail=False)
    assert_path(name, calls, groups, launches, path)
    bad = [(n, k, f"{a:.3e}", f"{b:.3e}", f"{q:.3f}") for n, k, a, b, q, ok in rows if not ok]
    if bad:
        raise MarginMissed(f"{name}: (tensor, slice kind, device, stand-in, ratio) over the margin: {bad}")
    return got


@pytest.mark.parametrize("name", [pytest.param(n, marks=pytest.mark.xfail(strict=True, raises=MarginMissed, reason=XFAIL[n])) if n in XFAIL else n
                                  for n in R.CASES if "lean" not in n and "grouped" not in n])
def test_block_schedule_against_float64(name, monkeypatch):
    case = R.CASES[name]
    if case.folded and case.kind == "event" and not case.lengths:
        from midi_model_amd.ops import _pick_splitk
        want = 2 if "splitk" in name else 1
        assert _pick_splitk(3 * case.D, case.D, case.M) == want and _pick_splitk(2 * case.I, case.D, case.M) == want
    hold(name, monkeypatch)


@pytest.mark.parametrize("env", ["1", "0"])
def test_grouped_weight_gradients_against_float64(env, monkeypatch):
    """one grouped launch of four problems (256 tiles); with MH_WGRAD_GROUPED=0 one split-K launch with the fold in its reduction
    per folded gradient -- each run against float64, not against the other"""
    monkeypatch.setenv("MH_WGRAD_GROUPED", env)
    name = "event folded grouped"
    path = PATHS[name] if env == "1" else ({**F_EVENT, "mh_gemm_wgrad_grouped": 0, "mh_gemm_splitk_reduce_fold": 2}, [], 0)
    hold(name, monkeypatch, path, tag=name if env == "1" else "grouped, GROUPED=0")


@pytest.mark.parametrize("name", ["event plain lean", "event folded lean"])
def test_lean_block_has_the_bits_of_the_full_one(name, monkeypatch):
    """``a`` is dropped and recomputed in the backward: every output is bit-equal to the run that kept it, and held to float64"""
    lean = hold(name, monkeypatch)
    full, _, _, _ = device_run(R.CASES[name].but(lean=False), monkeypatch)
    R.same_bits(lean, full)
