"""The work-item table of the grouped weight-gradient launch, seen from the host (mh_wgrad_grouped_item: the same table builder
and the same item -> (problem, tile) function the kernel runs, compiled for the host; no device is touched).  Over all workgroups
of every group of tests/test_gemm_wgrad_grouped_gpu.py and of the benchmarked layer (128 + 64 + 48 + 16 tiles), every
(problem, tile row, tile column) occurs exactly once, and the workgroups an XCD receives (linear id mod 8) are one contiguous
run of the problem-major tile order."""
import ctypes

import pytest

import test_gemm_wgrad_grouped_gpu as T

GROUP_SHAPES = [[T.OUTS[i] for i in g] for g in T.GROUPS] + [T.LAYER_DIV8, T.LAYER_TILES,
                                                             [T.LAYER_TILES[1], T.LAYER_TILES[0], T.LAYER_TILES[3], T.LAYER_TILES[2]],
                                                             [(256 * (j + 1), 256) for j in range(8)]]


def table(shapes):
    arr = (T.Problem * len(shapes))()
    for q, (N, K_out) in zip(arr, shapes):
        q.dz = q.x = q.dw = 16                      # (never dereferenced on the host)
        q.lddz, q.ldx, q.lddw, q.N, q.K_out = N, K_out, K_out, N, K_out
    return arr


@pytest.fixture(scope="module")
def item():
    from midi_model_amd.lib import lib
    fn = lib().cdll.mh_wgrad_grouped_item

    def item_of(arr, lin):
        p, tm, tn = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
        n = fn(arr, len(arr), lin, ctypes.byref(p), ctypes.byref(tm), ctypes.byref(tn))
        return n, (p.value, tm.value, tn.value)
    return item_of


@pytest.mark.parametrize("shapes", GROUP_SHAPES, ids=lambda s: "+".join(f"{n}x{k}" for n, k in s))
def test_every_tile_of_every_problem_exactly_once(item, shapes):
    arr = table(shapes)
    want = [(j, tm, tn) for j, (N, K_out) in enumerate(shapes) for tm in range(-(-N // 256)) for tn in range(-(-K_out // 256))]
    n, _ = item(arr, -1)
    assert n == len(want)
    got = [item(arr, lin)[1] for lin in range(n)]
    assert sorted(got) == sorted(want)
    # XCD x (workgroups lin = x mod 8) takes a contiguous range of the problem-major order: its problems never go backwards
    # and it misses no workgroup in between
    first = {j: sum(-(-N // 256) * -(-K // 256) for N, K in shapes[:j]) for j in range(len(shapes))}
    for x in range(8):
        probs = [got[lin][0] for lin in range(x, n, 8)]
        assert probs == sorted(probs)
    order = sorted(range(n), key=lambda lin: (lin % 8, lin // 8))            # the item order: XCD-major
    assert [got[lin][0] for lin in order] == sorted(g[0] for g in got)
    for j in first:                                                           # and inside a problem, items are consecutive
        lins = [lin for lin in order if got[lin][0] == j]
        assert [order.index(lin) for lin in lins] == list(range(first[j], first[j] + len(lins)))


def test_benchmarked_layer_fills_the_chip_and_bad_arguments(item):
    arr = table(T.LAYER_TILES)
    assert item(arr, -1)[0] == 256
    assert item(arr, 256) == (256, (-1, -1, -1))                              # past the grid: nothing resolved
    from midi_model_amd.lib import lib
    assert lib().cdll.mh_wgrad_grouped_item(arr, 0, 0, None, None, None) == -1
    assert lib().cdll.mh_wgrad_grouped_item(arr, 9, 0, None, None, None) == -1
    assert [lib().cdll.mh_wgrad_grouped_fold_blocks(n) for n in (1, 256, 257, 520, 8192)] == [1, 1, 2, 3, 32]
