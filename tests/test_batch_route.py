"""CPU: where solve_batch sends a problem, the workgroup kernel's envelope as the library states
it, and the argument checks of smx_batch_solve_wg (all before any device call)."""
from __future__ import annotations

import numpy as np
import pytest


def _lp(n, m, seed=0, ints=False):
    rng = np.random.default_rng(seed)
    if ints:
        cons = [[int(x) for x in rng.integers(-3, 4, size=m + 1)] for _ in range(n)]
        return cons, [int(x) for x in rng.integers(-3, 4, size=m)]
    return rng.uniform(-1, 1, size=(n, m + 1)).tolist(), rng.uniform(-1, 1, size=m).tolist()


def test_route_wave_workgroup_single():
    from simplex_mi355x.batch import route
    assert route(*_lp(3, 2)) == "wave"
    assert route(*_lp(63, 63)) == "wave"
    for n, m in ((64, 2), (3, 64), (65, 65), (300, 40), (40, 300)):
        assert route(*_lp(n, m)) == "workgroup", (n, m)
    assert route(*_lp(65, 65, ints=True)) == "single"
    cons, func = _lp(65, 65)
    cons[7] = cons[7][:-1]
    assert route(cons, func) == "single"                    # ragged
    cons, func = _lp(65, 65)
    cons[7][3] = 1
    assert route(cons, func) == "single"                    # one int entry
    cons, func = _lp(70, 5)
    assert route(cons, func[:3]) == "single"                # the reference's IndexError (f short)
    assert route(cons, func + [0.5]) == "workgroup"         # len(function) = m + 1
    assert route([], [1.0, 2.0]) == "single"


def test_route_oversize_is_single():
    from simplex_mi355x.batch import route
    row = [0.5] * 4001
    assert route([row] * 4000, [0.5] * 4000) == "single"


def test_route_agrees_with_eligible():
    """"wave" is exactly the old eligibility rule, so every existing call keeps its kernel."""
    from simplex_mi355x.batch import _eligible, route
    for n, m in ((1, 2), (3, 2), (63, 2), (64, 2), (3, 63), (3, 64), (20, 20)):
        cons, func = _lp(n, m)
        assert (route(cons, func) == "wave") == _eligible(cons, func) == (n < 64 and m < 64)


def test_wg_lds_bytes_envelope():
    from simplex_mi355x import _lib
    L = _lib.load()
    f = L.smx_batch_wg_lds_bytes
    assert f(66, 66) > 0
    assert f(66, 66) >= 66 * 66 * 8                         # holds the table at least
    assert f(66, 66) < 48 * 1024                            # several 65 x 65 LPs share a CU
    assert f(4001, 4001) == -1
    assert f(1, 66) == -1 and f(66, 1) == -1
    assert f(2, 2) > 0
    assert f(301, 41) > 0 and f(41, 301) > 0
    prev_r = prev_c = 0
    for k in range(2, 400):
        r, c = f(k, 40), f(40, k)
        for cur, prev in ((r, prev_r), (c, prev_c)):
            assert cur == -1 or cur > prev >= 0             # grows until it stops fitting
            assert not (prev == -1 and cur != -1)
        prev_r, prev_c = r, c
    fits = [k for k in range(2, 400) if f(k, k) >= 0]
    assert fits == list(range(2, fits[-1] + 1))             # one edge, no holes
    assert f(fits[-1], fits[-1]) <= 160 * 1024


def test_solve_wg_rejects_bad_arguments_before_any_device_call():
    from simplex_mi355x import _lib
    L = _lib.load()
    nul = (None,) * 6

    def call(B, Rmax, ldb, P):
        return L.smx_batch_solve_wg(None, None, B, Rmax, ldb, P, *nul, None)

    assert call(-1, 66, 66, 8) == 1
    assert call(4, 1, 66, 8) == 1
    assert call(4, 66, 1, 8) == 1
    assert call(4, 66, 66, -1) == 1
    assert call(4, 4001, 4001, 8) == 1                      # does not fit a CU's LDS
    assert call(0, 66, 66, 8) == 0                          # nothing to do, no launch


def test_choose_kernel():
    from simplex_mi355x.batch import choose_kernel
    assert choose_kernel(64, 64) == "wave"
    assert choose_kernel(65, 3) == "workgroup"
    assert choose_kernel(4, 65) == "workgroup"
    assert choose_kernel(4, 3, "workgroup") == "workgroup"
    assert choose_kernel(4, 3, "wave") == "wave"
    with pytest.raises(ValueError, match="envelope"):
        choose_kernel(100, 3, "wave")
    with pytest.raises(ValueError, match="envelope"):
        choose_kernel(4001, 4001)
    with pytest.raises(ValueError, match="envelope"):
        choose_kernel(4001, 4001, "workgroup")
    with pytest.raises(ValueError, match="kernel must be"):
        choose_kernel(4, 3, "warp")


def test_solve_batch_arrays_forced_wave_refuses_100_rows():
    """The shape check is choose_kernel, the first thing solve_batch_arrays does once it knows a
    device exists; with a device the call itself is made."""
    import torch
    from simplex_mi355x.batch import solve_batch_arrays
    tabs = np.zeros((2, 100, 3))
    dims = np.array([[99, 2, 2]] * 2, dtype=np.int32)
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="envelope"):
            solve_batch_arrays(tabs, dims, 8, kernel="wave")
    else:
        with pytest.raises(RuntimeError, match="no CPU path"):
            solve_batch_arrays(tabs, dims, 8, kernel="wave")


def test_wg_launches_rule():
    from simplex_mi355x.batch import SNAP_BUDGET, wg_launches, wg_lds_bytes
    shapes = [(65, 65)] * 5 + [(300, 40)] * 3 + [(40, 300)] * 3 + [(70, 5), (120, 8), (66, 64)]
    parts = wg_launches(shapes, 64, False)
    assert sorted(q for p in parts for q in p) == list(range(len(shapes)))
    for p in parts:
        R = max(shapes[q][0] for q in p) + 1
        C = max(shapes[q][1] for q in p) + 1
        lds = wg_lds_bytes(R, C)
        assert lds >= 0
        assert lds <= 2 * min(wg_lds_bytes(shapes[q][0] + 1, shapes[q][1] + 1) for q in p)
    assert any(set(p) == {0, 1, 2, 3, 4, 13} for p in parts)     # 65 x 65 with 66 x 64
    assert not any({5, 8} <= set(p) for p in parts)              # 300 x 40 never pads 40 x 300
    # history: 128 x 128 at 256 pivots is ~34 MB of snapshots per LP
    shapes = [(128, 128)] * 70
    per_lp = 256 * 129 * 129 * 8
    parts = wg_launches(shapes, 256, True)
    assert len(parts) > 1 and sum(len(p) for p in parts) == 70
    assert all(len(p) * per_lp <= SNAP_BUDGET for p in parts)
    assert len(wg_launches(shapes, 256, False)) == 1
