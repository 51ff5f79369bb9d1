"""CPU: the global-memory batch tier -- where solve_batch sends a problem past the LDS edge, the
kernel's envelope as the library states it, the argument checks of smx_batch_solve_gm and the
launch planner (all before any device call)."""
from __future__ import annotations

import numpy as np
import pytest


def _lp(n, m, seed=0, ints=False):
    rng = np.random.default_rng(seed)
    if ints:
        cons = [[int(x) for x in rng.integers(-3, 4, size=m + 1)] for _ in range(n)]
        return cons, [int(x) for x in rng.integers(-3, 4, size=m)]
    return rng.uniform(-1, 1, size=(n, m + 1)).tolist(), rng.uniform(-1, 1, size=m).tolist()


def test_route_global_past_the_lds_edge():
    from simplex_mi355x.batch import KERNELS, route, wg_lds_bytes
    assert "global" in KERNELS
    for n, m in ((141, 141), (200, 120), (40, 600), (1100, 20)):
        assert wg_lds_bytes(n + 1, m + 1) == -1
        assert route(*_lp(n, m)) == "global", (n, m)
    assert route(*_lp(141, 140)) == "workgroup"             # still fits LDS: the exact edge
    cons, func = _lp(200, 120)
    assert route(cons, func + [0.5]) == "global"            # len(function) = m + 1
    assert route(cons, func[:3]) == "single"                # the reference's IndexError (f short)


def test_route_single_cases_stay_single():
    from simplex_mi355x.batch import route
    assert route(*_lp(200, 120, ints=True)) == "single"
    cons, func = _lp(200, 120)
    cons[7][3] = 1
    assert route(cons, func) == "single"                    # one int entry
    cons, func = _lp(200, 120)
    cons[7] = cons[7][:-1]
    assert route(cons, func) == "single"                    # ragged
    row = [0.5] * 4001
    assert route([row] * 4000, [0.5] * 4000) == "single"
    # the tiers below are where they were
    assert route(*_lp(3, 2)) == "wave"
    assert route(*_lp(65, 65)) == "workgroup"
    assert route(*_lp(65, 65, ints=True)) == "single"


def test_gm_fits_envelope():
    from simplex_mi355x import _lib
    from simplex_mi355x.batch import gm_fits
    L = _lib.load()
    f = L.smx_batch_gm_fits
    assert f(2, 2) == 1 and f(142, 142) == 1 and f(201, 121) == 1 and f(1101, 21) == 1
    assert f(1, 66) == 0 and f(66, 1) == 0 and f(0, 0) == 0 and f(-5, 7) == 0
    assert f(4001, 4001) == 0
    assert f(601, 1101) == 0                                # the padded mix of the GPU test
    assert gm_fits(142, 142) and not gm_fits(4001, 4001) and not gm_fits(1 << 40, 2)
    # one edge and no holes along squares and along both thin directions
    sq = [k for k in range(2, 3000) if f(k, k)]
    assert sq == list(range(2, sq[-1] + 1)) and 142 <= sq[-1] < 4001
    for thin in (2, 21, 41):
        for g in (lambda k: f(k, thin), lambda k: f(thin, k)):
            fits = [k for k in range(2, 70000, 7) if g(k)]
            assert fits == list(range(2, fits[-1] + 1, 7)) and fits[-1] > 1101
            assert not g(fits[-1] + 7)
    # every shape the LDS kernel takes fits here too
    w = L.smx_batch_wg_lds_bytes
    for R in list(range(2, 160)) + [301, 401, 1000, 3000, 6783, 6784, 7000]:
        for C in list(range(2, 160)) + [301, 401, 1000, 3000, 6783, 6784, 7000]:
            if w(R, C) >= 0:
                assert f(R, C) == 1, (R, C)


def test_solve_gm_rejects_bad_arguments_before_any_device_call():
    from simplex_mi355x import _lib
    L = _lib.load()
    nul = (None,) * 6

    def call(B, Rmax, ldb, P):
        return L.smx_batch_solve_gm(None, None, B, Rmax, ldb, P, *nul, None)

    assert call(-1, 142, 142, 8) == 1
    assert call(4, 1, 142, 8) == 1
    assert call(4, 142, 1, 8) == 1
    assert call(4, 142, 142, -1) == 1
    assert call(4, 4001, 4001, 8) == 1                      # outside the envelope
    assert call(4, 601, 1101, 8) == 1
    assert call(0, 142, 142, 8) == 0                        # nothing to do, no launch


def test_choose_kernel_global():
    from simplex_mi355x.batch import choose_kernel
    assert choose_kernel(142, 142, "global") == "global"
    assert choose_kernel(4, 3, "global") == "global"        # any shape from 2 x 2
    assert choose_kernel(66, 66, "global") == "global"
    with pytest.raises(ValueError, match="envelope"):
        choose_kernel(4001, 4001, "global")
    with pytest.raises(ValueError, match="envelope"):
        choose_kernel(601, 1101, "global")
    # the others are as they were: "auto" still refuses a shape past the LDS edge
    assert choose_kernel(64, 64) == "wave"
    assert choose_kernel(142, 141) == "workgroup"
    for kernel in ("auto", "wave", "workgroup"):
        with pytest.raises(ValueError, match="envelope"):
            choose_kernel(143, 143, kernel)


def test_gm_launches_rule():
    from simplex_mi355x import batch
    from simplex_mi355x.batch import gm_fits, gm_launches
    shapes = ([(141, 141)] * 5 + [(200, 120)] * 3 + [(120, 200)] * 3 + [(600, 40), (40, 600)] +
              [(1100, 20), (20, 1100), (3, 2), (65, 65), (511, 511), (150, 141)])
    parts = gm_launches(shapes, 64, False)
    assert sorted(q for p in parts for q in p) == list(range(len(shapes)))
    for p in parts:
        R = max(shapes[q][0] for q in p) + 1
        C = max(shapes[q][1] for q in p) + 1
        assert gm_fits(R, C)
        assert R * C <= 2 * min((shapes[q][0] + 1) * (shapes[q][1] + 1) for q in p)
    assert any({0, 1, 2, 3, 4, 18} <= set(p) for p in parts)     # 141 x 141 with 150 x 141
    assert not any({11, 12} <= set(p) for p in parts)            # 600 x 40 never pads 40 x 600
    # the table budget: 512 x 512 is 2 MiB per LP
    shapes = [(511, 511)] * 1200
    parts = gm_launches(shapes, 256, False)
    assert len(parts) > 1 and sum(len(p) for p in parts) == 1200
    assert all(len(p) * 512 * 512 * 8 <= batch.GM_TABLE_BUDGET for p in parts)
    assert batch.GM_TABLE_BUDGET == 1 << 30
    # history: 141 x 141 at 256 pivots is ~41 MB of snapshots per LP
    shapes = [(141, 141)] * 70
    per_lp = 256 * 142 * 142 * 8
    parts = gm_launches(shapes, 256, True)
    assert len(parts) > 1 and sum(len(p) for p in parts) == 70
    assert all(len(p) * per_lp <= batch.SNAP_BUDGET for p in parts)
    assert len(gm_launches(shapes, 256, False)) == 1
    # a single LP is never split, even past the snapshot budget
    assert gm_launches([(511, 511)], 4096, True) == [[0]]
    assert isinstance(batch.GM_MIN_BATCH, int) and batch.GM_MIN_BATCH >= 1
