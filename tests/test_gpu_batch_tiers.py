"""GPU: one launch through every batch kernel that can take it (wave, workgroup, global) gives the
same arrays bit for bit, and each LP of it equals the C oracle."""
from __future__ import annotations

import numpy as np
import pytest

from batch_util import OUTCOME, case, same_as_oracle, solve

pytestmark = pytest.mark.gpu

# (kind, n, m) of the padded launch, seeds 0 and 1 of each: 41 x 31 blocks around 40 x 30, 12 x 30
# and 40 x 3 LPs, so each LP's own n, m sits inside the padding and every workgroup size is larger
# than some rows
PADDED = [(kind, n, m) for kind in ("uniform", "mixed") for n, m in ((40, 30), (12, 30), (40, 3))]
VARIANTS = [(1024, 1, 4), (1024, 0, 1), (1024, 1, 8), (512, 1, 1), (512, 0, 4), (256, 0, 8)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def _degenerate_20():
    """degenerate_mixed 20 x 20 (ties, +-0 ratios), cap 64, half the LPs at flen = m + 1."""
    return [(20, 20, case("degenerate_mixed", 20, 20, s, 64, 21 if s % 2 else 20))
            for s in range(8)], 64, {}


def _padded():
    return [(n, m, case(kind, n, m, s, 256, m)) for kind, n, m in PADDED
            for s in range(2)], 256, {"Rmax": 41, "ldb": 31}


def _degenerate_65():
    return [(65, 65, case("degenerate_mixed", 65, 65, s, 96, 65)) for s in range(4)], 96, {}


def _launch(refs, cap, pad, kernel):
    out = solve([(ref[0], n, m, ref[1]) for n, m, ref in refs], cap, history=True, kernel=kernel,
                **pad)
    for q, (n, m, ref) in enumerate(refs):                  # no agreement on a shared wrong answer
        same_as_oracle(out, q, n, m, ref, (kernel, q))
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _same_arrays(a, b, refs, what):
    """Every output of solve_batch_arrays(history=True) that the kernels define: tables inside
    each LP's own (n + 1) x (m + 1), rc and xv up to its pivot count."""
    for key in ("status", "npivots", "snap_off"):
        assert np.array_equal(a[key], b[key]), (what, key)
    assert a["snaps"].shape == b["snaps"].shape, what
    for q, (n, m, _) in enumerate(refs):
        done = int(a["npivots"][q])
        lo, hi = a["snap_off"][q], a["snap_off"][q + 1]
        assert hi - lo == done, (what, q)
        assert np.array_equal(a["rc"][q, :done], b["rc"][q, :done]), (what, q)
        assert np.array_equal(_bits(a["xv"][q, :done]), _bits(b["xv"][q, :done])), (what, q)
        assert np.array_equal(_bits(a["final"][q, :n + 1, :m + 1]),
                              _bits(b["final"][q, :n + 1, :m + 1])), (what, q)
        assert np.array_equal(_bits(a["snaps"][lo:hi, :n + 1, :m + 1]),
                              _bits(b["snaps"][lo:hi, :n + 1, :m + 1])), (what, q)


def test_cases_hold_the_outcomes_that_can_differ():
    """The C oracle's outcomes of the two three-tier sets (run on the CPU when this file was
    written): the comparison cannot pass on LPs that all stop at step 0."""
    seen = {OUTCOME[ref[3]] for make in (_degenerate_20, _padded) for _, _, ref in make()[0]}
    assert seen == {"optimum", "incorrect", "not_converge", "cap"}
    assert {OUTCOME[ref[3]] for _, _, ref in _degenerate_20()[0]} == {"cap", "not_converge"}
    assert sorted({ref[1] for _, _, ref in _degenerate_20()[0]}) == [20, 21]


@pytest.mark.parametrize("make", [_degenerate_20, _padded], ids=["degenerate-20x20", "padded-41x31"])
def test_wave_workgroup_global_give_the_same_arrays(make):
    refs, cap, pad = make()
    wave = _launch(refs, cap, pad, "wave")
    assert wave["final"].shape[1:] == (pad.get("Rmax", 21), pad.get("ldb", 21))
    for kernel in ("workgroup", "global"):
        _same_arrays(wave, _launch(refs, cap, pad, kernel), refs, kernel)


def test_workgroup_and_every_global_variant_give_the_same_arrays():
    from simplex_mi355x import _lib
    refs, cap, pad = _degenerate_65()
    wg = _launch(refs, cap, pad, "workgroup")
    assert {OUTCOME[int(v)] for v in wg["status"]} == {"cap"} and int(wg["npivots"].min()) == 96
    L = _lib.load()
    prev = L.smx_tune_batch_gm(-1, -1, -1)
    try:
        for threads, mirrors, unroll in VARIANTS:
            L.smx_tune_batch_gm(threads, mirrors, unroll)
            _same_arrays(wg, _launch(refs, cap, pad, "global"), refs, (threads, mirrors, unroll))
    finally:
        L.smx_tune_batch_gm(prev & 0xffff, (prev >> 16) & 0xf, prev >> 20)
    assert L.smx_tune_batch_gm(-1, -1, -1) == prev
