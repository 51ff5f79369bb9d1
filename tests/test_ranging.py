"""CPU: sensitivity ranging without a GPU -- smx_host_ranging against ranging_util on the C
oracle's tables by bit pattern, the hand-made tables of events the generators never produce, the
demo LP through SimplexMethod.ranging(), what a range means (the basis holds inside it and changes
outside), the C ABI's argument checks and the refusal of the new batch arguments before any device
call."""
from __future__ import annotations

import random

import numpy as np
import pytest

import ranging_util as ru
import solution_util as su

inf = float("inf")
DEMO = ([[1.0, 1.0, -2.0], [-1.0, 1.0, 1.5], [1.0, -2.0, 4.0]], [-1.0, -1.0])


def test_sharp_cases_keep_their_edge():
    """The seeded inputs of this file and of the GPU tests: variables in the basis, bounds with
    both ends finite, lo <= 0 <= hi at every optimum -- asserted on the oracle's own tables."""
    ru.check_sharp_cases()


@pytest.mark.parametrize("k", range(len(ru.CASES)),
                         ids=[f"{c[0]}-{c[1]}x{c[2]}-s{c[3]}" for c in ru.CASES])
def test_host_ranging_on_oracle_tables(k):
    _, n, m, _, _ = ru.CASES[k]
    ref = ru.case(k)
    basis, nonbasis, _ = su.replay(ref[5], n, m)
    exp = ru.of_case(ref, n, m)
    err, got = ru.host(ref[2], n, m, basis, nonbasis)
    assert err == 0
    ru.same_ranges(got, exp, ru.CASES[k])
    err, wide = ru.host(ref[2], n, m, basis, nonbasis, ld=m + 1 + 5)      # ld > m + 1
    assert err == 0
    ru.same_ranges(wide, exp, (ru.CASES[k], "ld"))


HANDMADE = ru.handmade()


@pytest.mark.parametrize("case", HANDMADE, ids=[c[0] for c in HANDMADE])
def test_host_ranging_on_handmade_tables(case):
    name, T, n, m, basis, nonbasis, pins = case
    err, got = ru.host(T, n, m, basis, nonbasis)
    assert err == 0
    ru.check_handmade(name, got, T, n, m, basis, nonbasis, pins)
    for (field, slot), v in pins.items():
        assert su.same_floats(getattr(got, field)[slot], v), (name, field, slot)


def test_handmade_tables_hold_their_events():
    names = [c[0] for c in HANDMADE]
    assert len(set(names)) == len(names) >= 12
    pinned = [v for c in HANDMADE for v in c[6].values()]
    assert any(np.isnan(v) for v in pinned)
    assert any(v == 0 and np.signbit(v) for v in pinned)
    assert any(v == 0 and not np.signbit(v) for v in pinned)


def _sm(cons, func):
    import simplex
    sm = simplex.SimplexMethod([list(r) for r in cons], list(func), device="cpu")
    assert sm.backend == "host"
    return sm


def test_demo_lp_ranges():
    from simplex_mi355x import Ranging
    sm = _sm(*DEMO)
    first = sm.ranging()
    assert isinstance(first, Ranging)
    assert first.rhs_lo.tolist() == [2.0, -1.5, -4.0] and first.rhs_hi.tolist() == [inf] * 3
    assert first.cost_lo.tolist() == [1.0, 1.0] and first.cost_hi.tolist() == [inf] * 2
    sm.solve()
    assert sm.status == "optimum"
    got = sm.ranging()
    assert all(a.dtype == np.float64 for a in got)
    assert list(zip(got.rhs_lo.tolist(), got.rhs_hi.tolist())) == \
        [(-10.5, inf), (-3.5, inf), (-5.25, inf)]
    assert list(zip(got.cost_lo.tolist(), got.cost_hi.tolist())) == [(-inf, 1.5), (-inf, 2.0)]
    exp = ru.expected(sm._dev.download(), su.label_codes(sm.column[:-1], 2),
                      su.label_codes(sm.row[:-1], 2), 3, 2)
    ru.same_ranges(got, exp, "demo")


def test_ranging_after_each_step_follows_the_labels():
    sm = _sm(*DEMO)
    while sm.step()[0]:
        basis, nonbasis, _ = su.replay(sm.pivot_log, 3, 2)
        ru.same_ranges(sm.ranging(), ru.expected(sm._dev.download(), basis, nonbasis, 3, 2),
                       sm.pivots)


def test_host_engine_ranging_on_a_sharp_case():
    """The host engine's chained loop, then ranging(): against ranging_util on the C oracle's
    final table."""
    k = 3                                                    # mixed 20 x 20
    _, n, m, _, cap = ru.CASES[k]
    ref = ru.case(k)
    sm = _sm(ref[0][:n].tolist(), ref[0][n, :m].tolist())
    sm.solve(record_history=False, max_pivots=cap)
    assert sm.pivot_log == [tuple(map(int, rc)) for rc in ref[5]]
    ru.same_ranges(sm.ranging(), ru.of_case(ref, n, m), ru.CASES[k])


# ----------------------------------------------------------------------------------------------
# what a range means
def _basis_set(T, n, m):
    """The set of basic codes the oracle stops at, or None without an optimum."""
    from oracle import c_oracle
    _, st, _, log = c_oracle.run(T, n, m, m, 256)
    if st != 1:
        return None
    return frozenset(su.replay(log, n, m)[0].tolist())


def test_the_basis_holds_inside_every_range_and_changes_outside():
    """200 seeded small LPs; every bound probed just inside (0.9 x, or +-5 where infinite) and,
    where finite, just outside (by max(1e-3, 0.1 |bound|)), re-solved with the C oracle: the same
    set of basic codes inside, another set or no optimum outside.  Bounds within 1e-9 of zero are
    skipped, nothing else."""
    from oracle import c_oracle
    rnd = random.Random()
    rnd.seed(1)
    probes = 0
    for _ in range(200):
        n, m = rnd.randint(3, 8), rnd.randint(2, 5)
        T = np.zeros((n + 1, m + 1))
        for i in range(n):
            T[i, :m] = [round(rnd.uniform(-5, 1), 2) for _ in range(m)]
            T[i, m] = round(rnd.uniform(1, 20), 2)
        T[n, :m] = [round(rnd.uniform(-3, -0.5), 2) for _ in range(m)]
        Tf, st, _, log = c_oracle.run(T, n, m, m, 256)
        if st != 1:
            continue
        basis, nonbasis, _ = su.replay(log, n, m)
        base = frozenset(basis.tolist())
        err, rng = ru.host(Tf, n, m, basis, nonbasis)
        assert err == 0
        cells = [((i, m), rng.rhs_lo[i], rng.rhs_hi[i]) for i in range(n)]
        cells += [((n, k), rng.cost_lo[k], rng.cost_hi[k]) for k in range(m)]
        for at, lo, hi in cells:
            assert lo <= 0 <= hi, (at, lo, hi)
            for bound, side in ((float(lo), -1.0), (float(hi), 1.0)):
                if abs(bound) <= 1e-9:
                    continue
                P = T.copy()
                P[at] += 0.9 * bound if np.isfinite(bound) else side * 5.0
                assert _basis_set(P, n, m) == base, (at, bound, "inside")
                probes += 1
                if np.isfinite(bound):
                    P = T.copy()
                    P[at] += bound + side * max(1e-3, 0.1 * abs(bound))
                    assert _basis_set(P, n, m) != base, (at, bound, "outside")
                    probes += 1
    assert probes == 5984


# ----------------------------------------------------------------------------------------------
# the C ABI and the Python arguments
def test_envelope_function():
    from simplex_mi355x import _lib
    from simplex_mi355x.batch import ranging_fits
    L = _lib.load()
    for Rmax, ldb in ((2, 2), (2, 8190), (8190, 2), (4097, 4095)):
        assert L.smx_batch_ranging_fits(Rmax, ldb) == 1, (Rmax, ldb)
        assert ranging_fits(Rmax, ldb) is True
    for Rmax, ldb in ((1, 3), (2, 8191), (-1, 4)):
        assert L.smx_batch_ranging_fits(Rmax, ldb) == 0, (Rmax, ldb)
        assert ranging_fits(Rmax, ldb) is False
    assert ranging_fits(1 << 40, 2) is False


def test_entry_point_refuses_bad_arguments_before_any_hip_call():
    """hipErrorInvalidValue (1) for a shape outside the envelope, a negative count or a null
    pointer; B == 0 is a success without a launch.  None of these reaches the HIP runtime."""
    from simplex_mi355x import _lib
    L = _lib.load()
    null = [None] * 6
    assert L.smx_batch_ranging(None, None, 0, 4, 3, *null, None) == 0
    assert L.smx_batch_ranging(None, None, -1, 4, 3, *null, None) == 1
    assert L.smx_batch_ranging(None, None, 0, 1, 3, *null, None) == 1
    assert L.smx_batch_ranging(None, None, 0, 2, 8191, *null, None) == 1
    assert L.smx_batch_ranging(None, None, 2, 4, 3, *null, None) == 1
    assert L.smx_host_ranging(None, 3, 2, 2, *null) == -1
    T = np.zeros((3, 3))
    lab = np.zeros(2, dtype=np.int32)
    out = [np.zeros(2) for _ in range(4)]
    ptrs = [a.ctypes.data for a in (lab, lab, *out)]
    assert L.smx_host_ranging(T.ctypes.data, 2, 2, 2, *ptrs) == -1          # ld < m + 1
    assert L.smx_host_ranging(T.ctypes.data, 3, 0, 2, *ptrs) == -1
    assert L.smx_host_ranging(T.ctypes.data, 3, 2, 2, *ptrs) == 0


def test_new_arguments_are_refused_before_any_device_call(monkeypatch):
    import torch
    from simplex_mi355x import batch
    tabs = np.zeros((1, 3, 3))
    tabs[0] = [[1.0, 1.0, 2.0], [1.0, -1.0, 1.0], [-1.0, -1.0, 0.0]]
    dims = np.array([[2, 2, 2]], dtype=np.int32)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)

    def boom(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(torch, "from_numpy", boom)
    with pytest.raises(ValueError, match="ranging=True needs solution=True"):
        batch.solve_batch_arrays(tabs, dims, ranging=True)
    with pytest.raises(ValueError, match="solution=True"):
        batch.solve_batch_arrays(tabs, dims, ranging=True, tables=False)
    # without a device the new mode refuses like the rest of the batch path: no CPU fall-back
    with pytest.raises(RuntimeError, match="no CPU path"):
        batch.solve_batch_arrays(tabs, dims, solution=True, ranging=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        batch.solve_batch_arrays(tabs, dims, solution=True, ranging=True, tables=False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        batch.solve_batch_ranges([([[1.0, 1.0, 2.0]], [-1.0, -1.0])])
    with pytest.raises(ValueError, match="kernel must be"):
        batch.solve_batch_ranges([], kernel="lds")
