"""CPU: what-if scenarios without a GPU -- smx_host_scenario against scenario_util's restatement on
the C oracle's tables by bit pattern, the hand-made tables, what a scenario means (a warm run on
the scenario table ends where the cold run on the perturbed original ends), SimplexMethod.what_if
on the host backend, the case in which a warm run does not terminate, the C ABI's argument checks
and the refusal of the new batch calls before any device call."""
from __future__ import annotations

import numpy as np
import pytest

import ranging_util as ru
import scenario_util as scu
import solution_util as su

DEMO = ([[1.0, 1.0, -2.0], [-1.0, 1.0, 1.5], [1.0, -2.0, 4.0]], [-1.0, -1.0])
FRAC, PROB = 0.05, 0.25


@pytest.mark.parametrize("k", range(len(ru.CASES)),
                         ids=[f"{c[0]}-{c[1]}x{c[2]}-s{c[3]}" for c in ru.CASES])
def test_host_scenario_on_oracle_tables(k):
    _, n, m, seed, _ = ru.CASES[k]
    ref = ru.case(k)
    applied = 0
    for s in range(3):
        drhs, dcost, S, func_s, basis, nonbasis = scu.scenario_of_case(ref, n, m, seed, s, FRAC,
                                                                       PROB)
        applied += int((drhs != 0).sum() + (dcost != 0).sum())
        for ld, ld_out in ((None, None), (m + 1 + 5, m + 1 + 3)):
            err, got, fgot = scu.host(ref[2], n, m, basis, nonbasis, ref[0][n, :m], drhs, dcost,
                                      ld=ld, ld_out=ld_out)
            assert err == 0
            scu.same_table(got, S, (ru.CASES[k], s, ld))
            assert su.same_floats(fgot, func_s), (ru.CASES[k], s, "func_s")
        # everything but row n and column m is T's bits
        assert np.array_equal(su.bits(S[:n, :m]), su.bits(ref[2][:n, :m]))
    assert applied > 0, ru.CASES[k]


def test_the_ordered_sums_are_sharp():
    """At 63 x 63 and at 300 x 40 the ordered sums of step 1 and of step 2 differ in the last bits
    from np.dot over the same terms in at least one scenario each: a tree or blocked reduction in
    the twin or the kernel fails the comparisons of this file and of the GPU tests."""
    for k in (2, 7):
        _, n, m, seed, _ = ru.CASES[k]
        assert (n, m) in ((63, 63), (300, 40))
        ref = ru.case(k)
        differs = [0, 0]
        for s in range(3):
            drhs, dcost, S, _, basis, nonbasis = scu.scenario_of_case(ref, n, m, seed, s, FRAC,
                                                                      PROB)
            frow = S[n, :m].copy()
            # step 2 on T alone, so that np.dot sees the same terms as the ordered sum
            S2, _ = scu.restate(ref[2], n, m, basis, nonbasis, ref[0][n, :m], drhs, np.zeros(m))
            dfrow, _ = scu.dot_variant(ref[2], n, m, basis, nonbasis, np.zeros(n), dcost)
            _, db = scu.dot_variant(ref[2], n, m, basis, nonbasis, drhs, np.zeros(m))
            assert np.allclose(dfrow, frow, rtol=1e-9, atol=1e-12)
            assert np.allclose(db, S2[:n, m], rtol=1e-9, atol=1e-12)
            differs[0] += int((su.bits(dfrow) != su.bits(frow)).any())
            differs[1] += int((su.bits(db) != su.bits(S2[:n, m])).any())
        assert differs[0] > 0 and differs[1] > 0, (ru.CASES[k], differs)


HANDMADE = scu.handmade()


@pytest.mark.parametrize("case", HANDMADE, ids=[c[0] for c in HANDMADE])
def test_host_scenario_on_handmade_tables(case):
    name, T, n, m, basis, nonbasis, func, dr, dc, pins = case
    err, S, func_s = scu.host(T, n, m, basis, nonbasis, func, dr, dc)
    assert err == 0
    scu.check_handmade(case, S, func_s)
    for (p, j), v in pins.items():
        assert su.same_floats(S[p, j], v, nan_aware=True), (name, p, j, float(S[p, j]).hex())
    if name == "all zero":                                   # bit-identical, NaN included
        assert np.array_equal(su.bits(S), su.bits(T))
        assert np.array_equal(su.bits(func_s), su.bits(func))


def test_handmade_tables_hold_their_events():
    names = [c[0] for c in HANDMADE]
    assert len(set(names)) == len(names) >= 8
    pinned = [v for c in HANDMADE for v in c[9].values()]
    assert any(np.isnan(v) for v in pinned) and any(np.isinf(v) for v in pinned)
    assert any(v == 0 and np.signbit(v) for v in pinned)
    assert any(v == 0 and not np.signbit(v) for v in pinned)
    assert any(np.isnan(c[7]).any() and np.isnan(c[8]).any() for c in HANDMADE)
    assert any((c[4] < 0).any() and (c[4] >= c[2] + c[3]).any() for c in HANDMADE)


# ----------------------------------------------------------------------------------------------
# what a scenario means
def _perturbed(T0, n, m, drhs, dcost):
    P = np.array(T0, dtype=np.float64)
    P[:n, m] = np.where(drhs != 0, P[:n, m] + drhs, P[:n, m])
    P[n, :m] = np.where(dcost != 0, P[n, :m] + dcost, P[n, :m])
    return P


def test_a_warm_run_ends_where_the_cold_run_of_the_perturbed_original_ends():
    """Uniform LPs, seeds 0..199, n = 3 + seed % 9, m = 2 + seed % 5, cap 256; scenarios 0..3 at
    frac 0.5, prob 0.5, re-solved with the C oracle only.  On every LP whose base run ends at
    `optimum` the warm run on S and the cold run on the perturbed original end with the same
    status, and at `optimum` with the same set of basis codes.  The counts are pinned (the pivot
    totals over the 581 scenarios that end at `optimum`)."""
    from oracle import c_oracle
    from simplex_mi355x import lp
    lps = pairs = 0
    by_status = {0: 0, 1: 0, 2: 0, 3: 0}
    nowarm = warm_pivots = cold_pivots = 0
    for seed in range(200):
        n, m = 3 + seed % 9, 2 + seed % 5
        T0 = lp.dense_tableau("uniform", seed, n, m)
        Tf, st, _, log = c_oracle.run(T0, n, m, m, 256)
        if st != 1:
            continue
        lps += 1
        basis, nonbasis, _ = su.replay(log, n, m)
        for s in range(4):
            drhs, dcost = scu.deltas(T0, n, m, seed, s, 0.5, 0.5)
            S, _ = scu.restate(Tf, n, m, basis, nonbasis, T0[n, :m], drhs, dcost)
            _, wst, wdone, wlog = c_oracle.run(S, n, m, m, 256)
            _, cst, cdone, clog = c_oracle.run(_perturbed(T0, n, m, drhs, dcost), n, m, m, 256)
            assert wst == cst, (seed, s, wst, cst)
            if wst == 1:
                wb, _ = scu.warm_labels(basis, nonbasis, wlog, n, m)
                cb, _, _ = su.replay(clog, n, m)
                assert set(wb.tolist()) == set(cb.tolist()), (seed, s)
            pairs += 1
            by_status[wst] += 1
            nowarm += wdone == 0
            if wst == 1:                                     # the totals: runs to `optimum`
                warm_pivots += wdone
                cold_pivots += cdone
    assert (lps, pairs) == (158, 632)
    assert (by_status[1], by_status[2], by_status[3], by_status[0]) == (581, 44, 7, 0)
    assert (nowarm, pairs - nowarm) == (371, 261)
    assert (warm_pivots, cold_pivots) == (470, 1535)


def test_the_fallback_case_exists_on_the_oracle():
    """Uniform 60 x 12, seed 5, scenario 1 at frac 0.2, prob 0.5: the base run takes 12 pivots to
    `optimum`, the warm run is still pivoting at cap 512, the cold run reaches `optimum` in 22."""
    from oracle import c_oracle
    from simplex_mi355x import lp
    n, m, seed = 60, 12, 5
    T0 = lp.dense_tableau("uniform", seed, n, m)
    Tf, st, done, log = c_oracle.run(T0, n, m, m, 256)
    assert (st, done) == (1, 12)
    basis, nonbasis, _ = su.replay(log, n, m)
    drhs, dcost = scu.deltas(T0, n, m, seed, 1, 0.2, 0.5)
    S, _ = scu.restate(Tf, n, m, basis, nonbasis, T0[n, :m], drhs, dcost)
    _, wst, wdone, _ = c_oracle.run(S, n, m, m, 512)
    assert (wst, wdone) == (0, 512)
    _, cst, cdone, _ = c_oracle.run(_perturbed(T0, n, m, drhs, dcost), n, m, m, 512)
    assert (cst, cdone) == (1, 22)


# ----------------------------------------------------------------------------------------------
# SimplexMethod.what_if on the host backend
def _sm(cons, func):
    import simplex
    sm = simplex.SimplexMethod([list(r) for r in cons], list(func), device="cpu")
    assert sm.backend == "host"
    return sm


def _what_if_case(cons, func, n, m, drhs, dcost, cap):
    """Base solve on the host engine, what_if, warm solve: against the restatement on the C
    oracle's final table and the oracle's warm run on it."""
    from oracle import c_oracle
    T0 = np.zeros((n + 1, m + 1))
    T0[:n] = cons
    T0[n, :m] = func
    Tf, _, done, log = c_oracle.run(T0, n, m, m, cap)
    basis, nonbasis, _ = su.replay(log, n, m)
    S, func_s = scu.restate(Tf, n, m, basis, nonbasis, func, drhs, dcost)
    sm = _sm(cons, func)
    sm.solve(record_history=False, max_pivots=cap)
    assert sm.pivots == done
    wi = sm.what_if(drhs, dcost)
    assert wi is not sm and wi.backend == "host" and wi.pivots == 0 and wi.status == "ready"
    assert wi.row == sm.row and wi.column == sm.column and wi.row is not sm.row
    assert su.label_codes(wi.column[:-1], m) == basis.tolist()
    assert su.label_codes(wi.row[:-1], m) == nonbasis.tolist()
    assert su.same_floats(wi.function, func_s)
    scu.same_table(wi._dev.download()[:n + 1, :m + 1], S, "what_if table")
    Tw, wst, wdone, wlog = c_oracle.run(S, n, m, m, cap)
    wi.solve(record_history=False, max_pivots=cap)
    assert wi.pivots == wdone and wi.pivot_log == [tuple(map(int, rc)) for rc in wlog]
    assert wi.status == {0: "cap", 1: "optimum", 2: "error", 3: "error"}[wst]
    wb, wn = scu.warm_labels(basis, nonbasis, wlog, n, m)
    su.same_solution(wi.solution(), scu.expected_solution(Tw, wb, wn, n, m, func_s, wdone),
                     "what_if solution")
    ru.same_ranges(wi.ranging(), ru.expected(Tw, wb, wn, n, m), "what_if ranging")
    # the base object is untouched
    assert sm.pivots == done and list(sm.function) == list(func)
    return wdone


def test_what_if_on_the_demo_lp():
    cons, func = DEMO
    # the demo's ranges (test_ranging.py): rhs 0 holds to -10.5, cost 0 to +1.5 -- inside: no pivot
    assert _what_if_case(cons, func, 3, 2, [-1.0, 0.0, 0.0], [0.5, 0.0], 64) == 0
    # past the cost range the basis changes: the warm run pivots
    assert _what_if_case(cons, func, 3, 2, [-1.0, 0.0, 0.0], [2.0, 0.0], 64) > 0
    # before the first pivot: the caller's own lists under the identity labels
    sm = _sm(cons, func)
    wi = sm.what_if([0.5, 0.0, 0.0], [0.0, 0.25])
    T = np.array(cons + [func + [0.0]])
    T[0, 2] += 0.5
    T[3, 1] += 0.25
    scu.same_table(wi._dev.download()[:4, :3], T, "pristine")
    assert wi.function == [-1.0, -0.75]
    none = sm.what_if()
    scu.same_table(none._dev.download()[:4, :3], np.array(cons + [func + [0.0]]), "no change")


@pytest.mark.parametrize("k", (1, 3, 4))
def test_what_if_on_seeded_cases(k):
    _, n, m, seed, cap = ru.CASES[k]
    ref = ru.case(k)
    drhs, dcost = scu.deltas(ref[0], n, m, seed, 0, 0.5, 0.5)
    _what_if_case(ref[0][:n].tolist(), ref[0][n, :m].tolist(), n, m, drhs, dcost, cap)


# ----------------------------------------------------------------------------------------------
# the C ABI and the Python arguments
def test_envelope_function():
    from simplex_mi355x import _lib
    from simplex_mi355x.batch import scenario_fits
    L = _lib.load()
    for Rmax, ldb in ((2, 2), (2, 8190), (8190, 2), (4097, 4095)):
        assert L.smx_batch_scenario_fits(Rmax, ldb) == 1, (Rmax, ldb)
        assert scenario_fits(Rmax, ldb) is True
    for Rmax, ldb in ((1, 3), (2, 8191), (-1, 4)):
        assert L.smx_batch_scenario_fits(Rmax, ldb) == 0, (Rmax, ldb)
        assert scenario_fits(Rmax, ldb) is False
    assert scenario_fits(1 << 40, 2) is False


def test_entry_points_refuse_bad_arguments_before_any_hip_call():
    """hipErrorInvalidValue (1) for a shape outside the envelope, a negative count, a count past
    2^31 - 1, a group below 1 or a null pointer; B == 0 or S == 0 is a success without a launch.
    None of these reaches the HIP runtime."""
    from simplex_mi355x import _lib
    L = _lib.load()
    null = [None] * 8
    assert L.smx_batch_scenario(None, None, 0, 3, 4, 3, *null, None) == 0
    assert L.smx_batch_scenario(None, None, 5, 0, 4, 3, *null, None) == 0
    assert L.smx_batch_scenario(None, None, -1, 3, 4, 3, *null, None) == 1
    assert L.smx_batch_scenario(None, None, 1, -3, 4, 3, *null, None) == 1
    assert L.smx_batch_scenario(None, None, 1 << 20, 1 << 12, 4, 3, *null, None) == 1
    assert L.smx_batch_scenario(None, None, 0, 3, 1, 3, *null, None) == 1
    assert L.smx_batch_scenario(None, None, 0, 3, 2, 8191, *null, None) == 1
    assert L.smx_batch_scenario(None, None, 2, 3, 4, 3, *null, None) == 1
    sol = [None] * 5
    assert L.smx_batch_solution_from(None, None, 0, 4, 3, 8, None, None, None, None, None, 1,
                                     *sol, None) == 0
    assert L.smx_batch_solution_from(None, None, 0, 4, 3, 8, None, None, None, None, None, 0,
                                     *sol, None) == 1
    assert L.smx_batch_solution_from(None, None, -1, 4, 3, 8, None, None, None, None, None, 1,
                                     *sol, None) == 1
    assert L.smx_batch_solution_from(None, None, 0, 4, 8189, 8, None, None, None, None, None, 1,
                                     *sol, None) == 1
    assert L.smx_batch_solution_from(None, None, 2, 4, 3, 8, None, None, None, None, None, 1,
                                     *sol, None) == 1
    assert L.smx_host_scenario(None, 3, 2, 2, *[None] * 5, None, 3, None) == -1
    T = np.zeros((3, 3))
    lab = np.zeros(2, dtype=np.int32)
    vec = [np.zeros(2) for _ in range(3)]
    out, fout = np.zeros((3, 3)), np.zeros(2)
    ptrs = [a.ctypes.data for a in (lab, lab, *vec)]
    assert L.smx_host_scenario(T.ctypes.data, 2, 2, 2, *ptrs, out.ctypes.data, 3,
                               fout.ctypes.data) == -1                      # ld < m + 1
    assert L.smx_host_scenario(T.ctypes.data, 3, 2, 2, *ptrs, out.ctypes.data, 2,
                               fout.ctypes.data) == -1                      # ld_out < m + 1
    assert L.smx_host_scenario(T.ctypes.data, 3, 0, 2, *ptrs, out.ctypes.data, 3,
                               fout.ctypes.data) == -1
    assert L.smx_host_scenario(T.ctypes.data, 3, 2, 2, *ptrs, out.ctypes.data, 3,
                               fout.ctypes.data) == 0


def test_new_calls_refuse_before_any_device_call(monkeypatch):
    import torch
    from simplex_mi355x import batch
    tabs = np.zeros((1, 3, 3))
    tabs[0] = [[1.0, 1.0, 2.0], [1.0, -1.0, 1.0], [-1.0, -1.0, 0.0]]
    dims = np.array([[2, 2, 2]], dtype=np.int32)
    drhs, dcost = np.zeros((1, 2, 2)), np.zeros((1, 2, 2))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)

    def boom(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(torch, "from_numpy", boom)
    with pytest.raises(ValueError, match="drhs must be"):
        batch.solve_batch_scenarios_arrays(tabs, dims, np.zeros((1, 2, 3)), dcost)
    with pytest.raises(ValueError, match="dcost must be"):
        batch.solve_batch_scenarios_arrays(tabs, dims, drhs, np.zeros((1, 3, 2)))
    with pytest.raises(ValueError, match="kernel must be"):
        batch.solve_batch_scenarios_arrays(tabs, dims, drhs, dcost, kernel="lds")
    # without a device the new calls refuse like the rest of the batch path: no CPU fall-back
    with pytest.raises(RuntimeError, match="no CPU path"):
        batch.solve_batch_scenarios_arrays(tabs, dims, drhs, dcost)
    with pytest.raises(RuntimeError, match="no CPU path"):
        batch.solve_batch_scenarios([([[1.0, 1.0, 2.0]], [-1.0, -1.0])], [[(None, None)]])
    with pytest.raises(ValueError, match="kernel must be"):
        batch.solve_batch_scenarios([], [], kernel="lds")
    with pytest.raises(ValueError, match="one list of scenarios per problem"):
        batch.solve_batch_scenarios([([[1.0, 1.0, 2.0]], [-1.0, -1.0])], [])
