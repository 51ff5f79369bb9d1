"""CPU: new constraints on a solved LP without a GPU -- smx_host_cuts against cuts_util's
restatement on the C oracle's tables by bit pattern, the hand-made tables, what an extended table
means (a warm run on it ends where the cold run on the enlarged original ends), the case in which
it does not, SimplexMethod.add_constraints on the host backend, the C ABI's argument checks and the
refusal of the new batch calls before any device call."""
from __future__ import annotations

import numpy as np
import pytest

import cuts_util as cu
import ranging_util as ru
import solution_util as su

DEMO = ([[1.0, 1.0, -2.0], [-1.0, 1.0, 1.5], [1.0, -2.0, 4.0]], [-1.0, -1.0])
SETS = (0, 1, 3)                                             # K' of cut sets 0, 1, 2


@pytest.mark.parametrize("k", range(len(ru.CASES)),
                         ids=[f"{c[0]}-{c[1]}x{c[2]}-s{c[3]}" for c in ru.CASES])
def test_host_cuts_on_oracle_tables(k):
    _, n, m, seed, _ = ru.CASES[k]
    ref = ru.case(k)
    applied = 0
    for s, K in enumerate(SETS):
        G, E, basis_c, basis, nonbasis = cu.cuts_of_case(ref, n, m, seed, s, K)
        applied += sum(int(G[c, basis[p]] != 0) for c in range(K) for p in range(n)
                       if basis[p] < m)
        for ld, ld_out in ((None, None), (m + 1 + 5, m + 1 + 3)):
            err, got, bgot = cu.host(ref[2], n, m, basis, nonbasis, G, ld=ld, ld_out=ld_out)
            assert err == 0
            cu.same_table(got, E, (ru.CASES[k], s, ld))
            assert np.array_equal(bgot, basis_c), (ru.CASES[k], s)
        # everything but the new rows is T's bits, the f-row K rows further down
        assert np.array_equal(su.bits(E[:n]), su.bits(ref[2][:n, :m + 1]))
        assert np.array_equal(su.bits(E[n + K]), su.bits(ref[2][n, :m + 1]))
    assert applied > 0, ru.CASES[k]


def test_identity_labels_give_the_enlarged_original():
    """A base run of zero pivots: E is the original table with the cuts appended, bit for bit."""
    for k in (0, 3, 4):
        _, n, m, seed, _ = ru.CASES[k]
        T0 = ru.case(k)[0]
        G = cu.cut_set(T0, n, m, seed, 0, 3, 0.05, np.zeros(m))
        G[1, 0], G[2, m - 1] = -0.0, 0.0
        err, E, bc = cu.host(T0, n, m, np.arange(m, m + n), np.arange(m), G)
        assert err == 0
        assert np.array_equal(su.bits(E), su.bits(cu.enlarged(T0, n, m, G)))
        assert bc.tolist() == list(range(m, m + n + 3))
        cu.same_table(cu.restate(T0, n, m, np.arange(m, m + n), np.arange(m), G)[0], E, k)


def test_the_ordered_sum_is_sharp():
    """At 63 x 63 and at 300 x 40 the ordered sum of a new row differs in the last bits from
    np.dot over the same terms in at least one of three cuts: a tree or blocked reduction in the
    twin or the kernel fails the comparisons of this file and of the GPU tests."""
    for k in (2, 7):
        _, n, m, seed, _ = ru.CASES[k]
        assert (n, m) in ((63, 63), (300, 40))
        ref = ru.case(k)
        G, E, _, basis, nonbasis = cu.cuts_of_case(ref, n, m, seed, 2, 3)
        differs = 0
        for c in range(3):
            dot = cu.dot_variant(ref[2], n, m, basis, nonbasis, G[c])
            assert np.allclose(dot, E[n + c], rtol=1e-9, atol=1e-12)
            differs += int((su.bits(dot) != su.bits(E[n + c])).any())
        assert differs > 0, ru.CASES[k]


HANDMADE = cu.handmade()


@pytest.mark.parametrize("case", HANDMADE, ids=[c[0] for c in HANDMADE])
def test_host_cuts_on_handmade_tables(case):
    name, T, n, m, basis, nonbasis, G, pins = case
    err, E, basis_c = cu.host(T, n, m, basis, nonbasis, G)
    assert err == 0
    cu.check_handmade(case, E, basis_c)
    for (c, j), v in pins.items():
        assert su.same_floats(E[n + c, j], v, nan_aware=True), (name, c, j, float(E[n + c, j]).hex())
    if name == "zero coefficients over inf and nan":
        assert not np.isnan(E[n:n + 2]).any()
    if name == "no cuts":
        assert np.array_equal(su.bits(E), su.bits(T)) and E.shape == (n + 1, m + 1)


def test_handmade_tables_hold_their_events():
    names = [c[0] for c in HANDMADE]
    assert len(set(names)) == len(names) >= 7
    pinned = [v for c in HANDMADE for v in c[7].values()]
    assert any(np.isnan(v) for v in pinned) and any(np.isinf(v) for v in pinned)
    assert any(v == 0 and np.signbit(v) for v in pinned)
    assert any(v == 0 and not np.signbit(v) for v in pinned)
    assert any(np.isnan(np.asarray(c[6], dtype=float)).any() for c in HANDMADE)
    assert any((c[4] < 0).any() and (c[4] >= c[2] + c[3]).any() for c in HANDMADE)
    assert any(len(c[6]) == 0 for c in HANDMADE)


# ----------------------------------------------------------------------------------------------
# what an extended table means
def _pair(seed, s, K, viol, cap):
    from oracle import c_oracle
    from simplex_mi355x import lp
    n, m = 3 + seed % 9, 2 + seed % 5
    T0 = lp.dense_tableau("uniform", seed, n, m)
    Tf, _, _, log = c_oracle.run(T0, n, m, m, cap)
    basis, nonbasis, _ = su.replay(log, n, m)
    G = cu.cut_set(T0, n, m, seed, s, K, viol, su.expected(Tf, log, n, m, T0[n]).x)
    E, basis_c = cu.restate(Tf, n, m, basis, nonbasis, G)
    _, wst, wdone, wlog = c_oracle.run(E, n + K, m, m, cap)
    _, cst, cdone, clog = c_oracle.run(cu.enlarged(T0, n, m, G), n + K, m, m, cap)
    wb, _ = cu.warm_labels(basis_c, nonbasis, wlog, n + K, m)
    cb, _, _ = su.replay(clog, n + K, m)
    return wst, wdone, set(wb.tolist()), cst, cdone, set(cb.tolist())


def test_a_warm_run_ends_where_the_cold_run_of_the_enlarged_original_ends():
    """Uniform LPs, seeds 0..199, n = 3 + seed % 9, m = 2 + seed % 5, cap 512; cut sets 0..3 of one
    cut each at 5 % of the mean constant, re-solved with the C oracle only, whatever the base run's
    status.  In all 800 pairs the warm run on E and the cold run on the enlarged original end with
    the same status, and at `optimum` with the same set of basis codes.  The counts are pinned;
    the sets 1 and 3 are the ones the base answer already satisfies (no warm pivot)."""
    by_status = {0: 0, 1: 0, 2: 0, 3: 0}
    nowarm = [0, 0, 0, 0]
    pairs = warm_pivots = cold_pivots = 0
    for seed in range(200):
        for s in range(4):
            wst, wdone, wb, cst, cdone, cb = _pair(seed, s, 1, 0.05, 512)
            assert wst == cst, (seed, s, wst, cst)
            pairs += 1
            by_status[wst] += 1
            if wst == 1:
                assert wb == cb, (seed, s)
                nowarm[s] += wdone == 0
                warm_pivots += wdone
                cold_pivots += cdone
    assert pairs == 800
    assert (by_status[1], by_status[2], by_status[3], by_status[0]) == (615, 66, 119, 0)
    assert nowarm == [0, 158, 0, 158]
    assert (warm_pivots, cold_pivots) == (532, 2025)


def test_the_fallback_case_exists_on_the_oracle():
    """Seed 183 (n = 6, m = 5), cut set 2 of two cuts at 20 %: the warm run ends at "does not
    converge" after 4 pivots, the cold run of the enlarged original at `optimum` after 8.  The
    selection rule is no dual simplex; this is the only status disagreement among the 800 pairs
    of that kind."""
    pairs = {(seed, s): _pair(seed, s, 2, 0.2, 512) for seed in range(200) for s in range(4)}
    assert pairs[183, 2][:2] == (3, 4) and pairs[183, 2][3:5] == (1, 8)
    assert [key for key, p in pairs.items() if p[0] != p[3]] == [(183, 2)]


# ----------------------------------------------------------------------------------------------
# SimplexMethod.add_constraints on the host backend
def _sm(cons, func):
    import simplex
    sm = simplex.SimplexMethod([list(r) for r in cons], list(func), device="cpu")
    assert sm.backend == "host"
    return sm


def _add_case(cons, func, n, m, rows, cap):
    """Base solve on the host engine, add_constraints, warm solve: against the restatement on the
    C oracle's final table, the oracle's warm run on it and its cold run on the enlarged LP."""
    from oracle import c_oracle
    T0 = np.zeros((n + 1, m + 1))
    T0[:n] = cons
    T0[n, :m] = func
    K = len(rows)
    Tf, _, done, log = c_oracle.run(T0, n, m, m, cap)
    basis, nonbasis, _ = su.replay(log, n, m)
    E, basis_c = cu.restate(Tf, n, m, basis, nonbasis, rows)
    sm = _sm(cons, func)
    sm.solve(record_history=False, max_pivots=cap)
    assert sm.pivots == done
    ext = sm.add_constraints(rows)
    assert ext is not sm and ext.backend == "host" and ext.pivots == 0 and ext.status == "ready"
    assert (ext.n, ext.m) == (n + K, m) and ext.pivot_log == []
    assert ext.row == sm.row and ext.row is not sm.row
    assert ext.column == sm.column[:n] + [f"y{n + c + 1}" for c in range(K)] + ["f"]
    assert su.label_codes(ext.column[:-1], m) == basis_c.tolist()
    assert list(ext.function) == list(func)
    cu.same_table(ext._dev.download()[:n + K + 1, :m + 1], E, "add_constraints table")
    Tw, wst, wdone, wlog = c_oracle.run(E, n + K, m, m, cap)
    ext.solve(record_history=False, max_pivots=cap)
    assert ext.pivots == wdone and ext.pivot_log == [tuple(map(int, rc)) for rc in wlog]
    assert ext.status == {0: "cap", 1: "optimum", 2: "error", 3: "error"}[wst]
    wb, wn = cu.warm_labels(basis_c, nonbasis, wlog, n + K, m)
    su.same_solution(ext.solution(), cu.expected_solution(Tw, wb, wn, n + K, m, func, wdone),
                     "add_constraints solution")
    ru.same_ranges(ext.ranging(), ru.expected(Tw, wb, wn, n + K, m), "add_constraints ranging")
    _, cst, _, clog = c_oracle.run(cu.enlarged(T0, n, m, rows), n + K, m, m, cap)
    if wst == 1:
        assert cst == 1 and set(wb.tolist()) == set(su.replay(clog, n + K, m)[0].tolist())
    # the base object is untouched
    assert (sm.n, sm.pivots) == (n, done) and len(sm.column) == n + 1
    return wdone


def test_add_constraints_on_the_demo_lp():
    cons, func = DEMO
    sm = _sm(cons, func)
    sm.solve(record_history=False, max_pivots=64)
    x = sm.solution().x
    a = np.array([-1.0, -0.5])
    # the new row's value at the base answer is -0.5, then +0.5
    pivots = [_add_case(cons, func, 3, 2, [list(a) + [float(-(a @ x) - 0.5 * sign)]], 64)
              for sign in (1.0, -1.0)]
    assert sorted(pivots)[0] == 0 and sorted(pivots)[1] > 0   # one holds already, one cuts
    # before the first pivot: the caller's own lists under the identity labels
    ext = _sm(cons, func).add_constraints([[1.0, -0.0, 3.0]])
    cu.same_table(ext._dev.download()[:5, :3],
                  np.array(cons + [[1.0, -0.0, 3.0]] + [func + [0.0]]), "pristine")
    assert ext.column == ["y1", "y2", "y3", "y4", "f"]
    none = sm.add_constraints([])
    cu.same_table(none._dev.download()[:4, :3], sm._dev.download()[:4, :3], "no rows")
    assert none.column == sm.column and none.n == 3
    with pytest.raises(ValueError, match="coefficients and a constant"):
        sm.add_constraints([[1.0, 2.0]])


@pytest.mark.parametrize("k", (1, 3, 4))
def test_add_constraints_on_seeded_cases(k):
    _, n, m, seed, cap = ru.CASES[k]
    ref = ru.case(k)
    G = cu.cut_set(ref[0], n, m, seed, 0, 2, 0.05, cu.base_of_case(ref, n, m)[2])
    _add_case(ref[0][:n].tolist(), ref[0][n, :m].tolist(), n, m, G.tolist(), cap)


# ----------------------------------------------------------------------------------------------
# the C ABI and the Python arguments
def test_envelope_function():
    from simplex_mi355x import _lib
    from simplex_mi355x.batch import cuts_fits, warm_kernel
    L = _lib.load()
    for Rmax, ldb in ((2, 2), (2, 8190), (8190, 2), (4097, 4095)):
        assert L.smx_batch_cuts_fits(Rmax, ldb) == L.smx_batch_scenario_fits(Rmax, ldb) == 1
        assert cuts_fits(Rmax, ldb) is True
    for Rmax, ldb in ((1, 3), (2, 8191), (-1, 4)):
        assert L.smx_batch_cuts_fits(Rmax, ldb) == L.smx_batch_scenario_fits(Rmax, ldb) == 0
        assert cuts_fits(Rmax, ldb) is False
    assert cuts_fits(1 << 40, 2) is False
    # the warm tier: the first at or above the base tier that takes the enlarged block
    assert warm_kernel("wave", 64, 64) == "wave"
    assert warm_kernel("wave", 65, 64) == "workgroup"
    assert warm_kernel("workgroup", 64, 64) == "workgroup"
    assert warm_kernel("workgroup", 300, 300) == "global"
    assert warm_kernel("global", 10, 10) == "global"
    with pytest.raises(ValueError, match="envelope"):
        warm_kernel("wave", 725, 725)


def test_entry_points_refuse_bad_arguments_before_any_hip_call():
    """hipErrorInvalidValue (1) for a shape outside the envelope, a negative count, Rmax_out below
    Rmax, a count past 2^31 - 1 or a null pointer; B == 0 or S == 0 is a success without a launch.
    None of these reaches the HIP runtime."""
    from simplex_mi355x import _lib
    L = _lib.load()

    def call(B, S, Rmax, ldb, K, Rout):
        return L.smx_batch_cuts(None, None, B, S, Rmax, ldb, None, None, None, None, K, Rout,
                                None, None, None, None)
    assert call(0, 3, 4, 3, 2, 6) == 0
    assert call(5, 0, 4, 3, 2, 6) == 0
    assert call(-1, 3, 4, 3, 2, 6) == 1
    assert call(1, -3, 4, 3, 2, 6) == 1
    assert call(0, 3, 4, 3, -1, 6) == 1
    assert call(0, 3, 4, 3, 2, 3) == 1                       # Rmax_out < Rmax
    assert call(1 << 20, 1 << 12, 4, 3, 2, 6) == 1
    assert call(0, 3, 1, 3, 2, 6) == 1
    assert call(0, 3, 4, 8189, 2, 4) == 1
    assert call(0, 3, 4, 3, 2, 8190) == 1                    # the output block outside
    assert call(2, 3, 4, 3, 2, 6) == 1                       # null pointers with work to do
    assert L.smx_host_cuts(None, 3, 2, 2, None, None, None, 1, None, 3, None) == -1
    T = np.zeros((3, 3))
    lab = np.zeros(2, dtype=np.int32)
    G, E, bout = np.zeros((1, 3)), np.zeros((4, 3)), np.zeros(3, dtype=np.int32)
    args = (lab.ctypes.data, lab.ctypes.data, G.ctypes.data, 1, E.ctypes.data)
    assert L.smx_host_cuts(T.ctypes.data, 2, 2, 2, *args, 3, bout.ctypes.data) == -1
    assert L.smx_host_cuts(T.ctypes.data, 3, 2, 2, *args, 2, bout.ctypes.data) == -1
    assert L.smx_host_cuts(T.ctypes.data, 3, 0, 2, *args, 3, bout.ctypes.data) == -1
    assert L.smx_host_cuts(T.ctypes.data, 3, 2, 2, lab.ctypes.data, lab.ctypes.data, None, 1,
                           E.ctypes.data, 3, bout.ctypes.data) == -1
    assert L.smx_host_cuts(T.ctypes.data, 3, 2, 2, lab.ctypes.data, lab.ctypes.data,
                           G.ctypes.data, -1, E.ctypes.data, 3, bout.ctypes.data) == -1
    assert L.smx_host_cuts(T.ctypes.data, 3, 2, 2, *args, 3, bout.ctypes.data) == 0
    assert L.smx_host_cuts(T.ctypes.data, 3, 2, 2, lab.ctypes.data, lab.ctypes.data, None, 0,
                           E.ctypes.data, 3, bout.ctypes.data) == 0


def test_new_calls_refuse_before_any_device_call(monkeypatch):
    import torch
    from simplex_mi355x import batch
    tabs = np.zeros((1, 3, 3))
    tabs[0] = [[1.0, 1.0, 2.0], [1.0, -1.0, 1.0], [-1.0, -1.0, 0.0]]
    dims = np.array([[2, 2, 2]], dtype=np.int32)
    cuts, ncuts = np.zeros((1, 2, 2, 3)), np.zeros((1, 2), dtype=np.int32)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)

    def boom(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(torch, "from_numpy", boom)
    with pytest.raises(ValueError, match="cuts must be"):
        batch.solve_batch_cuts_arrays(tabs, dims, np.zeros((1, 2, 2, 4)), ncuts)
    with pytest.raises(ValueError, match="ncuts must be"):
        batch.solve_batch_cuts_arrays(tabs, dims, cuts, np.zeros((1, 3), dtype=np.int32))
    for bad in (-1, 3):
        with pytest.raises(ValueError, match="ncuts must lie in 0..K"):
            batch.solve_batch_cuts_arrays(tabs, dims, cuts, np.array([[0, bad]], dtype=np.int32))
    with pytest.raises(ValueError, match="kernel must be"):
        batch.solve_batch_cuts_arrays(tabs, dims, cuts, ncuts, kernel="lds")
    # without a device the new calls refuse like the rest of the batch path: no CPU fall-back
    with pytest.raises(RuntimeError, match="no CPU path"):
        batch.solve_batch_cuts_arrays(tabs, dims, cuts, ncuts)
    prob = ([[1.0, 1.0, 2.0]], [-1.0, -1.0])
    with pytest.raises(RuntimeError, match="no CPU path"):
        batch.solve_batch_cuts([prob], [[[[1.0, 0.0, 1.0]]]])
    with pytest.raises(ValueError, match="kernel must be"):
        batch.solve_batch_cuts([], [], kernel="lds")
    with pytest.raises(ValueError, match="one list of cut sets per problem"):
        batch.solve_batch_cuts([prob], [])
    with pytest.raises(ValueError, match="length of its problem's constraints"):
        batch.solve_batch_cuts([prob], [[[[1.0, 1.0]]]])
