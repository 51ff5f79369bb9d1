"""CPU: the dual-simplex selection rule (SMX_RULE_DUAL, include/smx.h) without a GPU -- dual_util's
restatement held to the C oracle on its reference branch, smx_host_select_rule / smx_host_run_rule
against the restatement by bit pattern, the hand-made one-step tables, what the rule means (a warm
run under it ends where the cold run of the changed problem ends, in dual steps only), the pinned
counts, SimplexMethod.solve(rule="dual") on the host backend and the refusals of the new
arguments before any device call."""
from __future__ import annotations

import numpy as np
import pytest

import cuts_util as cu
import dual_util as du
import ranging_util as ru
import scenario_util as scu
import solution_util as su

DEMO = ([[1.0, 1.0, -2.0], [-1.0, 1.0, 1.5], [1.0, -2.0, 4.0]], [-1.0, -1.0])
# the cases of ranging_util.CASES whose base run ends at `optimum` (ranging_util.OPTIMAL)
OPT = [k for k, c in enumerate(ru.CASES) if (c[1], c[2]) in ru.OPTIMAL]


def _ids(ks):
    return [f"{ru.CASES[k][0]}-{ru.CASES[k][1]}x{ru.CASES[k][2]}" for k in ks]


# ----------------------------------------------------------------------------------------------
# the restatement itself
@pytest.mark.parametrize("k", (0, 1, 2, 3, 4, 5, 9, 10), ids=_ids((0, 1, 2, 3, 4, 5, 9, 10)))
def test_the_reference_branch_is_the_oracle(k):
    """dual_util.run under the reference rule against c_oracle.run by bit pattern: log, status,
    pivot count and final table.  The dual branch then differs in the selection alone."""
    _, n, m, _, cap = ru.CASES[k]
    T0, flen, Tref, st, done, log = ru.case(k)
    got = du.run(T0, n, m, flen, cap, du.REFERENCE)
    du.same_run(got[:4], (Tref[:n + 1, :m + 1], st, done, log), ru.CASES[k])
    assert got[4] == 0


def test_the_reference_branch_is_the_oracle_on_the_fixtures_special_values():
    """The same on tables with NaN, inf and signed zeros: one pick each against c_oracle.pick."""
    from oracle import c_oracle
    import special_values as sv
    checked = 0
    n, m = 40, 40
    for name in sv.SCENARIOS:
        T = np.ascontiguousarray(sv.scenario(name, n, m, 5), dtype=np.float64)
        got = du.run(T, n, m, m, 6, du.REFERENCE)
        Tref, st, done, log = c_oracle.run(T, n, m, m, 6)
        assert got[1:3] == (st, done) and np.array_equal(got[3], log), name
        assert sv.same_bits_or_nan(got[0], Tref[:n + 1, :m + 1]), name
        checked += 1
    # the hand-made tables of this feature, too
    for case in du.handmade():
        name, T, n, m, flen, _, _ = case
        T = np.ascontiguousarray(T)
        st, r, c = c_oracle.pick(T, n, m, flen)
        got = du.select(T, n, m, flen, du.REFERENCE)
        assert got[0] == st, name
        if st == du.PIVOT:
            assert got[1:] == (r, c), name
        checked += 1
    assert checked >= len(du.handmade())


# ----------------------------------------------------------------------------------------------
# host twins against the restatement
def _warm_tables(k):
    """Warm tables of case k: three rhs-only scenarios and cut sets of one and two cuts."""
    _, n, m, seed, _ = ru.CASES[k]
    ref = ru.case(k)
    out = []
    for s in range(3):
        drhs, _, _, _, basis, nonbasis = scu.scenario_of_case(ref, n, m, seed, s, 0.2, 0.5)
        S, _ = scu.restate(ref[2], n, m, basis, nonbasis, ref[0][n, :m], drhs, np.zeros(m))
        out.append((f"scenario {s}", S, n))
    for s, K in ((0, 1), (1, 2)):
        _, E, _, _, _ = cu.cuts_of_case(ref, n, m, seed, s, K, viol=0.2)
        out.append((f"cuts {s}x{K}", E, n + K))
    return out


@pytest.mark.parametrize("k", OPT, ids=_ids(OPT))
def test_host_twins_on_warm_tables(k):
    _, n, m, _, _ = ru.CASES[k]
    dual_steps = 0
    for name, W, rows in _warm_tables(k):
        exp = du.run(W, rows, m, m, 512, du.DUAL)
        dual_steps += exp[4]
        assert exp[4] == exp[2], (ru.CASES[k], name, "a dual-feasible start takes dual steps only")
        for ld in (None, m + 1 + 5):
            du.same_run(du.host_run(W, rows, m, m, 512, du.DUAL, ld=ld), exp[:4],
                        (ru.CASES[k], name, ld))
        assert du.host_select(W, rows, m, m, du.DUAL, ld=m + 4) == du.select(W, rows, m, m, du.DUAL)
        # a cap inside the run: SMX_IDLE at the C ABI, reported as the cap
        if exp[2] > 1:
            part = du.run(W, rows, m, m, exp[2] - 1, du.DUAL)
            assert part[1] == du.PIVOT
            du.same_run(du.host_run(W, rows, m, m, exp[2] - 1, du.DUAL), part[:4], (name, "cap"))
    assert dual_steps > 0, ru.CASES[k]


HANDMADE = du.handmade()


@pytest.mark.parametrize("case", HANDMADE, ids=[c[0] for c in HANDMADE])
def test_handmade_one_step_tables(case):
    name, T, n, m, flen, want, dual = case
    du.check_handmade(case)
    assert du.host_select(T, n, m, flen, du.DUAL) == want, name
    assert du.host_select(T, n, m, flen, du.DUAL, ld=m + 7) == want, name
    du.same_run(du.host_run(T, n, m, flen, 1, du.DUAL), du.run(T, n, m, flen, 1, du.DUAL)[:4], name)
    if not dual:       # the reference's step, bit for bit
        du.same_run(du.host_run(T, n, m, flen, 1, du.DUAL),
                    du.host_run(T, n, m, flen, 1, du.REFERENCE), name)


def test_handmade_tables_hold_their_events():
    names = [c[0] for c in HANDMADE]
    assert len(set(names)) == len(names) >= 12
    assert sum(c[6] for c in HANDMADE) >= 9 and sum(not c[6] for c in HANDMADE) >= 3
    assert any(c[5][0] == du.INCORRECT for c in HANDMADE)
    assert all(c[5][1] in (2, du.NONE) for c in HANDMADE)     # nb is not row 0
    # the rules differ on them: the reference's first positive entry is another column somewhere
    differ = [c[0] for c in HANDMADE
              if c[6] and du.select(c[1], c[2], c[3], c[4], du.REFERENCE) != c[5]]
    assert len(differ) >= 5, differ
    # other placements of the same events (the GPU tests use them)
    for cols in ((5, 4, 3, 2, 1, 0), (0, 5, 2, 4, 1, 3)):
        for case in du.handmade(7, 6, 4, cols):
            du.check_handmade(case)
            assert du.host_select(case[1], 7, 6, case[4], du.DUAL) == case[5], (cols, case[0])


@pytest.mark.parametrize("k", (0, 1, 3, 10), ids=_ids((0, 1, 3, 10)))
def test_rule_zero_is_the_entry_without_a_rule(k):
    _, n, m, _, cap = ru.CASES[k]
    T0 = ru.case(k)[0]
    a = du.host_run(T0, n, m, m, cap, du.REFERENCE, ld=m + 3)
    b = du.host_run(T0, n, m, m, cap, du.REFERENCE, ld=m + 3, entry="smx_host_run")
    du.same_run(a, b, ru.CASES[k])
    for name, W, rows in _warm_tables(1):
        du.same_run(du.host_run(W, rows, 7, 7, 64, du.REFERENCE),
                    du.host_run(W, rows, 7, 7, 64, du.REFERENCE, entry="smx_host_run"), name)


def test_host_entries_refuse_an_unknown_rule():
    import ctypes
    from simplex_mi355x import _lib
    L = _lib.load()
    T = np.array([[1.0, 1.0, -2.0], [1.0, 1.0, 0.0]])
    buf = np.zeros((2, 2, 3))
    buf[0] = T
    before = buf.copy()
    shape = _lib.Shape(3, 1, 1, 2, 2, 0, 1)
    rc = np.full(2, 9, dtype=np.int32)
    st = ctypes.c_int32(77)
    for rule in (2, -1, 1 << 20):
        assert L.smx_host_select_rule(buf[0].ctypes.data, ctypes.byref(shape), rule,
                                      rc.ctypes.data) == -1
        assert L.smx_host_run_rule(buf[0].ctypes.data, buf[1].ctypes.data, ctypes.byref(shape), 0,
                                   4, rule, None, ctypes.byref(st)) == -1
    assert rc.tolist() == [9, 9] and st.value == 77 and np.array_equal(buf, before)
    assert _lib.rule_code("reference") == 0 and _lib.rule_code("dual") == 1
    for bad in ("Dual", "", None, 1, "primal"):
        with pytest.raises(ValueError, match="rule must be"):
            _lib.rule_code(bad)


# ----------------------------------------------------------------------------------------------
# what the rule means: the oracle and the restatement only
def _perturbed(T0, n, m, drhs, dcost):
    P = np.array(T0, dtype=np.float64)
    P[:n, m] = np.where(drhs != 0, P[:n, m] + drhs, P[:n, m])
    P[n, :m] = np.where(dcost != 0, P[n, :m] + dcost, P[n, :m])
    return P


def _close(a, b):
    return abs(a - b) <= 1e-9 * max(abs(a), abs(b))


def _bases(cap=256):
    """The 158 uniform LPs of seeds 0..199 (n = 3 + seed % 9, m = 2 + seed % 5) whose base run
    ends at `optimum`: (seed, n, m, T0, final, basis, nonbasis, x)."""
    from oracle import c_oracle
    from simplex_mi355x import lp
    for seed in range(200):
        n, m = 3 + seed % 9, 2 + seed % 5
        T0 = lp.dense_tableau("uniform", seed, n, m)
        Tf, st, _, log = c_oracle.run(T0, n, m, m, cap)
        if st != 1:
            continue
        basis, nonbasis, _ = su.replay(log, n, m)
        yield seed, n, m, T0, Tf, basis, nonbasis, su.expected(Tf, log, n, m, T0[n]).x


def _scenario_census(with_costs):
    from oracle import c_oracle
    by_status = {0: 0, 1: 0, 2: 0, 3: 0}
    pairs = dual = steps = steps_all = cold = ref = 0
    worst = 0.0
    for seed, n, m, T0, Tf, basis, nonbasis, _ in _bases():
        for s in range(4):
            drhs, dcost = scu.deltas(T0, n, m, seed, s, 0.5, 0.5)
            if not with_costs:
                dcost = np.zeros(m)
            S, func_s = scu.restate(Tf, n, m, basis, nonbasis, T0[n, :m], drhs, dcost)
            Tw, wst, wdone, wlog, wdual = du.run(S, n, m, m, 256, du.DUAL)
            Tc, cst, cdone, clog = c_oracle.run(_perturbed(T0, n, m, drhs, dcost), n, m, m, 256)
            assert wst == cst, (seed, s, wst, cst)
            if not with_costs:
                assert wdual == wdone, (seed, s, "a dual-feasible start takes dual steps only")
            pairs += 1
            by_status[wst] += 1
            steps_all += wdual
            if wst == 1:
                wb, wn = scu.warm_labels(basis, nonbasis, wlog, n, m)
                a = scu.expected_solution(Tw, wb, wn, n, m, func_s, wdone).objective
                b = su.expected(Tc, clog, n, m, func_s).objective
                assert _close(a, b), (seed, s, a, b)
                worst = max(worst, abs(a - b) / max(abs(a), abs(b), 1e-300))
                dual += wdone
                steps += wdual
                cold += cdone
                _, rst, rdone, _ = c_oracle.run(S, n, m, m, 256)
                ref += rdone if rst == 1 else 0
    return pairs, by_status, dual, steps, steps_all, cold, worst, ref


def test_rhs_only_scenarios_end_where_the_cold_run_ends():
    """Seeds 0..199, scenarios 0..3 at frac 0.5, prob 0.5 with their cost deltas zeroed, cap 256:
    the warm run under the dual rule and the oracle's cold run of the perturbed original end with
    the same status in all 632 pairs, at `optimum` with objectives within 1e-9 relative, and every
    warm run takes dual steps only.  The counts are pinned: pivots of the runs that end at
    `optimum` under the dual rule (warm), and of the cold runs of the same pairs."""
    pairs, by_status, dual, steps, steps_all, cold, worst, ref = _scenario_census(False)
    assert pairs == 632
    assert (by_status[1], by_status[2], by_status[3], by_status[0]) == (588, 44, 0, 0)
    assert (dual, steps, cold) == (189, 189, 1528)
    assert ref == 356                 # the reference rule's warm pivots on the same 588 pairs
    assert steps_all == 246           # the 44 runs that end at "incorrect system" included
    assert worst < 1e-11


def test_scenarios_with_cost_deltas_end_where_the_cold_run_ends():
    """The same scenarios with their cost deltas: a table with a negative f-row entry takes the
    reference's steps until it is dual feasible or primal feasible, so the rule promises no more
    than the reference's there -- on these 632 pairs every status is still the cold run's.  Of the
    359 pivots of the runs that end at `optimum` 137 are dual steps; over all 632 runs 187 are."""
    pairs, by_status, dual, steps, steps_all, cold, worst, _ = _scenario_census(True)
    assert pairs == 632
    assert (by_status[1], by_status[2], by_status[3], by_status[0]) == (581, 44, 7, 0)
    assert (dual, steps, steps_all, cold) == (359, 137, 187, 1535)
    assert worst < 1e-11


@pytest.mark.parametrize("K,viol,want", ((1, 0.05, (577, 55)), (2, 0.2, (410, 222))),
                         ids=("one-cut-5pct", "two-cuts-20pct"))
def test_cut_sets_end_where_the_cold_run_ends(K, viol, want):
    """Seeds 0..199, cut sets 0..3 of K cuts, cap 512: the warm run under the dual rule on the
    extended table and the oracle's cold run of the enlarged original end with the same status in
    all 632 pairs, at `optimum` with objectives within 1e-9 relative; every warm run takes dual
    steps only (an extended table keeps its base run's f-row).  Status counts pinned."""
    from oracle import c_oracle
    by_status = {0: 0, 1: 0, 2: 0, 3: 0}
    pairs = 0
    for seed, n, m, T0, Tf, basis, nonbasis, x in _bases():
        for s in range(4):
            G = cu.cut_set(T0, n, m, seed, s, K, viol, x)
            E, basis_c = cu.restate(Tf, n, m, basis, nonbasis, G)
            Tw, wst, wdone, wlog, wdual = du.run(E, n + K, m, m, 512, du.DUAL)
            Tc, cst, cdone, clog = c_oracle.run(cu.enlarged(T0, n, m, G), n + K, m, m, 512)
            assert wst == cst, (seed, s, wst, cst)
            assert wdual == wdone, (seed, s)
            pairs += 1
            by_status[wst] += 1
            if wst == 1:
                wb, wn = cu.warm_labels(basis_c, nonbasis, wlog, n + K, m)
                a = cu.expected_solution(Tw, wb, wn, n + K, m, T0[n, :m], wdone).objective
                b = su.expected(Tc, clog, n + K, m, T0[n]).objective
                assert _close(a, b), (seed, s, a, b)
    assert pairs == 632
    assert (by_status[1], by_status[2], by_status[0], by_status[3]) == (*want, 0, 0)


def test_the_case_the_reference_rule_does_not_finish():
    """Uniform 60 x 12, seed 5, scenario 1 at frac 0.2, prob 0.5, cost deltas zeroed (the LP of
    test_scenario.py::test_the_fallback_case_exists_on_the_oracle): the reference rule is still
    pivoting at cap 512, the dual rule reaches `optimum` after 2 pivots, both dual steps, the cold
    run after 22, with the same objective.  With the scenario's cost deltas kept the table is not
    dual feasible: no dual step is taken and the run is the reference's, still at the cap."""
    from oracle import c_oracle
    from simplex_mi355x import lp
    n, m, seed = 60, 12, 5
    T0 = lp.dense_tableau("uniform", seed, n, m)
    Tf, st, done, log = c_oracle.run(T0, n, m, m, 256)
    assert (st, done) == (1, 12)
    basis, nonbasis, _ = su.replay(log, n, m)
    drhs, dcost = scu.deltas(T0, n, m, seed, 1, 0.2, 0.5)
    zero = np.zeros(m)
    S, func_s = scu.restate(Tf, n, m, basis, nonbasis, T0[n, :m], drhs, zero)
    _, rst, rdone, _ = c_oracle.run(S, n, m, m, 512)
    assert (rst, rdone) == (0, 512)
    Tw, wst, wdone, wlog, wdual = du.run(S, n, m, m, 512, du.DUAL)
    assert (wst, wdone, wdual) == (1, 2, 2)
    Tc, cst, cdone, clog = c_oracle.run(_perturbed(T0, n, m, drhs, zero), n, m, m, 512)
    assert (cst, cdone) == (1, 22)
    wb, wn = scu.warm_labels(basis, nonbasis, wlog, n, m)
    a = scu.expected_solution(Tw, wb, wn, n, m, func_s, wdone).objective
    b = su.expected(Tc, clog, n, m, func_s).objective
    assert _close(a, b) and abs(a - b) <= 1e-14 * abs(b)
    du.same_run(du.host_run(S, n, m, m, 512, du.DUAL), (Tw, wst, wdone, wlog), "60 x 12")
    # the cost-delta form
    S2, _ = scu.restate(Tf, n, m, basis, nonbasis, T0[n, :m], drhs, dcost)
    assert (S2[n, :m] < 0).any()
    T2, st2, done2, log2, dual2 = du.run(S2, n, m, m, 512, du.DUAL)
    assert (st2, done2, dual2) == (0, 512, 0)
    Tr, _, _, rlog = c_oracle.run(S2, n, m, m, 512)
    du.same_run((T2, st2, done2, log2), (Tr[:n + 1, :m + 1], 0, 512, rlog), "cost-delta form")


# ----------------------------------------------------------------------------------------------
# SimplexMethod on the host backend
def _sm(cons, func):
    import simplex
    sm = simplex.SimplexMethod([list(r) for r in cons], list(func), device="cpu")
    assert sm.backend == "host"
    return sm


STATUS = {0: "cap", 1: "optimum", 2: "error", 3: "error"}


def _solved_like(warm, exp, labels0, rows, m, func, what):
    """A SimplexMethod after solve(rule="dual") against the restatement's run `exp` from the
    start labels `labels0`: log, status, pivots, labels, solution(), ranging()."""
    Tw, wst, wdone, wlog, _ = exp
    assert warm.pivots == wdone, what
    assert warm.pivot_log == [tuple(map(int, rc)) for rc in wlog], what
    assert warm.status == STATUS[wst], what
    wb, wn = scu.warm_labels(labels0[0], labels0[1], wlog, rows, m)
    assert su.label_codes(warm.column[:-1], m) == wb.tolist(), what
    assert su.label_codes(warm.row[:-1], m) == wn.tolist(), what
    scu.same_table(warm._dev.download()[:rows + 1, :m + 1], Tw, what)
    su.same_solution(warm.solution(), scu.expected_solution(Tw, wb, wn, rows, m, func, wdone), what)
    ru.same_ranges(warm.ranging(), ru.expected(Tw, wb, wn, rows, m), what)


def _warm_case(cons, func, n, m, drhs, rows_added, cap):
    """what_if(drhs).solve(rule="dual") and add_constraints(rows).solve(rule="dual") after a base
    solve on the host engine; returns the dual steps of both."""
    from oracle import c_oracle
    T0 = np.zeros((n + 1, m + 1))
    T0[:n] = cons
    T0[n, :m] = func
    Tf, _, done, log = c_oracle.run(T0, n, m, m, cap)
    basis, nonbasis, _ = su.replay(log, n, m)
    sm = _sm(cons, func)
    sm.solve(record_history=False, max_pivots=cap)
    assert sm.pivots == done
    S, func_s = scu.restate(Tf, n, m, basis, nonbasis, func, drhs, np.zeros(m))
    exp = du.run(S, n, m, m, cap, du.DUAL)
    wi = sm.what_if(drhs)
    out = wi.solve(record_history=False, max_pivots=cap, rule="dual")
    assert len(out) >= 2
    _solved_like(wi, exp, (basis, nonbasis), n, m, func_s, "what_if")
    K = len(rows_added)
    E, basis_c = cu.restate(Tf, n, m, basis, nonbasis, rows_added)
    exp2 = du.run(E, n + K, m, m, cap, du.DUAL)
    ac = sm.add_constraints(rows_added)
    ac.solve(record_history=False, max_pivots=cap, rule="dual")
    _solved_like(ac, exp2, (basis_c, nonbasis), n + K, m, np.asarray(func, dtype=np.float64),
                 "add_constraints")
    # step by step (pick_element / step with a rule) walks the same pivots
    st = sm.what_if(drhs)
    for r, c in exp[3]:
        ok, pr, pc, _ = st.pick_element(rule="dual")
        assert ok and (pr, pc) == (int(r), int(c))
        st.step(rule="dual")
    assert st.pivot_log == [tuple(map(int, rc)) for rc in exp[3]]
    # the history form
    hist = sm.what_if(drhs).get_solution(max_pivots=cap, rule="dual")
    assert sum(1 for h in hist if getattr(h, "i", None) is not None) == exp[2]
    assert sm.pivots == done                                 # the base object is untouched
    return exp[4], exp2[4]


def test_simplex_method_dual_on_the_demo_lp():
    cons, func = DEMO
    # the demo's rhs range of constraint 0 ends at -10.5 (test_ranging.py): at -12 the third row's
    # constant is negative and the row holds no positive entry -- "incorrect system" at once, under
    # either rule; the cut x1 <= 3 takes one dual step to its optimum
    d1, d2 = _warm_case(cons, func, 3, 2, [-12.0, 0.0, 0.0], [[-1.0, 0.0, 3.0]], 64)
    assert (d1, d2) == (0, 1)
    # inside the range nothing pivots; a cut that holds at the optimum adds nothing
    assert _warm_case(cons, func, 3, 2, [0.0, -3.0, 0.0], [[1.0, 0.0, -3.0]], 64) == (0, 0)


@pytest.mark.parametrize("k", (1, 9), ids=_ids((1, 9)))
def test_simplex_method_dual_on_seeded_cases(k):
    _, n, m, seed, cap = ru.CASES[k]
    ref = ru.case(k)
    drhs, _ = scu.deltas(ref[0], n, m, seed, 0, 0.5, 0.5)
    _, _, x = cu.base_of_case(ref, n, m)
    G = cu.cut_set(ref[0], n, m, seed, 0, 2, 0.2, x)
    d1, d2 = _warm_case(ref[0][:n].tolist(), ref[0][n, :m].tolist(), n, m, drhs, G.tolist(), cap)
    assert d1 + d2 > 0


def test_simplex_method_dual_keeps_the_int_first_pivot():
    """A pristine int table under rule="dual": the first pivot runs alone and gets the int fix,
    which does not depend on how (r, c) was chosen -- the table after it equals the one a forced
    pivot of the same (r, c) gives an int table under the reference protocol."""
    import simplex
    cons = [[2, -1, 0, -4], [1, 3, -2, 6], [0, 1, 1, -3]]
    func = [3, 0, 2]
    sm = simplex.SimplexMethod([list(r) for r in cons], list(func), device="cpu")
    exp = du.run(np.array(cons + [func + [0]], dtype=np.float64), 3, 3, 3, 16, du.DUAL)
    assert exp[4] > 0                                        # it starts with a dual step
    sm.solve(record_history=False, max_pivots=16, rule="dual")
    assert sm.pivot_log == [tuple(map(int, rc)) for rc in exp[3]]
    assert sm.status == STATUS[exp[1]]
    got = sm._dev.download()[:4, :4]
    assert np.array_equal(got, exp[0])                       # equal values; zero signs by the fix
    other = simplex.SimplexMethod([list(r) for r in cons], list(func), device="cpu")
    other.step(rule="dual")
    assert other.pivot_log == sm.pivot_log[:1] and other._int0 is None


def test_unknown_rules_are_refused(monkeypatch):
    import torch
    from simplex_mi355x import batch
    sm = _sm(*DEMO)
    for call in (lambda: sm.solve(rule="primal"), lambda: sm.step(rule="Dual"),
                 lambda: sm.pick_element(rule=None), lambda: sm.get_solution(rule=1)):
        with pytest.raises(ValueError, match="rule must be"):
            call()
    assert sm.pivots == 0 and sm.status == "ready"
    tabs = np.zeros((1, 3, 3))
    tabs[0] = [[1.0, 1.0, 2.0], [1.0, -1.0, 1.0], [-1.0, -1.0, 0.0]]
    dims = np.array([[2, 2, 2]], dtype=np.int32)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)

    def boom(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(torch, "from_numpy", boom)
    prob = [([[1.0, 1.0, 2.0]], [-1.0, -1.0])]
    calls = (
        lambda r: batch.solve_batch_arrays(tabs, dims, rule=r),
        lambda r: batch.solve_batch(prob, rule=r),
        lambda r: batch.solve_batch_solutions(prob, rule=r),
        lambda r: batch.solve_batch_ranges(prob, rule=r),
        lambda r: batch.solve_batch_scenarios_arrays(tabs, dims, np.zeros((1, 1, 2)),
                                                     np.zeros((1, 1, 2)), warm_rule=r),
        lambda r: batch.solve_batch_scenarios(prob, [[(None, None)]], warm_rule=r),
        lambda r: batch.solve_batch_cuts_arrays(tabs, dims, np.zeros((1, 1, 1, 3)),
                                                np.zeros((1, 1), dtype=np.int32), warm_rule=r),
        lambda r: batch.solve_batch_cuts(prob, [[[]]], warm_rule=r),
    )
    for call in calls:
        with pytest.raises(ValueError, match="rule must be"):
            call("primal")
        # a good rule gets as far as the device question: there is no CPU path
        with pytest.raises(RuntimeError, match="no CPU path"):
            call("dual")


def test_batch_rule_entries_refuse_before_any_hip_call():
    """The `_rule` entries with null pointers: an unknown rule, and every refusal and the B == 0
    answer of the entries without a rule, under both rules.  None reaches the HIP runtime."""
    from simplex_mi355x import _lib
    L = _lib.load()
    null = [None] * 6
    for name, ok_shape, bad_shapes in (
            ("smx_batch_solve", (4, 3), ((0, 3), (65, 3), (4, 0), (4, 65))),
            ("smx_batch_solve_wg", (70, 70), ((1, 3), (3, 1), (400, 400))),
            ("smx_batch_solve_gm", (300, 300), ((1, 3), (3, 1), (8000, 300), (800, 800)))):
        plain, ruled = getattr(L, name), getattr(L, name + "_rule")
        for rule in (0, 1):
            assert ruled(None, None, 0, *ok_shape, 8, *null, rule, None) == 0
            assert ruled(None, None, -1, *ok_shape, 8, *null, rule, None) == 1
            assert ruled(None, None, 0, *ok_shape, -1, *null, rule, None) == 1
            for shp in bad_shapes:
                assert ruled(None, None, 0, *shp, 8, *null, rule, None) == 1, (name, shp, rule)
                assert plain(None, None, 0, *shp, 8, *null, None) == 1, (name, shp)
        for rule in (2, -1, 7):
            assert ruled(None, None, 0, *ok_shape, 8, *null, rule, None) == 1
            assert ruled(None, None, 5, *ok_shape, 8, *null, rule, None) == 1
