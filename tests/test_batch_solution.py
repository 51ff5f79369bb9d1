"""CPU: the whole-solution surface without a GPU -- the envelope of k_batch_solution as the library
states it, SimplexMethod.solution() on the host engine against the reference's recorded answers
and against solution_util on the C oracle's tables, and the refusal of the new batch arguments
before any device call."""
from __future__ import annotations

import numpy as np
import pytest

import solution_util as su
from golden_util import dec, dec_input, load, same_value, trajectory_cap, trajectory_cases


def _sm(cons, func):
    import simplex
    sm = simplex.SimplexMethod([list(r) for r in cons], list(func), device="cpu")
    assert sm.backend == "host"
    return sm


def test_envelope_function():
    from simplex_mi355x import _lib
    from simplex_mi355x.batch import solution_lds_bytes
    L = _lib.load()
    for Rmax, ldb in ((2, 2), (64, 64), (725, 725), (2, 8190)):
        assert L.smx_batch_solution_lds_bytes(Rmax, ldb) == 16 * (Rmax + ldb), (Rmax, ldb)
        assert solution_lds_bytes(Rmax, ldb) == 16 * (Rmax + ldb)
    for Rmax, ldb in ((2, 8191), (1, 5), (5, 1), (8191, 2), (0, 0), (-3, 9)):
        assert L.smx_batch_solution_lds_bytes(Rmax, ldb) == -1, (Rmax, ldb)
    assert solution_lds_bytes(1 << 40, 2) == -1
    assert L.smx_batch_solution_lds_bytes(2, 8190) == 128 * 1024


def test_entry_point_refuses_bad_arguments_before_any_hip_call():
    """hipErrorInvalidValue (1) for a shape outside the envelope, a negative count or a null
    pointer; B == 0 is a success without a launch.  None of these reaches the HIP runtime, so they
    run on a machine without a device."""
    from simplex_mi355x import _lib
    L = _lib.load()
    null = [None] * 8
    assert L.smx_batch_solution(None, None, 0, 4, 3, 8, *null, None) == 0
    assert L.smx_batch_solution(None, None, 0, 1, 3, 8, *null, None) == 1
    assert L.smx_batch_solution(None, None, 0, 2, 8191, 8, *null, None) == 1
    assert L.smx_batch_solution(None, None, -1, 4, 3, 8, *null, None) == 1
    assert L.smx_batch_solution(None, None, 0, 4, 3, -1, *null, None) == 1
    assert L.smx_batch_solution(None, None, 2, 4, 3, 8, *null, None) == 1


def _check_against_recorded(sm, cons, func, last, row, column, what):
    n, m = len(cons), len(cons[0]) - 1
    sol = sm.solution()
    ints = any(isinstance(v, int) for r in (*cons, func) for v in r)
    assert sol.x.shape == (m,) and sol.duals.shape == (n,)
    assert sol.basis.tolist() == su.label_codes(column[:-1], m), what
    assert sol.nonbasis.tolist() == su.label_codes(row[:-1], m), what
    # the reference reports a non-basic variable as the int 0 and int inputs keep int arithmetic
    # at the start, so on those the sign of a zero is its own; values compare exactly otherwise
    assert same_value(float(sol.x[0]), dec(last["x1"]), signed_zero=False), what
    if m >= 2:
        assert same_value(float(sol.x[1]), dec(last["x2"]), signed_zero=False), what
    # (snapshot #0 of get_solution records the literal 0, 0, 0, not f(x1, x2): simplex.py:181)
    if m == 2 and sm.pivots > 0:
        assert same_value(sol.objective, dec(last["optimum"]), signed_zero=not ints), what
    assert sol.pivots == sm.pivots
    # and the definition itself, on this engine's own final table
    exp = su.expected(sm._dev.download(), sm.pivot_log, n, m, func)
    su.same_solution(sol, exp, what, nan_aware=True)


@pytest.mark.parametrize("name", list(load("examples.json")))
def test_host_solution_on_examples(name):
    case = load("examples.json")[name]
    cons, func = dec_input(case["input"])
    sm = _sm(cons, func)
    sm.get_solution()
    last = [e for e in case["solution"] if e["kind"] == "info"][-1]
    _check_against_recorded(sm, cons, func, last, last["row"], last["column"], name)


def _fixture_cases():
    """A dozen random.json trajectories and every edge.json one that ends without the reference's
    IndexError (the objective needs function[0..m-1])."""
    picks = [c for c in trajectory_cases() if c[0].startswith("random")][:12]
    picks += [c for c in trajectory_cases() if c[0].startswith("edge_")]
    return [c for c in picks if c[3]["outcome"]["kind"] != "exception"
            and len(c[2]) >= len(c[1][0]) - 1]


FIXTURES = _fixture_cases()


@pytest.mark.parametrize("case", FIXTURES, ids=[c[0] for c in FIXTURES])
def test_host_solution_on_fixtures(case):
    label, cons, func, rec = case
    sm = _sm(cons, func)
    sm.get_solution(max_pivots=trajectory_cap(rec))
    assert sm.row == rec["row"] and sm.column == rec["column"], label
    _check_against_recorded(sm, cons, func, rec["steps"][-1], rec["row"], rec["column"], label)


def test_fixture_cases_cover_the_shapes():
    ms = {len(cons[0]) - 1 for _, cons, _, _ in FIXTURES}
    assert 2 in ms and max(ms) > 2
    kinds = {rec["outcome"]["kind"] for _, _, _, rec in FIXTURES}
    assert {"optimum", "error"} <= kinds


def test_pristine_solution_is_all_zero_with_pythons_sign():
    sm = _sm([[1.0, 1.0, -2.0], [-1.0, 1.0, 1.5], [1.0, -2.0, 4.0]], [-1.0, -1.0])
    sol = sm.solution()
    assert sol.pivots == 0
    assert sol.basis.tolist() == [2, 3, 4] and sol.nonbasis.tolist() == [0, 1]
    assert not su.bits(sol.x).any() and not su.bits(sol.duals).any()          # all +0.0
    assert su.same_floats(sol.objective, -1.0 * 0.0 + -1.0 * 0.0)
    assert np.signbit(sol.objective)
    sol = _sm([[1.0, 1.0, -2.0]], [1.0, -1.0]).solution()
    assert su.same_floats(sol.objective, 1.0 * 0.0 + -1.0 * 0.0) and not np.signbit(sol.objective)
    sol = _sm([[3.0, -2.0]], [-4.0, 9.0]).solution()                 # m == 1: p[0] alone
    assert sol.x.shape == (1,) and su.same_floats(sol.objective, -0.0)


def test_solution_after_the_table_is_set_again_reads_the_callers_lists():
    """`table = ...` puts the caller's lists back (pristine) and keeps the labels where they
    stood: solution() then reads those lists, as find_optimum does."""
    cons = [[1.0, 1.0, -2.0], [-1.0, 1.0, 1.5], [1.0, -2.0, 4.0]]
    func = [-1.0, -1.0]
    sm = _sm(cons, func)
    sm.step()
    labels = (list(sm.row), list(sm.column))
    table = [[2.0, 3.0, 5.0], [7.0, 11.0, 13.0], [17.0, 19.0, 23.0], [29.0, 31.0]]
    sm.table = table
    assert (sm.row, sm.column) == labels and labels[1][0] == "x1"
    sol = sm.solution()
    x1, x2 = sm.find_optimum()
    assert (sol.x[0], sol.x[1]) == (x1, x2) == (5.0, 0)
    assert sol.duals.tolist() == [29.0, 0.0, 0.0] and sol.objective == -5.0


def test_solution_before_and_after_each_step_follows_the_labels():
    """x labels enter and leave the basis again on the demo LP; solution() after every step
    equals the definition on that step's table."""
    cons = [[1.0, 1.0, -2.0], [-1.0, 1.0, 1.5], [1.0, -2.0, 4.0]]
    func = [-1.0, -1.0]
    sm = _sm(cons, func)
    while sm.step()[0]:
        exp = su.expected(sm._dev.download(), sm.pivot_log, 3, 2, func)
        su.same_solution(sm.solution(), exp, sm.pivots)
    x1, x2 = sm.find_optimum()
    sol = sm.solution()
    assert (float(sol.x[0]), float(sol.x[1]), sol.objective) == (x1, x2, sm.f(x1, x2))
    assert (x1, x2, sol.objective) == (7.0, 5.5, -12.5)


def test_sharp_cases_keep_their_edge():
    """The inputs of the GPU tests: ordered sums that differ from numpy's, x labels that leave."""
    su.check_sharp_cases()


@pytest.mark.parametrize("k", range(len(su.SHARP)), ids=[f"{c[0]}-{c[1]}x{c[2]}-s{c[3]}"
                                                         for c in su.SHARP])
def test_host_solution_on_sharp_cases(k):
    """The host engine's chained loop, then solution(): against solution_util on the C oracle's
    final table, bit for bit -- the ordered objective included."""
    kind, n, m, seed, cap, _ = su.SHARP[k]
    ref = su.sharp_case(k)
    T = ref[0]
    sm = _sm(T[:n].tolist(), T[n, :m].tolist())
    sm.solve(record_history=False, max_pivots=cap)
    assert sm.pivot_log == [tuple(map(int, rc)) for rc in ref[5]]
    su.same_solution(sm.solution(), su.of_case(ref, n, m), su.SHARP[k])


def test_function_with_m_plus_1_entries_ignores_the_last():
    T = su.sharp_case(2)[0]
    n = m = 20
    a = _sm(T[:n].tolist(), T[n, :m].tolist())
    b = _sm(T[:n].tolist(), T[n, :m].tolist() + [123.0])
    for sm in (a, b):
        sm.solve(record_history=False, max_pivots=10)
    assert a.pivot_log == b.pivot_log
    sa, sb = a.solution(), b.solution()
    assert su.same_floats(sa.objective, sb.objective) and su.same_floats(sa.x, sb.x)


def test_new_arguments_are_refused_before_any_device_call(monkeypatch):
    import torch
    from simplex_mi355x import batch
    tabs = np.zeros((1, 3, 3))
    tabs[0] = [[1.0, 1.0, 2.0], [1.0, -1.0, 1.0], [-1.0, -1.0, 0.0]]
    dims = np.array([[2, 2, 2]], dtype=np.int32)
    with pytest.raises(ValueError, match="solution=True"):
        batch.solve_batch_arrays(tabs, dims, tables=False)
    with pytest.raises(ValueError, match="history"):
        batch.solve_batch_arrays(tabs, dims, history=True, solution=True, tables=False)
    # without a device the new mode refuses like the rest of the batch path: no CPU fall-back
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)

    def boom(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(torch, "from_numpy", boom)
    with pytest.raises(RuntimeError, match="no CPU path"):
        batch.solve_batch_arrays(tabs, dims, solution=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        batch.solve_batch_arrays(tabs, dims, solution=True, tables=False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        batch.solve_batch_solutions([([[1.0, 1.0, 2.0]], [-1.0, -1.0])])
    with pytest.raises(ValueError, match="kernel must be"):
        batch.solve_batch_solutions([], kernel="lds")
