"""GPU: the form of what the three array-level batch calls return -- the keys, their order and
every array's shape and dtype -- for every legal combination of the switches, for a call with no
sets (S == 0) and for a call with no problems (B == 0).  What the arrays hold is the business of
test_gpu_batch_solution, _ranging, _scenarios and _cuts; here one 2 x 2 LP is enough."""
from __future__ import annotations

import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAP = 4
F8, I4 = np.dtype(np.float64), np.dtype(np.int32)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def _lps(B):
    """B copies of the 2 x 2 LP of test_batch_solution (the second with another constant)."""
    tabs = np.zeros((B, 3, 3))
    for q in range(B):
        tabs[q] = [[1.0, 1.0, 2.0 + q], [1.0, -1.0, 1.0], [-1.0, -1.0, 0.0]]
    return tabs, np.full((B, 3), 2, dtype=np.int32)


def _answer_form(lead, rows, cols, ranging):
    """name -> (shape, dtype) of the solution arrays (and the range arrays) of blocks of `rows`
    rows and `cols` columns, in the order the calls return them."""
    form = {"x": ((*lead, cols - 1), F8), "duals": ((*lead, rows - 1), F8),
            "objective": (lead, F8), "basis": ((*lead, rows - 1), I4),
            "nonbasis": ((*lead, cols - 1), I4)}
    if ranging:
        form.update({"rhs_lo": ((*lead, rows - 1), F8), "rhs_hi": ((*lead, rows - 1), F8),
                     "cost_lo": ((*lead, cols - 1), F8), "cost_hi": ((*lead, cols - 1), F8)})
    return form


def _base_form(B, ranging, solution=True, tables=False):
    form = {"final": ((B, 3, 3), F8)} if tables else {}
    form.update({"rc": ((B, CAP, 2), I4), "xv": ((B, CAP, 2), F8), "status": ((B,), I4),
                 "npivots": ((B,), I4)})
    if solution:
        form.update(_answer_form((B,), 3, 3, ranging))
    return form


def _same_form(got, form, what):
    assert list(got) == list(form), what
    for key, (shape, dtype) in form.items():
        assert isinstance(got[key], np.ndarray), (what, key)
        assert got[key].shape == tuple(shape) and got[key].dtype == dtype, \
            (what, key, got[key].shape, got[key].dtype)


def _same_bits(a, b, what):
    assert list(a) == list(b), what
    for key in a:
        assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape, (what, key)
        assert a[key].tobytes() == b[key].tobytes(), (what, key)


SWITCHES = [(sol, rng, tab, his)
            for sol, rng, tab, his in itertools.product((False, True), repeat=4)
            if (tab or sol) and (sol or not rng) and (tab or not his)]


@pytest.mark.parametrize("solution,ranging,tables,history", SWITCHES,
                         ids=["".join(n for n, on in zip("srth", sw) if on) or "plain"
                              for sw in SWITCHES])
def test_result_keys_of_solve_batch_arrays(solution, ranging, tables, history):
    """``list(result)``: final, the solve's four, the solution's five, the four ranges, the
    history's two -- each only where asked for, in that order."""
    from simplex_mi355x.batch import solve_batch_arrays
    assert len(SWITCHES) == 8
    tabs, dims = _lps(1)
    out = solve_batch_arrays(tabs, dims, max_pivots=CAP, history=history, solution=solution,
                             tables=tables, ranging=ranging)
    form = _base_form(1, ranging, solution, tables)
    done = int(out["npivots"][0])
    assert 0 <= done <= CAP
    if history:
        form.update({"snaps": ((done, 3, 3), F8), "snap_off": ((2,), np.dtype(np.int64))})
    _same_form(out, form, (solution, ranging, tables, history))
    if history:
        assert out["snap_off"].tolist() == [0, done]


def _warm_form(B, S, K, ranging, log):
    form = {"base": None, "status": ((B, S), I4), "npivots": ((B, S), I4)}
    if log:
        form["rc"] = ((B, S, CAP, 2), I4)
    form.update(_answer_form((B, S), 3 + K, 3, ranging))
    return form


def _same_warm_form(out, B, S, K, ranging, log, what):
    form = _warm_form(B, S, K, ranging, log)
    base = out["base"]
    _same_form({k: v for k, v in out.items() if k != "base"},
               {k: v for k, v in form.items() if k != "base"}, what)
    assert list(out) == list(form), what
    _same_form(base, _base_form(B, ranging), (what, "base"))
    return base


def _scenarios(B, S, ranging):
    from simplex_mi355x.batch import solve_batch_scenarios_arrays
    tabs, dims = _lps(B)
    return solve_batch_scenarios_arrays(tabs, dims, np.zeros((B, S, 2)), np.zeros((B, S, 2)),
                                        CAP, ranging=ranging)


def _cuts(B, S, K, ranging, log):
    from simplex_mi355x.batch import solve_batch_cuts_arrays
    tabs, dims = _lps(B)
    return solve_batch_cuts_arrays(tabs, dims, np.zeros((B, S, K, 3)),
                                   np.zeros((B, S), dtype=np.int32), CAP, ranging=ranging, log=log)


@pytest.mark.parametrize("ranging", [False, True])
def test_no_scenarios(ranging):
    """S == 0: the keys of any other call, every per-scenario array with a second axis of 0, and
    ``base`` the dict of solve_batch_arrays(solution=True, tables=False, ranging=ranging)."""
    from simplex_mi355x.batch import solve_batch_arrays
    tabs, dims = _lps(2)
    base = _same_warm_form(_scenarios(2, 0, ranging), 2, 0, 0, ranging, False, ranging)
    _same_bits(base, solve_batch_arrays(tabs, dims, CAP, solution=True, tables=False,
                                        ranging=ranging), ranging)
    # and a call with scenarios has the same keys
    assert list(_scenarios(2, 1, ranging)) == list(_warm_form(2, 1, 0, ranging, False))


@pytest.mark.parametrize("K", [0, 1])
@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("ranging", [False, True])
def test_no_cut_sets(ranging, log, K):
    """S == 0, with room for K cuts per set: the row labels and duals are Rmax + K - 1 wide, and
    with ``log`` the warm log ``rc`` stands after ``npivots``, where a call with sets has it (a
    hand-written S == 0 dictionary once had it after ``nonbasis``)."""
    from simplex_mi355x.batch import solve_batch_arrays
    tabs, dims = _lps(2)
    what = (ranging, log, K)
    base = _same_warm_form(_cuts(2, 0, K, ranging, log), 2, 0, K, ranging, log, what)
    _same_bits(base, solve_batch_arrays(tabs, dims, CAP, solution=True, tables=False,
                                        ranging=ranging), what)
    _same_warm_form(_cuts(2, 1, K, ranging, log), 2, 1, K, ranging, log, (what, "S = 1"))


@pytest.mark.parametrize("ranging", [False, True])
def test_no_problems(ranging):
    """B == 0 (with blocks of the 2 x 2 shape): every array has a first axis of 0."""
    from simplex_mi355x.batch import solve_batch_arrays
    tabs, dims = _lps(0)
    for tables, history in ((True, False), (True, True), (False, False)):
        out = solve_batch_arrays(tabs, dims, CAP, history=history, solution=True, tables=tables,
                                 ranging=ranging)
        form = _base_form(0, ranging, True, tables)
        if history:
            form.update({"snaps": ((0, 3, 3), F8), "snap_off": ((1,), np.dtype(np.int64))})
        _same_form(out, form, (ranging, tables, history))
    for S in (0, 2):
        _same_warm_form(_scenarios(0, S, ranging), 0, S, 0, ranging, False, (ranging, S))
        _same_warm_form(_cuts(0, S, 1, ranging, True), 0, S, 1, ranging, True, (ranging, S))
