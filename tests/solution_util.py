"""What a solved LP's whole answer is, restated in Python and numpy from the C oracle's final table
and pivot log (batch_util.case), for the tests of k_batch_solution, solve_batch_solutions and
SimplexMethod.solution(): the label replay (simplex.py:152), x for every variable
(find_optimum, simplex.py:51-68), the f-row entries under the slack labels, and the objective as
function[0]*x[0] + function[1]*x[1] + ... with every product rounded on its own and the sum taken
strictly left to right from the first product.  Everything compares by bit pattern.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

Expected = namedtuple("Expected", "x duals objective basis nonbasis pivots")


def replay(log, n, m):
    """(basis [n], nonbasis [m], times an x label left the basis) after the pivots of `log`.
    Codes: k in 0..m-1 is 'x{k+1}', m + i is 'y{i+1}'; an entry outside r < n, c < m is skipped."""
    basis = [m + i for i in range(n)]
    nonbasis = list(range(m))
    left = 0
    for r, c in np.asarray(log).reshape(-1, 2).tolist():
        if 0 <= r < n and 0 <= c < m:
            left += basis[r] < m
            basis[r], nonbasis[c] = nonbasis[c], basis[r]
    return np.array(basis, dtype=np.int32), np.array(nonbasis, dtype=np.int32), left


def ordered_objective(function, x) -> float:
    """p[0] + p[1] + ... + p[m-1], p[k] = function[k] * x[k], in Python floats: each product and
    each partial sum rounded once, no FMA, the sum starting from p[0] (not from 0.0)."""
    f = [float(v) for v in function]
    xs = [float(v) for v in x]
    total = f[0] * xs[0]
    for k in range(1, len(xs)):
        total = total + f[k] * xs[k]
    return total


def expected(final, log, n, m, function) -> Expected:
    """The answer for the table `final` ([n + 1][m + 1] at least) reached by the pivots of `log`;
    `function` is the ORIGINAL objective (only its first m entries are used)."""
    final = np.asarray(final, dtype=np.float64)
    basis, nonbasis, _ = replay(log, n, m)
    x = np.zeros(m, dtype=np.float64)
    duals = np.zeros(n, dtype=np.float64)
    for i in range(n):
        if basis[i] < m:
            x[basis[i]] = final[i, m]
    for j in range(m):
        if nonbasis[j] >= m:
            duals[nonbasis[j] - m] = final[n, j]
    return Expected(x, duals, ordered_objective(function[:m], x), basis, nonbasis,
                    len(np.asarray(log).reshape(-1, 2)))


def of_case(ref, n, m) -> Expected:
    """`expected` of a batch_util.case tuple (T, flen, oracle final table, status, pivots, log)."""
    T, _flen, Tref, _st, _done, log = ref
    return expected(Tref, log, n, m, T[n])


def label_codes(labels, m):
    """['y1', 'x2', ...] (a reference `row` / `column` without its last entry) -> codes."""
    return [int(s[1:]) - 1 + (m if s[0] == "y" else 0) for s in labels]


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_floats(got, exp, nan_aware=False) -> bool:
    """Equal bit patterns; with `nan_aware`, NaN positions equal and the bits elsewhere (NaN
    payload and sign are outside the contract)."""
    got = np.atleast_1d(np.asarray(got, dtype=np.float64))
    exp = np.atleast_1d(np.asarray(exp, dtype=np.float64))
    if got.shape != exp.shape:
        return False
    if nan_aware:
        gn, en = np.isnan(got), np.isnan(exp)
        return bool(np.array_equal(gn, en) and np.array_equal(bits(got[~en]), bits(exp[~en])))
    return bool(np.array_equal(bits(got), bits(exp)))


def same_solution(got, exp, what, nan_aware=False):
    """A Solution (or any tuple with the same six fields) against `expected`'s answer."""
    assert np.array_equal(np.asarray(got.basis), exp.basis), (what, "basis")
    assert np.array_equal(np.asarray(got.nonbasis), exp.nonbasis), (what, "nonbasis")
    assert np.asarray(got.basis).dtype == np.int32 and np.asarray(got.nonbasis).dtype == np.int32
    assert same_floats(got.x, exp.x, nan_aware), (what, "x")
    assert same_floats(got.duals, exp.duals, nan_aware), (what, "duals")
    assert same_floats(got.objective, exp.objective, nan_aware), \
        (what, "objective", float(got.objective).hex(), float(exp.objective).hex())
    assert int(got.pivots) == exp.pivots, (what, "pivots")


def same_arrays(out, q, n, m, exp, what, nan_aware=False):
    """Problem q of a solve_batch_arrays(solution=True) result: the answer inside (n, m) and the
    padding past it (+0.0 in x and duals, -1 in the labels)."""
    R1, C1 = out["basis"].shape[1], out["nonbasis"].shape[1]
    assert out["x"].shape[1] == C1 and out["duals"].shape[1] == R1, what
    assert out["basis"].dtype == np.int32 and out["nonbasis"].dtype == np.int32, what
    assert np.array_equal(out["basis"][q, :n], exp.basis), (what, "basis")
    assert np.array_equal(out["nonbasis"][q, :m], exp.nonbasis), (what, "nonbasis")
    assert (out["basis"][q, n:] == -1).all() and (out["nonbasis"][q, m:] == -1).all(), what
    assert same_floats(out["x"][q, :m], exp.x, nan_aware), (what, "x")
    assert same_floats(out["duals"][q, :n], exp.duals, nan_aware), (what, "duals")
    assert not bits(out["x"][q, m:]).any() and not bits(out["duals"][q, n:]).any(), (what, "pad")
    assert same_floats(out["objective"][q], exp.objective, nan_aware), \
        (what, "objective", float(out["objective"][q]).hex(), float(exp.objective).hex())
    assert int(out["npivots"][q]) == exp.pivots, (what, "pivots")


# Cases whose ordered objective differs in the last bits from numpy's pairwise np.sum (the two
# uniform ones from np.dot too), and in which x labels leave the basis again: (kind, n, m, seed,
# cap, times an x label left).  A reduction in another order, or a replay that only ever moves
# labels into rows, fails on them.  check_sharp_cases() asserts both properties on the oracle's
# own tables, so a change of generator cannot quietly blunt them.
SHARP = [("uniform", 100, 100, 0, 256, 108), ("uniform", 100, 100, 1, 256, 69),
         ("mixed", 20, 20, 0, 64, 27)]
SHARP_OBJECTIVE_0 = "-0x1.c401f6314f4eep+0"      # uniform 100 x 100 seed 0, ordered


def sharp_case(k):
    from batch_util import case
    kind, n, m, seed, cap, _ = SHARP[k]
    return case(kind, n, m, seed, cap, m)


def check_sharp_cases():
    for k, (kind, n, m, seed, cap, left) in enumerate(SHARP):
        ref = sharp_case(k)
        exp = of_case(ref, n, m)
        p = np.asarray(ref[0][n, :m]) * exp.x
        assert np.isfinite(exp.objective), SHARP[k]
        others = (float(np.sum(p)), float(np.dot(ref[0][n, :m], exp.x)))
        assert others[0] != exp.objective, (SHARP[k], "the ordered sum no longer differs")
        if kind == "uniform":
            assert others[1] != exp.objective, (SHARP[k], "np.dot no longer differs")
        assert all(abs(o - exp.objective) <= 4 * np.spacing(abs(exp.objective)) for o in others)
        assert replay(ref[5], n, m)[2] == left, (SHARP[k], replay(ref[5], n, m)[2])
    assert of_case(sharp_case(0), 100, 100).objective.hex() == SHARP_OBJECTIVE_0
