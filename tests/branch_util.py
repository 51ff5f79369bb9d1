"""Branch and bound on solved LPs, restated for the tests of smx_host_branch_pick / smx_host_branch,
k_batch_branch_pick / k_batch_branch, SimplexMethod.solve_integer() and solve_batch_integer: the
PICK of include/smx.h in Python floats (every operation rounded once), the children as cuts_util's
restatement of the two single-variable cuts (nothing new is restated for the tables), the
hand-made "-b" columns with their pinned results, and the small integer programs of the meaning
test with their brute-force answers.  Everything compares by bit pattern.
"""
from __future__ import annotations

import math

import numpy as np

import cuts_util as cu
import solution_util as su

inf, nan = float("inf"), float("nan")
TOL = 1e-6


def frac(v: float) -> float:
    """d of the contract: NaN for a NaN or infinite v."""
    if math.isnan(v) or math.isinf(v):
        return nan
    lo = float(math.floor(v))
    a = v - lo
    b = (lo + 1.0) - v
    return b if b < a else a


def pick(T, n, m, basis, ints, tol):
    """(bvar, brow, bval, bneg, bmin) of the table `T` under the row labels `basis` [n] and the
    mask `ints` [m]."""
    best = None                                              # (d, k, p, v)
    bneg, bmin, seen = 0.0, 0.0, False
    for p in range(n):
        v = float(T[p][m])
        if v < 0.0 and not seen:
            seen, bneg = True, v
        if v < bmin:
            bmin = v
        k = int(basis[p])
        if not (0 <= k < m) or not ints[k]:
            continue
        d = frac(v)
        if not d > tol:
            continue
        if best is None or (d, -k, -p) > (best[0], -best[1], -best[2]):
            best = (d, k, p, v)
    if best is None:
        return -1, -1, 0.0, bneg, bmin
    return best[1], best[2], best[3], bneg, bmin


def two_cuts(m, k, v):
    """The down and the up cut of a branch on x{k+1} at the value v, as rows of cuts_util."""
    down, up = np.zeros(m + 1), np.zeros(m + 1)
    down[k], down[m] = -1.0, math.floor(v)
    up[k], up[m] = 1.0, -math.ceil(v)
    return down, up


def children(T, n, m, basis, nonbasis, p):
    """(E_down, E_up, basis_c) of a branch on row p: cuts_util.restate of each cut alone."""
    k = int(basis[p])
    out = [cu.restate(T, n, m, basis, nonbasis, [g]) for g in two_cuts(m, k, float(T[p][m]))]
    assert np.array_equal(out[0][1], out[1][1])
    return out[0][0], out[1][0], out[0][1]


def snapped(E, n, m, snap):
    """E with the "-b" entries of rows 0..n-1 that lie in [-snap, 0) written as +0.0."""
    E = np.array(E, dtype=np.float64)
    col = E[:n, m]
    col[(col < 0) & (col >= -snap)] = 0.0
    return E


def host_pick(T, n, m, basis, ints, tol, ld=None):
    """smx_host_branch_pick on `T` in a buffer of leading dimension `ld` (the gap filled with a
    value that would show) -> (return code, (bvar, brow, bval, bneg, bmin))."""
    import ctypes
    from simplex_mi355x import _lib
    T = np.asarray(T, dtype=np.float64)
    ld = ld or m + 1
    buf = np.full((n + 1, ld), 777.5)
    buf[:, :m + 1] = T[:n + 1, :m + 1]
    basis = np.ascontiguousarray(basis, dtype=np.int32)
    ints = np.ascontiguousarray(ints, dtype=np.int32)
    bvar, brow = ctypes.c_int32(77), ctypes.c_int32(77)
    vals = [ctypes.c_double(7.0) for _ in range(3)]
    err = _lib.load().smx_host_branch_pick(buf.ctypes.data, ld, n, m, basis.ctypes.data,
                                           ints.ctypes.data, float(tol), ctypes.byref(bvar),
                                           ctypes.byref(brow), *(ctypes.byref(v) for v in vals))
    return err, (bvar.value, brow.value, *(v.value for v in vals))


def host_branch(T, n, m, basis, nonbasis, p, snap=0.0, ld=None, ld_out=None):
    """smx_host_branch on `T` -> (return code, E_down, E_up [n + 2][m + 1], basis_c [n + 1]); the
    gaps of the output buffers must come back untouched."""
    from simplex_mi355x import _lib
    T = np.asarray(T, dtype=np.float64)
    ld = ld or m + 1
    ld_out = ld_out or m + 1
    buf = np.full((n + 1, ld), 777.0)
    buf[:, :m + 1] = T[:n + 1, :m + 1]
    out = [np.full((n + 2, ld_out), 555.0) for _ in range(2)]
    bout = np.full(n + 1, 77, dtype=np.int32)
    basis = np.ascontiguousarray(basis, dtype=np.int32)
    nonbasis = np.ascontiguousarray(nonbasis, dtype=np.int32)
    err = _lib.load().smx_host_branch(buf.ctypes.data, ld, n, m, basis.ctypes.data,
                                      nonbasis.ctypes.data, int(p), float(snap),
                                      out[0].ctypes.data, out[1].ctypes.data, ld_out,
                                      bout.ctypes.data)
    if err == 0:
        assert all((e[:, m + 1:] == 555.0).all() for e in out)
    return err, out[0][:, :m + 1].copy(), out[1][:, :m + 1].copy(), bout


def same_pick(got, exp, what):
    assert got[:2] == exp[:2], (what, got, exp)
    assert su.same_floats(np.array(got[2:]), np.array(exp[2:])), \
        (what, [float(v).hex() for v in got[2:]], [float(v).hex() for v in exp[2:]])


# ----------------------------------------------------------------------------------------------
# Hand-made "-b" columns: (name, column [n], basis [n], ints [m], m, tol, pinned (bvar, brow,
# bval)).  The table around a column is all 1.0; only the column and the labels matter.
def ulp_up(x):
    return float(np.nextafter(x, inf))


def handmade():
    m = 4
    all_ = [1] * m
    out = [
        # a tie at .5: x1 sits in the LATER row and still wins
        ("tie at half", [2.5, 7.0, 1.5], [2, m, 0], all_, m, TOL, (0, 2, 1.5)),
        ("tie at half, rows swapped", [1.5, 7.0, 2.5], [0, m, 2], all_, m, TOL, (0, 0, 1.5)),
        ("minus one and a half", [-1.5, 3.0], [1, 0], all_, m, TOL, (1, 0, -1.5)),
        ("minus one and a quarter", [-1.25, 3.0], [1, 0], all_, m, TOL, (1, 0, -1.25)),
        ("never candidates", [1e300, inf, -inf, nan], [0, 1, 2, 3], all_, m, TOL, (-1, -1, 0.0)),
        ("never candidates, tol 0", [1e300, inf, -inf, nan], [0, 1, 2, 3], all_, m, 0.0,
         (-1, -1, 0.0)),
        ("minus zero", [-0.0, 0.0], [0, 1], all_, m, 0.0, (-1, -1, 0.0)),
        # 3.25 is 0.25 away exactly; 0.25 is not past the tolerance 0.25, one ulp further is
        ("exactly tol away", [3.25, 5.75], [0, 1], all_, m, 0.25, (-1, -1, 0.0)),
        ("one ulp past tol", [3.25, ulp_up(5.25)], [0, 1], all_, m, 0.25,
         (1, 1, ulp_up(5.25))),
        ("tol 0 takes one ulp", [ulp_up(3.0), 4.0], [0, 1], all_, m, 0.0, (0, 0, ulp_up(3.0))),
        ("unmarked fractional variable", [2.5, 3.75], [0, 1], [0, 1, 1, 1], m, TOL,
         (1, 1, 3.75)),
        ("fractional slack row", [2.5, 3.5, 1.25], [m, m + 1, 3], all_, m, TOL, (3, 2, 1.25)),
        ("codes outside", [2.5, 3.5, 1.125], [-1, m + 3, 2], all_, m, TOL, (2, 2, 1.125)),
        ("no candidate", [2.0, 3.0, 1.0 + 1e-9, 4.0 - 1e-9], [0, 1, 2, 3], all_, m, TOL,
         (-1, -1, 0.0)),
        ("largest distance wins", [2.25, 3.5, 1.75], [0, 1, 2], all_, m, TOL, (1, 1, 3.5)),
    ]
    cases = []
    for name, col, basis, ints, m_, tol, pin in out:
        n = len(col)
        if "codes outside" in name:
            basis = [-1, n + m_, 2]
        T = np.ones((n + 1, m_ + 1))
        T[:n, m_] = col
        cases.append((name, T, n, m_, np.array(basis, dtype=np.int32),
                      np.array(ints, dtype=np.int32), tol, pin))
    return cases


def check_handmade(case, got):
    """`got` = (bvar, brow, bval, bneg, bmin) against `pick` and the pinned result, so that
    `pick` itself is held to the contract."""
    name, T, n, m, basis, ints, tol, pin = case
    exp = pick(T, n, m, basis, ints, tol)
    assert exp[:2] == pin[:2] and su.same_floats(exp[2], pin[2]), (name, "pick()", exp, pin)
    same_pick(got, exp, name)


# ----------------------------------------------------------------------------------------------
# The meaning set: small integer programs with a bounded box and the origin feasible.
SEEDS = range(200)


def instance(seed):
    """(A [n][m] ints 0..9 with a positive entry in every column, b [n] ints 10..60, c [m] ints
    -9..-1): minimise c.x subject to A x <= b, x >= 0 whole."""
    g = np.random.default_rng([seed, 4242])
    m, n = 2 + seed % 3, 2 + seed % 4
    A = g.integers(0, 10, size=(n, m))
    for k in range(m):
        if not (A[:, k] > 0).any():
            A[g.integers(0, n), k] = g.integers(1, 10)
    return A, g.integers(10, 61, size=n), g.integers(-9, 0, size=m)


def problem(A, b, c):
    """(constraints, function) of the solver: y_i = -sum_k a_ik x_k + b_i >= 0."""
    cons = [[-float(a) for a in A[i]] + [float(b[i])] for i in range(len(b))]
    return cons, [float(v) for v in c]


def brute(A, b, c):
    """The minimum of c.x over every whole point of the box x_k <= min_i b_i / a_ik that
    satisfies A x <= b, in integer arithmetic; None where there is none."""
    n, m = A.shape
    ub = [min(int(b[i]) // int(A[i, k]) for i in range(n) if A[i, k] > 0) for k in range(m)]
    grid = np.stack(np.meshgrid(*[np.arange(u + 1) for u in ub], indexing="ij"), -1).reshape(-1, m)
    ok = ((grid @ A.T) <= b).all(axis=1)
    return int((grid[ok] @ c).min()) if ok.any() else None


_BRUTE = {}


def brute_of(seed):
    """`brute` of `instance(seed)`, computed once."""
    if seed not in _BRUTE:
        _BRUTE[seed] = brute(*instance(seed))
    return _BRUTE[seed]
