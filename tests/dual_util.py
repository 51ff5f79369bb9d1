"""The selection rules of include/smx.h restated in Python, for the tests of the dual-simplex rule
(SMX_RULE_DUAL): smx_host_select_rule / smx_host_run_rule, the three dual batch kernels,
solve_batch_*(warm_rule="dual") and SimplexMethod.solve(rule="dual").

`select` decides one step in Python floats (every comparison and the one division per candidate
are single IEEE operations), `run` chains steps with the reference's element expression
(t*e - pr*pc)/e (numpy float64 element by element: each operation rounded on its own, no FMA).
The reference branch is held to the C oracle by bit pattern (test_dual.py), so the dual branch
differs from a checked run in the selection alone.  Everything compares by bit pattern.
"""
from __future__ import annotations

import math

import numpy as np

import solution_util as su

inf, nan = float("inf"), float("nan")

REFERENCE, DUAL = 0, 1
PIVOT, OPTIMUM, INCORRECT, NOT_CONVERGE, FSHORT, IDLE = 0, 1, 2, 3, 4, 5
NONE = 0x7F7F7F7F


def _reference(t, n, m, flen):
    """simplex.py:70-141 as include/smx.h states it: (status, r, c)."""
    for i in range(n):
        if t[i][m] < 0.0:
            for j in range(m):
                if t[i][j] > 0.0:
                    return PIVOT, i, j
            return INCORRECT, i, NONE
    f = t[n]
    c = NONE
    for j in range(min(flen, m)):
        if f[j] < 0.0:
            c = j
            break
    if c == NONE:
        return (FSHORT if flen < m else OPTIMUM), NONE, NONE
    first, first_v = NONE, 0.0
    best = (3, 0.0, NONE)                                    # (class, v, row)
    for i in range(n):
        a = t[i][c]
        if a != 0.0:                                         # a NaN entry counts
            v = _div(t[i][m], a)
            if first == NONE:
                first, first_v = i, v
            if not math.isnan(v):
                cls = 0 if v < 0.0 else (1 if v == 0.0 else 2)
                if _ratio_before((cls, v, i), best):
                    best = (cls, v, i)
    if first == NONE:
        return NOT_CONVERGE, NONE, c
    if math.isnan(first_v):
        return PIVOT, first, c
    if best[0] >= 2:
        return NOT_CONVERGE, NONE, c
    return PIVOT, best[2], c


def _ratio_before(a, b):
    if a[0] != b[0]:
        return a[0] < b[0]
    if a[0] == 0:
        return a[1] > b[1] or (a[1] == b[1] and a[2] > b[2])
    return a[2] < b[2]


def _div(num, den):
    """One IEEE fp64 division (Python raises on a zero denominator; numpy does not)."""
    with np.errstate(all="ignore"):
        return float(np.float64(num) / np.float64(den))


def is_dual_step(t, n, m, flen, rule):
    """Item 2 of the contract: a negative "-b", no negative f-row entry, flen >= m."""
    if rule != DUAL or flen < m:
        return False
    nb = any(t[i][m] < 0.0 for i in range(n))
    nf = any(t[n][j] < 0.0 for j in range(min(flen, m)))
    return nb and not nf


def select(t, n, m, flen, rule):
    """One selection on the table `t` (list of lists or array): (status, r, c); r and c are NONE
    where the rule names none (r is the offending row after INCORRECT)."""
    if rule not in (REFERENCE, DUAL):
        raise ValueError(rule)
    t = [[float(v) for v in row[:m + 1]] for row in np.asarray(t, dtype=np.float64)[:n + 1].tolist()]
    if not is_dual_step(t, n, m, flen, rule):
        return _reference(t, n, m, flen)
    r = next(i for i in range(n) if t[i][m] < 0.0)
    best = None                                              # (NaN-ness, q, j)
    for j in range(m):
        if t[r][j] > 0.0:                                    # a NaN entry is no candidate
            q = _div(t[n][j], t[r][j])
            cand = (1 if math.isnan(q) else 0, q, j)
            if best is None or _dual_before(cand, best):
                best = cand
    if best is None:
        return INCORRECT, r, NONE
    return PIVOT, r, best[2]


def _dual_before(a, b):
    if a[0] != b[0]:
        return a[0] < b[0]
    if a[0] == 0 and a[1] != b[1]:                           # -0.0 == +0.0: a tie
        return a[1] < b[1]
    return a[2] < b[2]


def pivot(T, r, c):
    """The Jordan step (simplex.py:149-177) on the whole array, out of place."""
    T = np.asarray(T, dtype=np.float64)
    e = T[r, c]
    with np.errstate(all="ignore"):
        t1 = T * e
        t2 = np.multiply.outer(T[:, c], T[r])
        out = (t1 - t2) / e
        out[:, c] = T[:, c] / e
        out[r] = -T[r] / e
        out[r, c] = np.float64(1.0) / e
    return out


def run(T, n, m, flen, cap, rule):
    """Steps until a terminal status or `cap` pivots, as smx_host_run_rule and the batch kernels
    take them: (final [n + 1][m + 1], status (PIVOT = the cap was reached), pivots, log [pivots][2]
    int32, dual steps among them)."""
    T = np.ascontiguousarray(np.asarray(T, dtype=np.float64)[:n + 1, :m + 1]).copy()
    log = []
    duals = 0
    status = PIVOT
    while len(log) < cap:
        t = T.tolist()
        was_dual = is_dual_step(t, n, m, flen, rule)
        status, r, c = select(T, n, m, flen, rule)
        if status != PIVOT:
            break
        T = pivot(T, r, c)
        log.append((r, c))
        duals += was_dual
    return T, status, len(log), np.array(log, dtype=np.int32).reshape(-1, 2), duals


def host_select(T, n, m, flen, rule, ld=None):
    """smx_host_select_rule on `T` in a buffer of leading dimension `ld` (the gap filled with a
    value that would show): (status, r, c)."""
    import ctypes
    from simplex_mi355x import _lib
    ld = ld or m + 1
    buf = np.full((n + 1, ld), -777.0)
    buf[:, :m + 1] = np.asarray(T, dtype=np.float64)[:n + 1, :m + 1]
    shape = _lib.Shape(ld, n, n, m, flen, 0, 1)
    rc = np.full(2, -5, dtype=np.int32)
    st = _lib.load().smx_host_select_rule(buf.ctypes.data, ctypes.byref(shape), rule,
                                          rc.ctypes.data)
    return int(st), int(rc[0]), int(rc[1])


def host_run(T, n, m, flen, cap, rule, ld=None, entry="smx_host_run_rule"):
    """smx_host_run_rule (or, with `entry`, smx_host_run) on `T`: (final, status with IDLE read as
    PIVOT, pivots, log)."""
    import ctypes
    from simplex_mi355x import _lib
    ld = ld or m + 1
    buf = np.full((2, n + 1, ld), -777.0)
    buf[0, :, :m + 1] = np.asarray(T, dtype=np.float64)[:n + 1, :m + 1]
    shape = _lib.Shape(ld, n, n, m, flen, 0, 1)
    log = np.zeros((max(cap, 1), 2), dtype=np.int32)
    st = ctypes.c_int32(-1)
    L = _lib.load()
    if entry == "smx_host_run":
        done = L.smx_host_run(buf[0].ctypes.data, buf[1].ctypes.data, ctypes.byref(shape), 0, cap,
                              log.ctypes.data, ctypes.byref(st))
    else:
        done = L.smx_host_run_rule(buf[0].ctypes.data, buf[1].ctypes.data, ctypes.byref(shape), 0,
                                   cap, rule, log.ctypes.data, ctypes.byref(st))
    done = int(done)
    assert (buf[done & 1][:, m + 1:] == -777.0).all()
    status = PIVOT if st.value == IDLE else int(st.value)
    return buf[done & 1][:, :m + 1].copy(), status, done, log[:done].copy()


def same_run(got, exp, what):
    """(final, status, pivots, log) of two runs, by bit pattern."""
    assert got[1] == exp[1] and got[2] == exp[2], (what, got[1:3], exp[1:3])
    assert np.array_equal(np.asarray(got[3]).reshape(-1, 2), np.asarray(exp[3]).reshape(-1, 2)), what
    a, b = su.bits(got[0]), su.bits(exp[0])
    assert a.shape == b.shape, what
    diff = np.argwhere(a != b)
    assert not len(diff), (what, [(int(p), int(j)) for p, j in diff[:4]])


# ----------------------------------------------------------------------------------------------
# Hand-made one-step tables: what generators never produce.  `onestep(n, m, ...)` builds a table
# whose row `nb` is the first with a negative "-b" and whose f-row is non-negative; the cases set
# row nb and the f-row at chosen columns.  Each case is (name, T, n, m, flen, (status, r, c) under
# the dual rule, whether that step is a dual step).
def blank(n, m, nb):
    """A = -1.0 (no candidate anywhere), "-b" = 2.0 but -3.0 in row nb and -1.0 in every later
    third row (rows the rule must not pick), f-row = 8.0, constant 0.5."""
    T = -np.ones((n + 1, m + 1))
    T[:n, m] = 2.0
    T[nb:n:3, m] = -1.0
    T[nb, m] = -3.0
    T[n, :m] = 8.0
    T[n, m] = 0.5
    return T


def place(n, m, nb, entries, frow=None):
    """`blank` with row nb's entries {column: value} and the f-row's {column: value}."""
    T = blank(n, m, nb)
    for j, v in entries.items():
        T[nb, j] = v
    for j, v in (frow or {}).items():
        T[n, j] = v
    return T


def handmade(n=5, m=6, nb=2, cols=None):
    """The one-step cases at n x m with the offending row `nb`; `cols` = six distinct columns
    (a, b, c, d, e, g) at which the events are placed (default 0..5 spread over m)."""
    a, b, c, d, e, g = cols or (1, 3, 0, 2, 4, 5)
    lo, hi = min(a, b), max(a, b)
    out = []
    # q = 2.0 at both a and b, 3.0 at c: the tie goes to the smaller column
    out.append(("tie", place(n, m, nb, {a: 4.0, b: 2.0, c: 1.0}, {a: 8.0, b: 4.0, c: 3.0}),
                n, m, m, (PIVOT, nb, lo), True))
    # f entries -0.0 and +0.0 tie under <: the smaller column, whichever zero it holds
    out.append(("signed zeros", place(n, m, nb, {a: 4.0, b: 2.0}, {lo: 0.0, hi: -0.0}),
                n, m, m, (PIVOT, nb, lo), True))
    out.append(("signed zeros swapped", place(n, m, nb, {a: 4.0, b: 2.0}, {lo: -0.0, hi: 0.0}),
                n, m, m, (PIVOT, nb, lo), True))
    # one NaN ratio (inf / inf) among finite ones, at the smallest column: a finite one wins
    out.append(("one nan ratio", place(n, m, nb, {c: inf, a: 1.0, b: 1.0}, {c: inf, a: 7.0, b: 6.0}),
                n, m, m, (PIVOT, nb, b), True))
    # every ratio NaN (a NaN f entry is not negative): the smaller column
    out.append(("all nan ratios", place(n, m, nb, {a: 1.0, b: 2.0}, {a: nan, b: nan}),
                n, m, m, (PIVOT, nb, lo), True))
    # an inf entry in the row: q = 8 / inf = 0 beats every positive ratio
    out.append(("inf entry", place(n, m, nb, {a: 1.0, b: inf}, {a: 0.25}),
                n, m, m, (PIVOT, nb, b), True))
    # a NaN entry in row nb is no candidate
    out.append(("nan entry", place(n, m, nb, {c: nan, a: 1.0}, {c: 0.0, a: 5.0}),
                n, m, m, (PIVOT, nb, a), True))
    # no candidate: zeros, negatives and a NaN only
    out.append(("no candidate", place(n, m, nb, {a: 0.0, b: -0.0, c: nan}),
                n, m, m, (INCORRECT, nb, NONE), True))
    # a negative f entry beside the negative constants: the reference's step (first positive)
    T = place(n, m, nb, {a: 4.0, b: 2.0}, {a: 8.0, b: 1.0, g: -1.0})
    out.append(("not dual feasible", T, n, m, m, (PIVOT, nb, lo), False))
    # flen = m - 1: the reference's step although the f-row holds no negative entry
    T = place(n, m, nb, {a: 4.0, b: 2.0}, {a: 8.0, b: 1.0})
    out.append(("short f-row", T, n, m, m - 1, (PIVOT, nb, lo), False))
    # flen = m + 1 is as good as m
    T = place(n, m, nb, {a: 4.0, b: 2.0}, {a: 8.0, b: 1.0})
    out.append(("long f-row", T, n, m, m + 1, (PIVOT, nb, b), True))
    # the smallest ratio at the last of many candidates
    T = place(n, m, nb, {j: 1.0 for j in range(m)}, {j: 9.0 + j for j in range(m)})
    T[n, d] = 0.125
    out.append(("every column a candidate", T, n, m, m, (PIVOT, nb, d), True))
    # primal feasible: the reference's phase 2, here the optimum
    T = blank(n, m, nb)
    T[:n, m] = 2.0
    out.append(("primal feasible", T, n, m, m, (OPTIMUM, NONE, NONE), False))
    return out


def check_handmade(case):
    """`select` itself against the pinned outcome of a hand-made case."""
    name, T, n, m, flen, want, dual = case
    assert is_dual_step(T.tolist(), n, m, flen, DUAL) == dual, name
    assert select(T, n, m, flen, DUAL) == want, (name, select(T, n, m, flen, DUAL), want)
