"""What the sensitivity ranges of a final table are, restated in plain Python from the contract of
include/smx.h (smx_batch_ranging), for the tests of smx_host_ranging, k_batch_ranging,
solve_batch_ranges and SimplexMethod.ranging(): the rule by the position of each label, one IEEE
division per candidate, and bounds folded with a key that orders -0.0 below +0.0 while one NaN
candidate makes the bound NaN.  It works on the C oracle's final table and on solution_util.replay's
labels from its log.  Everything compares by bit pattern.
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np

import solution_util as su

Expected = namedtuple("Expected", "rhs_lo rhs_hi cost_lo cost_hi")
FIELDS = Expected._fields
inf, nan = float("inf"), float("nan")


def _key(v):
    """The total order of the contract: by value, -0.0 below +0.0 (never called on a NaN)."""
    return (v, 0 if math.copysign(1.0, v) < 0 else 1)


def fold(cands, smallest: bool) -> float:
    """A bound from its candidates: NaN if any is NaN, +inf / -inf if there is none, else the
    minimum / maximum under `_key`."""
    if any(math.isnan(q) for q in cands):
        return nan
    if not cands:
        return inf if smallest else -inf
    return min(cands, key=_key) if smallest else max(cands, key=_key)


def _div(num, a) -> float:
    with np.errstate(all="ignore"):
        return float(np.float64(num) / np.float64(a))


def expected(final, basis, nonbasis, n, m) -> Expected:
    """The four arrays for the table `final` ([n + 1][m + 1] at least) under the labels `basis`
    [n] / `nonbasis` [m]; a code outside 0..n+m-1 is skipped, an unnamed slot is +0.0."""
    T = np.asarray(final, dtype=np.float64)
    rhs_lo, rhs_hi = np.zeros(n), np.zeros(n)
    cost_lo, cost_hi = np.zeros(m), np.zeros(m)
    for j in range(m):
        code = int(nonbasis[j])
        if m <= code < m + n:
            col = [(float(T[p, j]), float(T[p, m])) for p in range(n)]
            rhs_hi[code - m] = fold([_div(b, a) for a, b in col if a > 0], True)
            rhs_lo[code - m] = fold([_div(b, a) for a, b in col if a < 0], False)
        elif 0 <= code < m:
            cost_lo[code] = -float(T[n, j])
            cost_hi[code] = inf
    for p in range(n):
        code = int(basis[p])
        if m <= code < m + n:
            rhs_lo[code - m] = -float(T[p, m])
            rhs_hi[code - m] = inf
        elif 0 <= code < m:
            row = [(float(T[p, j]), -float(T[n, j])) for j in range(m)]
            cost_lo[code] = fold([_div(f, a) for a, f in row if a > 0], False)
            cost_hi[code] = fold([_div(f, a) for a, f in row if a < 0], True)
    return Expected(rhs_lo, rhs_hi, cost_lo, cost_hi)


def of_case(ref, n, m) -> Expected:
    """`expected` of a batch_util.case tuple (T, flen, oracle final table, status, pivots, log)."""
    basis, nonbasis, _ = su.replay(ref[5], n, m)
    return expected(ref[2], basis, nonbasis, n, m)


def host(T, n, m, basis, nonbasis, ld=None):
    """smx_host_ranging on `T` (copied into a buffer of leading dimension `ld`, the gap filled
    with a value that would show) -> (return code, Expected)."""
    from simplex_mi355x import _lib
    T = np.asarray(T, dtype=np.float64)
    ld = ld or m + 1
    buf = np.full((n + 1, ld), 777.0)
    buf[:, :m + 1] = T[:n + 1, :m + 1]
    basis = np.ascontiguousarray(basis, dtype=np.int32)
    nonbasis = np.ascontiguousarray(nonbasis, dtype=np.int32)
    out = [np.full(k, 7.0) for k in (n, n, m, m)]
    err = _lib.load().smx_host_ranging(buf.ctypes.data, ld, n, m, basis.ctypes.data,
                                       nonbasis.ctypes.data, *(a.ctypes.data for a in out))
    return err, Expected(*out)


def same_ranges(got, exp, what, nan_aware=False):
    """A Ranging (or any tuple with the same four fields) against `expected`'s answer."""
    for name, g, e in zip(FIELDS, got, exp):
        assert np.asarray(g).dtype == np.float64, (what, name)
        assert su.same_floats(g, e, nan_aware), \
            (what, name, [(i, float(a).hex(), float(b).hex())
                          for i, (a, b) in enumerate(zip(np.atleast_1d(g), np.atleast_1d(e)))
                          if su.bits(a) != su.bits(b)][:4])


def same_arrays(out, q, n, m, exp, what, nan_aware=False):
    """Problem q of a solve_batch_arrays(ranging=True) result (or of raw [B][Rmax] / [B][ldb]
    kernel outputs): the ranges inside (n, m) and +0.0 in the padding past them."""
    for name, e in zip(FIELDS, exp):
        k = n if name.startswith("rhs") else m
        assert su.same_floats(out[name][q, :k], e, nan_aware), \
            (what, name, [(i, float(a).hex(), float(b).hex())
                          for i, (a, b) in enumerate(zip(out[name][q, :k], e))
                          if su.bits(a) != su.bits(b)][:4])
        assert not su.bits(out[name][q, k:]).any(), (what, name, "padding")


# ----------------------------------------------------------------------------------------------
# The seeded cases of the CPU test (batch_util.case with flen = m): (kind, n, m, seed, cap).
CASES = [("uniform", 3, 2, 0, 64), ("uniform", 40, 7, 1, 64), ("uniform", 63, 63, 0, 64),
         ("mixed", 20, 20, 0, 64), ("mixed", 9, 33, 2, 64), ("uniform", 65, 65, 0, 1024),
         ("uniform", 100, 100, 0, 256), ("uniform", 300, 40, 0, 1024),
         ("uniform", 40, 300, 0, 1024), ("uniform", 257, 3, 0, 64), ("degenerate", 40, 30, 1, 64)]
# What makes them sharp, counted on the oracle's own tables: (n, m) -> (variables in the basis,
# bounds with both ends finite).  A kernel that only ever applies the one-entry rules, or that
# reduces one side only, fails on every one of them.
COUNTS = {(63, 63): (12, 24), (100, 100): (21, 42), (300, 40): (18, 36), (40, 300): (20, 22)}
# The cases that end at `optimum`, where lo <= 0 <= hi holds everywhere; 65 x 65 after 502 pivots.
OPTIMAL = [(3, 2), (40, 7), (65, 65), (300, 40), (257, 3)]


def case(k):
    from batch_util import case as _case
    kind, n, m, seed, cap = CASES[k]
    return _case(kind, n, m, seed, cap, m)


def census(exp: Expected):
    """(bounds with both ends finite) of one answer."""
    two = int((np.isfinite(exp.rhs_lo) & np.isfinite(exp.rhs_hi)).sum())
    return two + int((np.isfinite(exp.cost_lo) & np.isfinite(exp.cost_hi)).sum())


def check_sharp_cases():
    seen_optimal = []
    for k, (kind, n, m, seed, cap) in enumerate(CASES):
        ref = case(k)
        basis, _, _ = su.replay(ref[5], n, m)
        exp = of_case(ref, n, m)
        nvar = int((basis < m).sum())
        assert nvar > 0 and census(exp) > 0, (CASES[k], nvar, census(exp))
        if (n, m) in COUNTS:
            assert (nvar, census(exp)) == COUNTS[n, m], (CASES[k], nvar, census(exp))
        if ref[3] == 1:                                      # SMX_OPTIMUM
            seen_optimal.append((n, m))
            for lo, hi in ((exp.rhs_lo, exp.rhs_hi), (exp.cost_lo, exp.cost_hi)):
                assert (lo <= 0).all() and (hi >= 0).all(), CASES[k]
    assert seen_optimal == OPTIMAL, seen_optimal
    assert case(5)[4] == 502


# ----------------------------------------------------------------------------------------------
# Hand-made tables: the events the generators never produce.  Each is (name, T, n, m, basis,
# nonbasis, {(field, slot): expected value}); everything else follows from `expected`.
def _blank(n, m):
    """All entries 1.0 in A, "-b" 2.0, f-row 3.0: finite, no zeros, identity labels."""
    T = np.ones((n + 1, m + 1))
    T[:n, m] = 2.0
    T[n, :m] = 3.0
    T[n, m] = 0.0
    return T, np.arange(m, m + n, dtype=np.int32), np.arange(m, dtype=np.int32)


def handmade():
    out = []
    n, m = 8, 6
    # a slack label over column 1 (swap with row 7's label), a variable label on row 7
    for rows, tag in (((0, 5), "0,5"), ((5, 0), "5,0")):
        T, basis, nonbasis = _blank(n, m)
        basis[7], nonbasis[1] = nonbasis[1], basis[7]        # y8 over column 1, x2 on row 7
        T[:n, 1] = 0.0                                       # only the two rows below take part
        T[rows[0], 1], T[rows[1], 1] = 1.0, 4.0
        T[rows[0], m], T[rows[1], m] = 0.0, -0.0             # q = +0.0 and -0.0
        out.append((f"pos a, zeros rows {tag}", T, n, m, basis, nonbasis,
                    {("rhs_hi", 7): -0.0, ("rhs_lo", 7): -inf}))
        T = T.copy()
        T[rows[0], 1], T[rows[1], 1] = -1.0, -4.0            # q = -0.0 and +0.0
        out.append((f"neg a, zeros rows {tag}", T, n, m, basis, nonbasis,
                    {("rhs_lo", 7): 0.0, ("rhs_hi", 7): inf}))
    T, basis, nonbasis = _blank(n, m)
    basis[7], nonbasis[1] = nonbasis[1], basis[7]
    T[:n, 1] = [1.0, -2.0, nan, 0.0, -0.0, 2.0, -4.0, 0.5]
    T[0, m] = nan                                            # NaN "-b" under a > 0
    T[2, m] = 9.0                                            # a NaN a: skipped
    out.append(("nan b under pos a", T, n, m, basis, nonbasis,
                {("rhs_hi", 7): nan, ("rhs_lo", 7): -0.5}))
    T, basis, nonbasis = _blank(n, m)
    basis[7], nonbasis[1] = nonbasis[1], basis[7]
    T[:n, 1] = 0.0
    T[3, 1], T[3, m] = inf, inf                              # inf / inf: a NaN candidate
    T[4, 1], T[4, m] = -inf, 5.0                             # 5 / -inf = -0.0
    out.append(("inf over inf", T, n, m, basis, nonbasis,
                {("rhs_hi", 7): nan, ("rhs_lo", 7): -0.0}))
    T, basis, nonbasis = _blank(n, m)
    basis[7], nonbasis[1] = nonbasis[1], basis[7]
    T[:n, 1] = [0.0, -0.0] * 4                               # a column of zeros
    out.append(("zero column", T, n, m, basis, nonbasis,
                {("rhs_lo", 7): -inf, ("rhs_hi", 7): inf}))
    # the same events along a variable's row (x2 on row 7): q = (-T[n][j]) / T[7][j]
    T, basis, nonbasis = _blank(n, m)
    basis[7], nonbasis[1] = nonbasis[1], basis[7]
    T[7, :m] = [1.0, 0.0, 4.0, -1.0, -4.0, nan]
    T[n, :m] = [0.0, 7.0, -0.0, -0.0, 0.0, 1.0]              # q = -0.0, -, +0.0 | -0.0, +0.0, -
    out.append(("row zeros", T, n, m, basis, nonbasis,
                {("cost_lo", 1): 0.0, ("cost_hi", 1): -0.0}))
    T = T.copy()
    T[n, 0] = nan                                            # NaN f-row entry under a > 0
    out.append(("row nan f", T, n, m, basis, nonbasis,
                {("cost_lo", 1): nan, ("cost_hi", 1): -0.0}))
    T = T.copy()
    T[7, :m] = 0.0
    out.append(("zero row", T, n, m, basis, nonbasis,
                {("cost_lo", 1): -inf, ("cost_hi", 1): inf}))
    T = T.copy()
    T[7, 2], T[n, 2] = inf, -inf                             # (+inf) / inf
    T[7, 3], T[n, 3] = -inf, 3.0                             # -3 / -inf = +0.0
    out.append(("row inf over inf", T, n, m, basis, nonbasis,
                {("cost_lo", 1): nan, ("cost_hi", 1): 0.0}))
    # label codes outside 0..n+m-1: skipped, and the slots nobody names stay +0.0
    T, basis, nonbasis = _blank(n, m)
    basis[2], basis[6] = -1, n + m                           # y3, y7 named by nobody
    nonbasis[0], nonbasis[4] = n + m, -1                     # x1, x5 named by nobody
    out.append(("codes outside", T, n, m, basis, nonbasis,
                {("rhs_lo", 2): 0.0, ("rhs_hi", 2): 0.0, ("rhs_lo", 6): 0.0, ("rhs_hi", 6): 0.0,
                 ("cost_lo", 0): 0.0, ("cost_hi", 0): 0.0, ("cost_lo", 4): 0.0,
                 ("cost_hi", 4): 0.0, ("rhs_lo", 0): -2.0, ("cost_lo", 1): -3.0}))
    return out


def check_handmade(name, got, T, n, m, basis, nonbasis, pins):
    """`got` against `expected` by bit pattern (the NaNs here are all folded ones, so even they
    compare by bits), and the pinned values, so that `expected` itself is held to the contract."""
    exp = expected(T, basis, nonbasis, n, m)
    for (field, slot), v in pins.items():
        assert su.same_floats(getattr(exp, field)[slot], v), (name, field, slot, "expected()")
    same_ranges(got, exp, name)


def seeded_labels(n, m, seed):
    """A seeded permutation of 0..n+m-1 as (basis [n], nonbasis [m])."""
    perm = np.random.default_rng([seed, n, m]).permutation(n + m).astype(np.int32)
    return perm[:n].copy(), perm[n:].copy()
