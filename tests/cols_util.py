"""What the widened table of a final table and a set of new variables is, restated in plain Python
from the contract of include/smx.h (smx_batch_cols), for the tests of smx_host_cols, k_batch_cols,
solve_batch_columns and SimplexMethod.add_variables(): the one ordered sum per row in Python
floats (every product and every partial sum rounded once, no FMA, a coefficient equal to zero
skipped), the label recoding, the hand-made tables and the seeded column generator.  It works on
the C oracle's final table and on solution_util.replay's labels.  Everything compares by bit
pattern.
"""
from __future__ import annotations

import numpy as np

import scenario_util as scu
import solution_util as su

inf, nan = float("inf"), float("nan")


def recode(codes, n, m, K):
    """Label codes of the LP with K variables appended to the original: c < m stays, m + i becomes
    m + K + i, anything else names nothing (-1)."""
    return [c if 0 <= c < m else (c + K if m <= c < m + n else -1) for c in map(int, codes)]


def restate(T, n, m, basis, nonbasis, A):
    """(W [n + 1][m + K + 1], basis_v [n], nonbasis_v [m + K]) for the table `T` under the labels
    `basis` [n] / `nonbasis` [m] and the new variables `A` [K][n + 1] (entry n the cost)."""
    T = np.asarray(T, dtype=np.float64)
    A = np.asarray(A, dtype=np.float64).reshape(-1, n + 1)
    K = len(A)
    W = np.empty((n + 1, m + K + 1), dtype=np.float64)
    W[:, :m] = T[:n + 1, :m]
    W[:, m + K] = T[:n + 1, m]
    t = T.tolist()
    basis = [int(c) for c in basis[:n]]
    nonbasis = [int(c) for c in nonbasis[:m]]
    for c in range(K):
        a = A[c].tolist()
        for p in range(n + 1):
            if p == n:
                v = a[n]
            elif m <= basis[p] < m + n:
                v = a[basis[p] - m]
            else:
                v = 0.0
            for j in range(m):
                i = nonbasis[j] - m
                if 0 <= i < n and a[i] != 0:
                    v = v - t[p][j] * a[i]
            W[p, m + c] = v
    return (W, np.array(recode(basis, n, m, K), dtype=np.int32),
            np.array(recode(nonbasis, n, m, K) + [m + c for c in range(K)], dtype=np.int32))


def col_set(T0, n, m, seed, s, K, viol, Tf, basis, nonbasis):
    """Column set s of the LP `T0` (the ORIGINAL table): K new variables [a, cost] whose reduced
    cost under the base answer (the f-row entry of their column in the table `Tf` under `basis` /
    `nonbasis`) is -d, d = +-`viol` times the mean magnitude of the costs, the sign alternating
    with q + s.  The cost is found by restating the column with cost 0 and moving it by the rest."""
    g = np.random.default_rng([seed, n, m, s, 99])
    out = []
    for q in range(K):
        a = g.normal(size=n) * (g.random(n) < 0.75)
        if not a.any():
            a[0] = 1.0
        col = list(a) + [0.0]
        at_zero = restate(Tf, n, m, basis, nonbasis, [col])[0][n, m]
        d = viol * abs(T0[n, :m]).mean() * (1 if (q + s) % 2 == 0 else -1)
        col[n] = -d - at_zero
        out.append(col)
    return np.array(out, dtype=np.float64).reshape(K, n + 1)


def plain_cols(n, seed, s, K):
    """K seeded new variables [a, cost] that look at no table: normal entries, exact zeros on a
    quarter of them.  For the kernel's edge shapes and for tables holding NaN or inf."""
    g = np.random.default_rng([seed, n, s, 98])
    A = g.normal(size=(K, n + 1)) * (g.random((K, n + 1)) < 0.75)
    if K:
        A[:, 0] += (~A[:, :n].any(axis=1)) * 1.0
    return A


def dot_variant(T, n, m, basis, nonbasis, a):
    """One new column's sums taken by np.dot over the same terms: what a tree or blocked reduction
    would give.  Only for the sharpness check."""
    T = np.asarray(T, dtype=np.float64)
    a = np.asarray(a, dtype=np.float64)
    cols = [j for j in range(m) if m <= nonbasis[j] < m + n and a[nonbasis[j] - m] != 0]
    start = np.array([a[basis[p] - m] if m <= basis[p] < m + n else 0.0 for p in range(n)] + [a[n]])
    if not cols:
        return start
    return start - np.dot(T[:n + 1][:, cols], a[np.asarray(nonbasis)[cols] - m])


def host(T, n, m, basis, nonbasis, A, ld=None, ld_out=None):
    """smx_host_cols on `T` (copied into a buffer of leading dimension `ld`, the gap filled with a
    value that would show) -> (return code, W [n + 1][m + K + 1], basis_v [n], nonbasis_v
    [m + K]); the gap of the output buffer must come back untouched."""
    from simplex_mi355x import _lib
    T = np.asarray(T, dtype=np.float64)
    A = np.ascontiguousarray(np.asarray(A, dtype=np.float64).reshape(-1, n + 1))
    K = len(A)
    ld = ld or m + 1
    ld_out = ld_out or m + K + 1
    buf = np.full((n + 1, ld), 777.0)
    buf[:, :m + 1] = T[:n + 1, :m + 1]
    out = np.full((n + 1, ld_out), 555.0)
    bout = np.full(n, 77, dtype=np.int32)
    nout = np.full(m + K, 77, dtype=np.int32)
    basis = np.ascontiguousarray(basis, dtype=np.int32)
    nonbasis = np.ascontiguousarray(nonbasis, dtype=np.int32)
    err = _lib.load().smx_host_cols(buf.ctypes.data, ld, n, m, basis.ctypes.data,
                                    nonbasis.ctypes.data, A.ctypes.data if K else None, K,
                                    out.ctypes.data, ld_out, bout.ctypes.data, nout.ctypes.data)
    assert (out[:, m + K + 1:] == 555.0).all()
    return err, out[:, :m + K + 1].copy(), bout, nout


def widened(T0, n, m, A):
    """The ORIGINAL table with the new variables inserted as columns m..m+K-1, "-b" to their
    right."""
    A = np.asarray(A, dtype=np.float64).reshape(-1, n + 1)
    return np.hstack([T0[:n + 1, :m], A.T, T0[:n + 1, m:m + 1]])


def base_of_case(ref, n, m):
    """(basis, nonbasis) of a batch_util.case tuple's base run."""
    basis, nonbasis, _ = su.replay(ref[5], n, m)
    return basis, nonbasis


def cols_of_case(ref, n, m, seed, s, K, viol=0.05):
    """(A, W, basis_v, nonbasis_v, basis, nonbasis) of column set s with K new variables of a
    batch_util.case tuple."""
    basis, nonbasis = base_of_case(ref, n, m)
    A = col_set(ref[0], n, m, seed, s, K, viol, ref[2], basis, nonbasis)
    W, basis_v, nonbasis_v = restate(ref[2], n, m, basis, nonbasis, A)
    return A, W, basis_v, nonbasis_v, basis, nonbasis


same_table = scu.same_table
warm_labels = scu.warm_labels
expected_solution = scu.expected_solution


# ----------------------------------------------------------------------------------------------
# Hand-made tables: what generators never produce.  Each is (name, T, n, m, basis, nonbasis, A,
# {(p, kappa): expected value of W[p][m + kappa]}); everything else follows from `restate`.
def _blank(n, m):
    T, basis, nonbasis, _, _, _ = scu._blank(n, m)
    return T, basis, nonbasis


COLUMN_1 = [1.0, -2.0, 0.5, 4.0, -1.0, 3.0]


def _y5_nonbasic(n, m):
    """x2 on row 4, y5 over column 1, which holds 1, -2, 0.5, 4, -1 | 3."""
    T, basis, nonbasis = _blank(n, m)
    basis[4], nonbasis[1] = nonbasis[1], basis[4]
    T[:, 1] = COLUMN_1
    return T, basis, nonbasis


def handmade():
    out = []
    n, m = 5, 4
    # coefficients +0.0 and -0.0 on a non-basic slack (y1 over column 0) whose column holds inf,
    # NaN and -0.0: skipped
    T, basis, nonbasis = _y5_nonbasic(n, m)
    basis[0], nonbasis[0] = nonbasis[0], basis[0]            # x1 on row 0, y1 over column 0
    T[:, 0] = [inf, nan, -0.0, -inf, inf, nan]
    A = [[0.0, 0.0, 0.0, 0.0, 2.0, 1.0], [-0.0, 0.0, 0.0, -0.0, 2.0, 1.0]]
    pins = {(p, c): v for c in (0, 1) for p, v in enumerate([-2.0, 4.0, -1.0, -8.0, 2.0, -5.0])}
    out.append(("zero coefficients over inf and nan", T, n, m, basis, nonbasis, A, pins))
    # a -0.0 coefficient on a basic slack: the column's own bits under identity labels
    T, basis, nonbasis = _blank(n, m)
    A = [[-0.0, 0.0, 1.5, -0.0, 2.0, -0.0]]
    out.append(("own bits", T, n, m, basis, nonbasis, A, {(p, 0): v for p, v in enumerate(A[0])}))
    # NaN and inf coefficients: not equal to zero, applied (on y5 over column 1, and a NaN on the
    # basic slack y1)
    T, basis, nonbasis = _y5_nonbasic(n, m)
    A = [[0.0, 0.0, 0.0, 0.0, nan, 1.0], [0.0, 0.0, 0.0, 0.0, inf, 1.0],
         [nan, 0.0, 0.0, 0.0, 0.0, 0.5]]
    pins = {(p, 0): nan for p in range(n + 1)}
    pins.update({(p, 1): v for p, v in enumerate([-inf, inf, -inf, -inf, inf, -inf])})
    pins.update({(p, 2): v for p, v in enumerate([nan, 0.0, 0.0, 0.0, 0.0, 0.5])})
    out.append(("nan and inf coefficients", T, n, m, basis, nonbasis, A, pins))
    # one slack basic (y1 on row 0), one non-basic (y5 over column 1)
    T, basis, nonbasis = _y5_nonbasic(n, m)
    A = [[0.25, 0.0, 0.0, 0.0, 2.0, -3.0]]
    out.append(("basic and non-basic", T, n, m, basis, nonbasis, A,
                {(0, 0): 0.25 - 2.0, (1, 0): 4.0, (2, 0): -1.0, (3, 0): -8.0, (4, 0): 2.0,
                 (n, 0): -3.0 - 6.0}))
    # two non-basic slacks: the sum runs in ascending column order (1e16 + 1 - 1e16 is 0, not 1)
    T, basis, nonbasis = _blank(n, m)
    basis[1], nonbasis[0] = nonbasis[0], basis[1]            # y2 over column 0
    basis[3], nonbasis[2] = nonbasis[2], basis[3]            # y4 over column 2
    T[0, 0], T[0, 2] = -1.0, 1e16
    A = [[1e16, 1.0, 0.0, 1.0, 0.0, 0.0], [-1e16, -1.0, 0.0, -1.0, 0.0, 0.0]]
    out.append(("ascending columns", T, n, m, basis, nonbasis, A,
                {(0, 0): (1e16 + 1.0) - 1e16, (0, 1): (-1e16 - 1.0) + 1e16, (1, 0): -2.0,
                 (1, 1): 2.0, (n, 0): -6.0}))
    # label codes -1 and n + m: they name nothing and are recoded to -1; the coefficients the lost
    # labels would have named (y3, y5) stay unused
    T, basis, nonbasis = _blank(n, m)
    basis[2], basis[4] = -1, n + m
    nonbasis[0], nonbasis[2] = n + m, -1
    A = [[0.5, 0.25, 9.0, 0.75, 9.0, 1.0]]
    out.append(("codes outside", T, n, m, basis, nonbasis, A,
                {(p, 0): v for p, v in enumerate([0.5, 0.25, 0.0, 0.75, 0.0, 1.0])}))
    # no columns: W is T with "-b" in place
    T, basis, nonbasis = _y5_nonbasic(n, m)
    T[0, 0], T[n, 2], T[2, m] = nan, -0.0, -inf
    out.append(("no columns", T, n, m, basis, nonbasis, [], {}))
    return out


def check_handmade(case, W, basis_v, nonbasis_v):
    """`W` and the labels against `restate` by bit pattern (NaNs by position: a NaN's payload is
    outside the contract), and the pinned values, so that `restate` itself is held to the rule."""
    name, T, n, m, basis, nonbasis, A, pins = case
    exp, bexp, nexp = restate(T, n, m, basis, nonbasis, A)
    K = len(A)
    for (p, c), v in pins.items():
        assert su.same_floats(exp[p, m + c], v, nan_aware=True), (name, p, c, "restate()",
                                                                  float(exp[p, m + c]).hex())
    assert su.same_floats(W, exp, nan_aware=True), (name, "W")
    assert np.array_equal(basis_v, bexp) and np.array_equal(nonbasis_v, nexp), (name, "labels")
    assert nexp[m:].tolist() == [m + c for c in range(K)], name
    # columns 0..m-1 and the "-b" column: T's bits, NaN payloads included
    assert np.array_equal(su.bits(W[:, :m]), su.bits(T[:, :m])), name
    assert np.array_equal(su.bits(W[:, m + K]), su.bits(T[:, m])), name
