"""What a what-if scenario of a final table is, restated in plain Python from the contract of
include/smx.h (smx_batch_scenario), for the tests of smx_host_scenario, k_batch_scenario,
solve_batch_scenarios and SimplexMethod.what_if(): the two ordered update steps in Python floats
(every product and every partial sum rounded once, no FMA, a delta equal to zero skipped), the
labels after a warm pivot log, the hand-made tables and the seeded deltas.  It works on the C
oracle's final table and on solution_util.replay's labels.  Everything compares by bit pattern.
"""
from __future__ import annotations

import numpy as np

import solution_util as su

inf, nan = float("inf"), float("nan")


def deltas(T0, n, m, seed, s, frac, prob):
    """Scenario s of the LP `T0` (the ORIGINAL table): normal deltas of `frac` times the mean
    magnitude of the constants / costs on a share `prob` of the entries, exact zeros elsewhere."""
    g = np.random.default_rng([seed, n, m, s])
    sr, sc = np.abs(T0[:n, m]).mean(), np.abs(T0[n, :m]).mean()
    return (g.normal(size=n) * frac * sr * (g.random(n) < prob),
            g.normal(size=m) * frac * sc * (g.random(m) < prob))


def restate(T, n, m, basis, nonbasis, function, drhs, dcost):
    """(S [n + 1][m + 1], func_s [m]) for the table `T` under the labels `basis` [n] /
    `nonbasis` [m]; `function` is the ORIGINAL objective (its first m entries are used)."""
    T = np.asarray(T, dtype=np.float64)
    S = T[:n + 1, :m + 1].copy()
    t = T.tolist()
    basis = [int(c) for c in basis]
    nonbasis = [int(c) for c in nonbasis]
    dr = [float(v) for v in drhs]
    dc = [float(v) for v in dcost]
    frow = []
    for j in range(m + 1):                                   # step 1: costs -> f-row
        v = t[n][j]
        if j < m and 0 <= nonbasis[j] < m and dc[nonbasis[j]] != 0:
            v = v + dc[nonbasis[j]]
        for p in range(n):
            k = basis[p]
            if 0 <= k < m and dc[k] != 0:
                v = v + dc[k] * t[p][j]
        frow.append(v)
    S[n, :] = frow
    for p in range(n + 1):                                   # step 2: constants -> "-b"
        row = t[p] if p < n else frow
        v = row[m]
        if p < n and m <= basis[p] < m + n and dr[basis[p] - m] != 0:
            v = v + dr[basis[p] - m]
        for j in range(m):
            c = nonbasis[j]
            if m <= c < m + n and dr[c - m] != 0:
                v = v - row[j] * dr[c - m]
        S[p, m] = v
    func_s = np.array([float(function[k]) + dc[k] if dc[k] != 0 else float(function[k])
                       for k in range(m)], dtype=np.float64)
    return S, func_s


def dot_variant(T, n, m, basis, nonbasis, drhs, dcost):
    """The same sums taken by np.dot over the same terms (S[n][:m] of step 1 and S[:n][m] of step
    2): what a tree or blocked reduction would give.  Only for the sharpness check."""
    T = np.asarray(T, dtype=np.float64)
    rows = [p for p in range(n) if 0 <= basis[p] < m and dcost[basis[p]] != 0]
    cols = [j for j in range(m) if m <= nonbasis[j] < m + n and drhs[nonbasis[j] - m] != 0]
    frow = T[n, :m].copy()
    for j in range(m):
        if 0 <= nonbasis[j] < m and dcost[nonbasis[j]] != 0:
            frow[j] += dcost[nonbasis[j]]
    if rows:
        frow = frow + np.dot(np.asarray(dcost)[np.asarray(basis)[rows]], T[rows, :m])
    b = T[:n, m].copy()
    for p in range(n):
        if m <= basis[p] < m + n and drhs[basis[p] - m] != 0:
            b[p] += drhs[basis[p] - m]
    if cols:
        b = b - np.dot(T[:n][:, cols], np.asarray(drhs)[np.asarray(nonbasis)[cols] - m])
    return frow, b


def host(T, n, m, basis, nonbasis, function, drhs, dcost, ld=None, ld_out=None):
    """smx_host_scenario on `T` (copied into a buffer of leading dimension `ld`, the gap filled
    with a value that would show) -> (return code, S [n + 1][m + 1], func_s [m]); the gap of the
    output buffer must come back untouched."""
    from simplex_mi355x import _lib
    T = np.asarray(T, dtype=np.float64)
    ld = ld or m + 1
    ld_out = ld_out or m + 1
    buf = np.full((n + 1, ld), 777.0)
    buf[:, :m + 1] = T[:n + 1, :m + 1]
    out = np.full((n + 1, ld_out), 555.0)
    fout = np.full(m, 7.0)
    basis = np.ascontiguousarray(basis, dtype=np.int32)
    nonbasis = np.ascontiguousarray(nonbasis, dtype=np.int32)
    func = np.ascontiguousarray(np.asarray(function, dtype=np.float64)[:m])
    dr = np.ascontiguousarray(drhs, dtype=np.float64)
    dc = np.ascontiguousarray(dcost, dtype=np.float64)
    err = _lib.load().smx_host_scenario(buf.ctypes.data, ld, n, m, basis.ctypes.data,
                                        nonbasis.ctypes.data, func.ctypes.data, dr.ctypes.data,
                                        dc.ctypes.data, out.ctypes.data, ld_out, fout.ctypes.data)
    assert (out[:, m + 1:] == 555.0).all()
    return err, out[:, :m + 1].copy(), fout


def same_table(got, exp, what):
    got = np.ascontiguousarray(got, dtype=np.float64)
    exp = np.ascontiguousarray(exp, dtype=np.float64)
    assert got.shape == exp.shape, what
    diff = np.argwhere(su.bits(got) != su.bits(exp))
    assert not len(diff), (what, [(int(p), int(j), float(got[p, j]).hex(), float(exp[p, j]).hex())
                                  for p, j in diff[:4]])


def warm_labels(basis0, nonbasis0, log, n, m):
    """The labels after the pivots of a warm `log`, started from `basis0` / `nonbasis0`."""
    basis = [int(c) for c in basis0[:n]]
    nonbasis = [int(c) for c in nonbasis0[:m]]
    for r, c in np.asarray(log).reshape(-1, 2).tolist():
        if 0 <= r < n and 0 <= c < m:
            basis[r], nonbasis[c] = nonbasis[c], basis[r]
    return np.array(basis, dtype=np.int32), np.array(nonbasis, dtype=np.int32)


def expected_solution(final, basis, nonbasis, n, m, func_s, pivots) -> su.Expected:
    """solution_util.expected for a table reached from given start labels: `basis` / `nonbasis`
    are the labels the table stands under."""
    final = np.asarray(final, dtype=np.float64)
    x = np.zeros(m, dtype=np.float64)
    duals = np.zeros(n, dtype=np.float64)
    for i in range(n):
        if 0 <= basis[i] < m:
            x[basis[i]] = final[i, m]
    for j in range(m):
        if m <= nonbasis[j] < m + n:
            duals[nonbasis[j] - m] = final[n, j]
    return su.Expected(x, duals, su.ordered_objective(func_s[:m], x), np.asarray(basis, np.int32),
                       np.asarray(nonbasis, np.int32), int(pivots))


def scenario_of_case(ref, n, m, seed, s, frac, prob):
    """(drhs, dcost, S, func_s, basis, nonbasis) of scenario s of a batch_util.case tuple."""
    T0, _flen, Tref, _st, _done, log = ref
    basis, nonbasis, _ = su.replay(log, n, m)
    drhs, dcost = deltas(T0, n, m, seed, s, frac, prob)
    S, func_s = restate(Tref, n, m, basis, nonbasis, T0[n, :m], drhs, dcost)
    return drhs, dcost, S, func_s, basis, nonbasis


# ----------------------------------------------------------------------------------------------
# Hand-made tables: what generators never produce.  Each is (name, T, n, m, basis, nonbasis,
# function, drhs, dcost, {(p, j): expected S value}); everything else follows from `restate`.
def _blank(n, m):
    """A = 1.0, "-b" = 2.0, f-row = 3.0, constant 0.5: finite, no zeros, identity labels."""
    T = np.ones((n + 1, m + 1))
    T[:n, m] = 2.0
    T[n, :m] = 3.0
    T[n, m] = 0.5
    return (T, np.arange(m, m + n, dtype=np.int32), np.arange(m, dtype=np.int32),
            np.arange(1.0, m + 1.0), np.zeros(n), np.zeros(m))


def handmade():
    out = []
    n, m = 5, 4
    # all deltas zero (of both signs): S is T's bits, whatever T holds
    T, basis, nonbasis, func, dr, dc = _blank(n, m)
    basis[4], nonbasis[1] = nonbasis[1], basis[4]            # x2 on row 4, y5 over column 1
    T[1, m], T[n, 2], T[n, m] = -0.0, -0.0, -0.0
    T[0, 0], T[2, 3], T[3, 1] = inf, nan, -inf
    dr[:] = [0.0, -0.0, 0.0, -0.0, -0.0]
    dc[:] = [-0.0, 0.0, -0.0, 0.0]
    out.append(("all zero", T, n, m, basis, nonbasis, func, dr, dc,
                {(1, m): -0.0, (n, 2): -0.0, (n, m): -0.0, (0, 0): inf, (3, 1): -inf}))
    # a changed non-basic variable (x1 over column 0) and a changed basic one (x2 on row 4)
    T, basis, nonbasis, func, dr, dc = _blank(n, m)
    basis[4], nonbasis[1] = nonbasis[1], basis[4]
    T[4, :] = [2.0, 4.0, -1.0, 0.5, 7.0]
    dc[0], dc[1] = 0.25, 2.0
    out.append(("cost basic and non-basic", T, n, m, basis, nonbasis, func, dr, dc,
                {(n, 0): 3.0 + 0.25 + 2.0 * 2.0, (n, 1): 3.0 + 2.0 * 4.0, (n, 2): 3.0 - 2.0,
                 (n, 3): 4.0, (n, m): 0.5 + 2.0 * 7.0}))
    # a changed slack of each kind: y1 on row 0 (basic), y5 over column 1 (non-basic)
    T, basis, nonbasis, func, dr, dc = _blank(n, m)
    basis[4], nonbasis[1] = nonbasis[1], basis[4]
    T[:, 1] = [1.0, -2.0, 0.5, 4.0, -1.0, 3.0]
    dr[0], dr[4] = 0.75, 2.0
    out.append(("rhs basic and non-basic", T, n, m, basis, nonbasis, func, dr, dc,
                {(0, m): 2.0 + 0.75 - 1.0 * 2.0, (1, m): 2.0 + 4.0, (2, m): 1.0, (3, m): -6.0,
                 (4, m): 4.0, (n, m): 0.5 - 6.0}))
    # the constant S[n][m] moves through both steps: x2 basic on row 4 with a cost delta, y5
    # over column 1 with an rhs delta; step 2 reads step 1's S[n][1]
    T, basis, nonbasis, func, dr, dc = _blank(n, m)
    basis[4], nonbasis[1] = nonbasis[1], basis[4]
    T[4, :] = [1.0, 4.0, 1.0, 1.0, 7.0]
    dc[1], dr[4] = 2.0, 0.5
    out.append(("constant through both steps", T, n, m, basis, nonbasis, func, dr, dc,
                {(n, 1): 3.0 + 8.0, (n, m): (0.5 + 14.0) - 11.0 * 0.5, (4, m): 7.0 - 4.0 * 0.5}))
    # a non-zero delta over a column holding +0.0 / -0.0 and over one holding inf
    T, basis, nonbasis, func, dr, dc = _blank(n, m)
    basis[4], nonbasis[1] = nonbasis[1], basis[4]
    T[:n, 1] = [0.0, -0.0, inf, -inf, 1.0]
    T[0, m], T[1, m] = -0.0, -0.0
    dr[4] = 3.0
    out.append(("delta over zeros and inf", T, n, m, basis, nonbasis, func, dr, dc,
                {(0, m): -0.0, (1, m): 0.0, (2, m): -inf, (3, m): inf, (4, m): -1.0}))
    # an inf on a changed basic variable's row
    T, basis, nonbasis, func, dr, dc = _blank(n, m)
    basis[4], nonbasis[1] = nonbasis[1], basis[4]
    T[4, :] = [inf, 0.0, -0.0, -inf, 1.0]
    T[n, 1], T[n, 2] = -0.0, -0.0
    dc[1] = -2.0
    out.append(("cost delta over zeros and inf", T, n, m, basis, nonbasis, func, dr, dc,
                {(n, 0): -inf, (n, 1): -0.0, (n, 2): 0.0, (n, 3): inf, (n, m): -1.5}))
    # NaN deltas: not equal to zero, applied
    T, basis, nonbasis, func, dr, dc = _blank(n, m)
    basis[4], nonbasis[1] = nonbasis[1], basis[4]
    dr[4], dc[0] = nan, nan
    out.append(("nan deltas", T, n, m, basis, nonbasis, func, dr, dc,
                {(0, m): nan, (n, 0): nan, (n, 1): 3.0, (n, m): nan}))
    # label codes -1 and n + m: they name nothing; the deltas the lost labels would have named
    # (y3, y5 / x1, x3) stay unused
    T, basis, nonbasis, func, dr, dc = _blank(n, m)
    basis[2], basis[4] = -1, n + m
    nonbasis[0], nonbasis[2] = n + m, -1
    dr[:] = [0.5, 0.0, 9.0, 0.0, 9.0]
    dc[:] = [9.0, 0.25, 9.0, 0.0]
    out.append(("codes outside", T, n, m, basis, nonbasis, func, dr, dc,
                {(0, m): 2.5, (2, m): 2.0, (4, m): 2.0, (n, 0): 3.0, (n, 1): 3.25, (n, 2): 3.0,
                 (n, m): 0.5}))
    return out


def check_handmade(case, S, func_s):
    """`S`, `func_s` against `restate` by bit pattern (NaNs by position: a NaN's payload is
    outside the contract), and the pinned values, so that `restate` itself is held to the rule."""
    name, T, n, m, basis, nonbasis, func, dr, dc, pins = case
    exp, fexp = restate(T, n, m, basis, nonbasis, func, dr, dc)
    for (p, j), v in pins.items():
        assert su.same_floats(exp[p, j], v, nan_aware=True), (name, p, j, "restate()",
                                                              float(exp[p, j]).hex())
    assert su.same_floats(S, exp, nan_aware=True), (name, "S")
    assert su.same_floats(func_s, fexp, nan_aware=True), (name, "func_s")
