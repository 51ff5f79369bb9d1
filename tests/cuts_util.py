"""What the extended table of a final table and a set of new constraints is, restated in plain
Python from the contract of include/smx.h (smx_batch_cuts), for the tests of smx_host_cuts,
k_batch_cuts, solve_batch_cuts and SimplexMethod.add_constraints(): the one ordered sum per column
in Python floats (every product and every partial sum rounded once, no FMA, a coefficient equal to
zero skipped), the hand-made tables and the seeded cut generator.  It works on the C oracle's final
table and on solution_util.replay's labels.  Everything compares by bit pattern.
"""
from __future__ import annotations

import numpy as np

import scenario_util as scu
import solution_util as su

inf, nan = float("inf"), float("nan")


def cut_set(T0, n, m, seed, s, K, viol, x_base):
    """Cut set s of the LP `T0` (the ORIGINAL table): K rows [a, constant] whose value at the base
    answer `x_base` is -d, d = +-`viol` times the mean magnitude of the constants, the sign
    alternating with q + s."""
    g = np.random.default_rng([seed, n, m, s, 77])
    rows = []
    for q in range(K):
        a = g.normal(size=m) * (g.random(m) < 0.75)
        if not a.any():
            a[0] = 1.0
        d = viol * abs(T0[:n, m]).mean() * (1 if (q + s) % 2 == 0 else -1)
        rows.append(list(a) + [-(a @ x_base) - d])
    return np.array(rows, dtype=np.float64).reshape(K, m + 1)


def restate(T, n, m, basis, nonbasis, G):
    """(E [n + K + 1][m + 1], basis_c [n + K]) for the table `T` under the labels `basis` [n] /
    `nonbasis` [m] and the cuts `G` [K][m + 1]."""
    T = np.asarray(T, dtype=np.float64)
    G = np.asarray(G, dtype=np.float64).reshape(-1, m + 1)
    K = len(G)
    E = np.empty((n + K + 1, m + 1), dtype=np.float64)
    E[:n] = T[:n, :m + 1]
    E[n + K] = T[n, :m + 1]
    t = T.tolist()
    basis = [int(c) for c in basis[:n]]
    nonbasis = [int(c) for c in nonbasis[:m]]
    for c in range(K):
        g = G[c].tolist()
        row = []
        for j in range(m + 1):
            if j == m:
                v = g[m]
            elif 0 <= nonbasis[j] < m:
                v = g[nonbasis[j]]
            else:
                v = 0.0
            for p in range(n):
                k = basis[p]
                if 0 <= k < m and g[k] != 0:
                    v = v + g[k] * t[p][j]
            row.append(v)
        E[n + c] = row
    return E, np.array(basis + [m + n + c for c in range(K)], dtype=np.int32)


def dot_variant(T, n, m, basis, nonbasis, g):
    """One new row's sums taken by np.dot over the same terms: what a tree or blocked reduction
    would give.  Only for the sharpness check."""
    T = np.asarray(T, dtype=np.float64)
    g = np.asarray(g, dtype=np.float64)
    rows = [p for p in range(n) if 0 <= basis[p] < m and g[basis[p]] != 0]
    start = np.array([g[nonbasis[j]] if 0 <= nonbasis[j] < m else 0.0 for j in range(m)] + [g[m]])
    if not rows:
        return start
    return start + np.dot(g[np.asarray(basis)[rows]], T[rows, :m + 1])


def host(T, n, m, basis, nonbasis, G, ld=None, ld_out=None):
    """smx_host_cuts on `T` (copied into a buffer of leading dimension `ld`, the gap filled with a
    value that would show) -> (return code, E [n + K + 1][m + 1], basis_c [n + K]); the gap of the
    output buffer must come back untouched."""
    from simplex_mi355x import _lib
    T = np.asarray(T, dtype=np.float64)
    G = np.ascontiguousarray(np.asarray(G, dtype=np.float64).reshape(-1, m + 1))
    K = len(G)
    ld = ld or m + 1
    ld_out = ld_out or m + 1
    buf = np.full((n + 1, ld), 777.0)
    buf[:, :m + 1] = T[:n + 1, :m + 1]
    out = np.full((n + K + 1, ld_out), 555.0)
    bout = np.full(n + K, 77, dtype=np.int32)
    basis = np.ascontiguousarray(basis, dtype=np.int32)
    nonbasis = np.ascontiguousarray(nonbasis, dtype=np.int32)
    err = _lib.load().smx_host_cuts(buf.ctypes.data, ld, n, m, basis.ctypes.data,
                                    nonbasis.ctypes.data, G.ctypes.data if K else None, K,
                                    out.ctypes.data, ld_out, bout.ctypes.data)
    assert (out[:, m + 1:] == 555.0).all()
    return err, out[:, :m + 1].copy(), bout


def enlarged(T0, n, m, G):
    """The ORIGINAL table with the cuts appended as constraints n..n+K-1, the f-row below them."""
    G = np.asarray(G, dtype=np.float64).reshape(-1, m + 1)
    return np.vstack([T0[:n, :m + 1], G, T0[n:n + 1, :m + 1]])


def base_of_case(ref, n, m):
    """(basis, nonbasis, x) of a batch_util.case tuple's base run."""
    basis, nonbasis, _ = su.replay(ref[5], n, m)
    return basis, nonbasis, su.of_case(ref, n, m).x


def cuts_of_case(ref, n, m, seed, s, K, viol=0.05):
    """(G, E, basis_c, basis, nonbasis) of cut set s with K cuts of a batch_util.case tuple."""
    basis, nonbasis, x = base_of_case(ref, n, m)
    G = cut_set(ref[0], n, m, seed, s, K, viol, x)
    E, basis_c = restate(ref[2], n, m, basis, nonbasis, G)
    return G, E, basis_c, basis, nonbasis


same_table = scu.same_table
warm_labels = scu.warm_labels
expected_solution = scu.expected_solution


# ----------------------------------------------------------------------------------------------
# Hand-made tables: what generators never produce.  Each is (name, T, n, m, basis, nonbasis, G,
# {(kappa, j): expected value of E[n + kappa][j]}); everything else follows from `restate`.
def _blank(n, m):
    T, basis, nonbasis, _, _, _ = scu._blank(n, m)
    return T, basis, nonbasis


def _x2_basic(n, m):
    """x2 on row 4 (T[4] = 2, 4, -1, 0.5 | 7), y5 over column 1."""
    T, basis, nonbasis = _blank(n, m)
    basis[4], nonbasis[1] = nonbasis[1], basis[4]
    T[4, :] = [2.0, 4.0, -1.0, 0.5, 7.0]
    return T, basis, nonbasis


def handmade():
    out = []
    n, m = 5, 4
    # coefficients +0.0 and -0.0 on a basic variable whose row holds inf, NaN and -0.0: skipped
    T, basis, nonbasis = _x2_basic(n, m)
    basis[0], nonbasis[0] = nonbasis[0], basis[0]            # x1 on row 0, y1 over column 0
    T[0, :] = [inf, nan, -0.0, -inf, inf]
    G = [[0.0, 2.0, 0.0, 0.0, 1.0], [-0.0, 2.0, 0.0, -0.0, 1.0]]
    pins = {(c, j): v for c in (0, 1) for j, v in enumerate([4.0, 8.0, -2.0, 1.0, 15.0])}
    out.append(("zero coefficients over inf and nan", T, n, m, basis, nonbasis, G, pins))
    # a -0.0 coefficient on a non-basic variable: the cut's own bits under identity labels
    T, basis, nonbasis = _blank(n, m)
    G = [[-0.0, 0.0, 1.5, -0.0, -0.0]]
    out.append(("own bits", T, n, m, basis, nonbasis, G,
                {(0, j): v for j, v in enumerate(G[0])}))
    # NaN and inf coefficients: not equal to zero, applied
    T, basis, nonbasis = _x2_basic(n, m)
    G = [[nan, inf, 0.0, 0.0, 1.0], [0.0, nan, 0.0, 0.0, 1.0], [0.0, -inf, 0.0, 0.0, 1.0]]
    pins = {(0, 0): nan, (0, 1): inf, (0, 2): -inf, (0, 3): inf, (0, m): inf}
    pins.update({(1, j): nan for j in range(m + 1)})
    pins.update({(2, 0): -inf, (2, 2): inf, (2, m): -inf})
    out.append(("nan and inf coefficients", T, n, m, basis, nonbasis, G, pins))
    # one variable non-basic (x1 over column 0), one basic (x2 on row 4)
    T, basis, nonbasis = _x2_basic(n, m)
    G = [[0.25, 2.0, 0.0, 0.0, -3.0]]
    out.append(("basic and non-basic", T, n, m, basis, nonbasis, G,
                {(0, 0): 0.25 + 4.0, (0, 1): 8.0, (0, 2): -2.0, (0, 3): 1.0, (0, m): 11.0}))
    # two basic variables: the sum runs in ascending row order (1e16 + 1 - 1e16 is 0, not 1)
    T, basis, nonbasis = _blank(n, m)
    basis[1], nonbasis[0] = nonbasis[0], basis[1]            # x1 on row 1
    basis[3], nonbasis[2] = nonbasis[2], basis[3]            # x3 on row 3
    T[1, :], T[3, :] = [1.0, 1.0, 1.0, 1.0, 1.0], [1e16, 2.0, -1.0, 0.5, 1.0]
    G = [[1.0, 0.0, -1.0, 0.0, 1e16], [-1.0, 0.0, 1.0, 0.0, -1e16]]
    out.append(("ascending rows", T, n, m, basis, nonbasis, G,
                {(0, 0): (0.0 + 1.0) - 1e16, (0, m): (1e16 + 1.0) - 1.0, (0, 1): -1.0,
                 (1, 0): (0.0 - 1.0) + 1e16, (1, m): (-1e16 - 1.0) + 1.0}))
    # label codes -1 and n + m: they name nothing; the coefficients the lost labels would have
    # named (x1, x3) stay unused
    T, basis, nonbasis = _blank(n, m)
    basis[2], basis[4] = -1, n + m
    nonbasis[0], nonbasis[2] = n + m, -1
    G = [[9.0, 0.25, 9.0, 0.5, 1.0]]
    out.append(("codes outside", T, n, m, basis, nonbasis, G,
                {(0, 0): 0.0, (0, 1): 0.25, (0, 2): 0.0, (0, 3): 0.5, (0, m): 1.0}))
    # no cuts: E is T
    T, basis, nonbasis = _x2_basic(n, m)
    T[0, 0], T[n, 2], T[2, m] = nan, -0.0, -inf
    out.append(("no cuts", T, n, m, basis, nonbasis, [], {}))
    return out


def check_handmade(case, E, basis_c):
    """`E`, `basis_c` against `restate` by bit pattern (NaNs by position: a NaN's payload is
    outside the contract), and the pinned values, so that `restate` itself is held to the rule."""
    name, T, n, m, basis, nonbasis, G, pins = case
    exp, bexp = restate(T, n, m, basis, nonbasis, G)
    K = len(G)
    for (c, j), v in pins.items():
        assert su.same_floats(exp[n + c, j], v, nan_aware=True), (name, c, j, "restate()",
                                                                  float(exp[n + c, j]).hex())
    assert su.same_floats(E, exp, nan_aware=True), (name, "E")
    assert np.array_equal(basis_c, bexp), (name, "labels")
    assert bexp[n:].tolist() == [m + n + c for c in range(K)], name
    # rows 0..n-1 and the f-row: T's bits, NaN payloads included
    assert np.array_equal(su.bits(E[:n]), su.bits(T[:n])), name
    assert np.array_equal(su.bits(E[n + K]), su.bits(T[n])), name
