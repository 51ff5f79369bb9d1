"""CPU: branch and bound on solved LPs -- smx_host_branch against cuts_util's restatement and
smx_host_cuts with the two single-variable cuts, smx_host_branch_pick against branch_util's
restatement on hand-made columns with pinned results, and what SimplexMethod.solve_integer() means,
against brute force over every whole point, on the host engine.

The meaning set (branch_util.SEEDS, 200 small programs; max_pivots 256, max_depth 16) as run on
the host engine when this was written: 198 end "optimal", every one at the enumerated minimum, 2
end "limit" (seeds 1 and 158); 1808 nodes, 1744 warm pivots, the deepest tree 16 levels.
"""
from __future__ import annotations

import numpy as np
import pytest

import branch_util as bu
import cuts_util as cu
import ranging_util as ru
import solution_util as su


def _sm(cons, func):
    import simplex
    return simplex.SimplexMethod(cons, func, device="cpu")


# ----------------------------------------------------------------------------------------------
# the children
@pytest.mark.parametrize("k", range(len(ru.CASES)),
                         ids=[f"{c[0]}-{c[1]}x{c[2]}-s{c[3]}" for c in ru.CASES])
def test_host_branch_is_the_cuts_rule(k):
    """Every row of the oracle's final table whose label is a variable: both children equal
    cuts_util's restatement of the one cut and smx_host_cuts with it, by bit pattern, also with
    leading dimensions above m + 1."""
    _, n, m, _, _ = ru.CASES[k]
    ref = ru.case(k)
    basis, nonbasis, _ = su.replay(ref[5], n, m)
    T = ref[2]
    rows = [p for p in range(n) if basis[p] < m]
    assert rows, ru.CASES[k]
    for p in rows:
        down, up, bexp = bu.children(T, n, m, basis, nonbasis, p)
        for ld, ld_out in ((None, None), (m + 1 + 5, m + 1 + 3)):
            err, e0, e1, bgot = bu.host_branch(T, n, m, basis, nonbasis, p, ld=ld, ld_out=ld_out)
            assert err == 0
            cu.same_table(e0, down, (ru.CASES[k], p, "down", ld))
            cu.same_table(e1, up, (ru.CASES[k], p, "up", ld))
            assert np.array_equal(bgot, bexp) and bgot[n] == m + n
        for g, child in zip(bu.two_cuts(m, int(basis[p]), float(T[p][m])), (down, up)):
            err, viaC, _ = cu.host(T, n, m, basis, nonbasis, [g])
            assert err == 0
            cu.same_table(viaC, child, (ru.CASES[k], p, "smx_host_cuts"))
        # rows 0..n-1 and the f-row are T's bits; a fractional value violates both new rows
        assert np.array_equal(su.bits(down[:n]), su.bits(T[:n, :m + 1]))
        assert np.array_equal(su.bits(up[n + 1]), su.bits(T[n, :m + 1]))
        v = float(T[p][m])
        if np.isfinite(v) and v != np.floor(v):
            assert down[n, m] < 0 and up[n, m] < 0


def test_snap_writes_small_negative_constants_as_zero():
    """-snap <= v < 0 in the "-b" column of rows 0..n-1 becomes +0.0 in both children and nothing
    else moves; snap = 0 and a NaN snap nothing."""
    n, m = 5, 3
    T = np.arange(1.0, (n + 1) * (m + 1) + 1).reshape(n + 1, m + 1)
    basis = np.array([m, 0, m + 2, m + 3, m + 4], dtype=np.int32)
    nonbasis = np.array([m + 1, 1, 2], dtype=np.int32)
    T[:n, m] = [-1e-7, 2.5, -1e-6, -2e-6, -0.0]
    T[n, m] = -1e-9                                          # the f-row's constant is not a "-b"
    down, up, _ = bu.children(T, n, m, basis, nonbasis, 1)
    for snap in (0.0, float("nan")):
        err, e0, e1, _ = bu.host_branch(T, n, m, basis, nonbasis, 1, snap=snap)
        assert err == 0
        cu.same_table(e0, down, snap)
        cu.same_table(e1, up, snap)
    err, e0, e1, _ = bu.host_branch(T, n, m, basis, nonbasis, 1, snap=1e-6)
    assert err == 0
    cu.same_table(e0, bu.snapped(down, n, m, 1e-6), "down")
    cu.same_table(e1, bu.snapped(up, n, m, 1e-6), "up")
    assert su.bits(e0[:n, m]).tolist() == su.bits(np.array([0.0, 2.5, 0.0, -2e-6, -0.0])).tolist()
    assert e0[n + 1, m] == -1e-9


def test_host_branch_refusals():
    n, m = 3, 2
    T = np.ones((n + 1, m + 1))
    basis = np.array([m, 0, m + 2], dtype=np.int32)
    nonbasis = np.array([m + 1, 1], dtype=np.int32)
    assert bu.host_branch(T, n, m, basis, nonbasis, 1)[0] == 0
    for p in (-1, n, 0, 2):                                  # outside 0..n-1; a slack's row
        assert bu.host_branch(T, n, m, basis, nonbasis, p)[0] == -1, p
    from simplex_mi355x import _lib
    L = _lib.load()
    E = np.zeros((2, n + 2, m + 1))
    out = np.zeros(8)
    lab = np.zeros(n + 1, dtype=np.int32)
    ints = np.ones(m, dtype=np.int32)
    tp, bp, nbp = T.ctypes.data, basis.ctypes.data, nonbasis.ctypes.data

    def branch(ld=m + 1, ld_out=m + 1, t=tp, e0=E[0].ctypes.data):
        return L.smx_host_branch(t, ld, n, m, bp, nbp, 1, 0.0, e0, E[1].ctypes.data, ld_out,
                                 lab.ctypes.data)

    def pick(ld=m + 1, n_=n, m_=m, i=ints.ctypes.data):
        o = out.ctypes.data
        return L.smx_host_branch_pick(tp, ld, n_, m_, bp, i, 0.0, o, o + 8, o + 16, o + 24, o + 32)
    assert branch() == 0 and pick() == 0
    assert branch(ld=m) == -1 and branch(ld_out=m) == -1 and branch(t=None) == -1
    assert branch(e0=None) == -1
    assert pick(ld=m) == -1 and pick(n_=0) == -1 and pick(m_=0) == -1 and pick(i=None) == -1


# ----------------------------------------------------------------------------------------------
# the pick
HANDMADE = bu.handmade()


@pytest.mark.parametrize("case", HANDMADE, ids=[c[0] for c in HANDMADE])
def test_host_pick_on_handmade_columns(case):
    name, T, n, m, basis, ints, tol, _ = case
    for ld in (None, m + 4):
        err, got = bu.host_pick(T, n, m, basis, ints, tol, ld=ld)
        assert err == 0
        bu.check_handmade(case, got)


def test_handmade_columns_hold_their_events():
    names = [c[0] for c in HANDMADE]
    assert len(set(names)) == len(names) >= 12
    cols = np.concatenate([c[1][:c[2], c[3]] for c in HANDMADE])
    assert np.isnan(cols).any() and np.isposinf(cols).any() and np.isneginf(cols).any()
    assert (cols == 1e300).any() and any(v == 0 and np.signbit(v) for v in cols)
    assert any(c[6] == 0.0 for c in HANDMADE) and any(c[7][0] == -1 for c in HANDMADE)
    assert any((c[4] < 0).any() and (c[4] >= c[2] + c[3]).any() for c in HANDMADE)
    assert any((c[5] == 0).any() for c in HANDMADE)


def test_pick_on_oracle_tables():
    """The restatement and the twin agree on real final tables, with seeded masks; bneg and bmin
    are the first and the smallest negative constant of all rows."""
    for k in (1, 2, 5, 7):
        _, n, m, seed, _ = ru.CASES[k]
        ref = ru.case(k)
        basis, _, _ = su.replay(ref[5], n, m)
        for s in range(3):
            ints = (np.random.default_rng([seed, s]).random(m) < 0.7).astype(np.int32)
            for tol in (0.0, bu.TOL, 0.3):
                err, got = bu.host_pick(ref[2], n, m, basis, ints, tol)
                assert err == 0
                bu.same_pick(got, bu.pick(ref[2], n, m, basis, ints, tol), (k, s, tol))
    T = np.ones((4, 3))
    T[:3, 2] = [0.5, -2.0, -3.0]
    _, got = bu.host_pick(T, 3, 2, [2, 3, 4], [1, 1], bu.TOL)
    assert got == (-1, -1, 0.0, -2.0, -3.0)


# ----------------------------------------------------------------------------------------------
# what it means
def test_add_constraints_chains():
    """A warm chain of more than one stage: add_constraints accepts the result of
    add_constraints (it already did before solve_integer was added)."""
    sm = _sm([[-1.0, -2.0, 14.0], [-3.0, 1.0, 9.0], [-1.0, 1.0, 3.0]], [-3.0, -4.0])
    sm.solve(record_history=False)
    a = sm.add_constraints([[-1.0, 0.0, 3.0]])
    a.solve(record_history=False, rule="dual")
    b = a.add_constraints([[0.0, -1.0, 4.0]])
    b.solve(record_history=False, rule="dual")
    assert (a.status, b.status) == ("optimum", "optimum")
    assert a.solution().x.tolist() == [3.0, 5.5] and b.solution().x.tolist() == [3.0, 4.0]
    labels = b.column + b.row
    assert b.n == 5 and labels.count('y4') == 1 and labels.count('y5') == 1


PINNED = ([[-1.0, -1.0, 6.0], [-9.0, -5.0, 45.0]], [-8.0, -5.0])   # LP optimum (3.75, 2.25)


def test_pinned_two_variable_program():
    """minimise -8 x1 - 5 x2, x1 + x2 <= 6, 9 x1 + 5 x2 <= 45: the LP optimum (3.75, 2.25) rounds
    to (4, 2), which is infeasible; the whole optimum is (5, 0) at -40."""
    root = _sm(*PINNED)
    root.solve(record_history=False)
    assert np.allclose(root.solution().x, [3.75, 2.25], rtol=0, atol=1e-12)
    assert abs(root.solution().objective - -41.25) < 1e-12
    r = _sm(*PINNED).solve_integer()
    assert r.status == "optimal" and r.x.tolist() == [5.0, 0.0]
    assert r.objective == -40.0 and r.bound == -40.0
    assert r.nodes == 9 and r.warm_pivots == 7 and r.depth == 4
    assert abs(r.x_raw - r.x).max() < 1e-9


def test_integers_marking_some_variables():
    r = _sm(*PINNED).solve_integer(integers=[1, 0])
    assert r.status == "optimal" and r.x[0] == 4.0 and abs(r.x[1] - 1.8) < 1e-12
    assert abs(r.objective - -41.0) < 1e-12 and r.nodes == 3
    r = _sm(*PINNED).solve_integer(integers=[0, 1])
    assert r.status == "optimal" and r.x[1] == 2.0 and abs(r.x[0] - 35.0 / 9.0) < 1e-12
    r = _sm(*PINNED).solve_integer(integers=[0, 0])
    assert r.status == "optimal" and r.nodes == 1
    assert np.allclose(r.x, [3.75, 2.25], rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        _sm(*PINNED).solve_integer(integers=[1])


def test_an_infeasible_integer_program():
    """0.25 <= x1 <= 0.75: the LP is feasible, no whole point is."""
    cons = [[1.0, 0.0, -0.25], [-1.0, 0.0, 0.75], [0.0, -1.0, 3.0]]
    root = _sm(cons, [-1.0, -1.0])
    root.solve(record_history=False)
    assert root.status == "optimum" and root.solution().x.tolist() == [0.75, 3.0]
    r = _sm(cons, [-1.0, -1.0]).solve_integer()
    assert r.status == "infeasible" and r.x is None and r.objective == float("inf")
    assert r.bound == float("inf") and r.nodes == 3 and r.depth == 1


def test_a_limit():
    """The pinned program needs four levels: at max_depth = 1 the status is "limit" and the
    true optimum -40 lies between bound and objective; at 0 nothing but the root is solved."""
    r = _sm(*PINNED).solve_integer(max_depth=1)
    assert r.status == "limit" and r.depth == 1 and r.nodes == 3
    assert r.bound <= -40.0 <= r.objective and r.bound < r.objective
    assert r.x.tolist() == [3.0, 3.0] and r.objective == -39.0
    r = _sm(*PINNED).solve_integer(max_depth=0)
    assert r.status == "limit" and r.x is None and r.nodes == 1
    assert abs(r.bound - -41.25) < 1e-12 and r.objective == float("inf")
    r = _sm(*PINNED).solve_integer(warm_pivots=0)            # every warm run stops at its cap
    assert r.status == "limit" and abs(r.bound - -41.25) < 1e-12


def test_a_root_that_is_no_optimum_is_passed_through():
    r = _sm([[1.0, 1.0, -2.0], [-1.0, -1.0, 1.0]], [-1.0, -1.0]).solve_integer()
    assert r.status == "error" and r.x is None and r.nodes == 1
    r = _sm(*PINNED).solve_integer(max_pivots=1)
    assert r.status == "cap" and r.nodes == 1


def test_meaning_against_brute_force():
    """Seeds 0..199 on the host engine: the rounded x of every answer satisfies every constraint
    in integer arithmetic, every "optimal" is the enumerated minimum exactly, at most 5 % of the
    seeds end anywhere else, and a "limit" brackets the minimum."""
    other = []
    for seed in bu.SEEDS:
        A, b, c = bu.instance(seed)
        r = _sm(*bu.problem(A, b, c)).solve_integer(max_pivots=256, max_depth=16)
        best = bu.brute_of(seed)
        assert best is not None
        if r.x is not None:
            xi = np.rint(r.x).astype(np.int64)
            assert np.array_equal(xi.astype(np.float64), r.x), seed
            assert (xi >= 0).all() and (A @ xi <= b).all(), (seed, xi)
            assert r.objective == float(c @ xi), seed
        if r.status == "optimal":
            assert r.objective == float(best), (seed, r.objective, best)
        else:
            other.append(seed)
            assert r.status == "limit" and r.bound <= best <= r.objective, (seed, r)
    assert len(other) <= len(bu.SEEDS) // 20, other


def test_no_value_stands_near_the_tolerance():
    """No "-b" value of a marked variable at any visited node has d in (1e-9, 1e-3): the outcome of
    the meaning set does not hang on int_tol = 1e-6."""
    import simplex
    seen = []
    orig = simplex.SimplexMethod._branch_pick

    def spy(self, mask, tol):
        basis, _ = self._label_codes()
        T = self._dense_table()
        seen.extend(bu.frac(float(T[p, self.m])) for p in range(self.n) if basis[p] < self.m)
        return orig(self, mask, tol)

    simplex.SimplexMethod._branch_pick = spy
    try:
        for seed in bu.SEEDS:
            _sm(*bu.problem(*bu.instance(seed))).solve_integer(max_pivots=256, max_depth=16)
    finally:
        simplex.SimplexMethod._branch_pick = orig
    d = np.array(seen)
    assert len(d) > 1000 and not ((d > 1e-9) & (d < 1e-3)).any(), d[(d > 1e-9) & (d < 1e-3)][:5]
