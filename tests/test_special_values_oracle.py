"""CPU: the special-value scenarios of special_values.py on the C oracle and the host engine.

(a) The census conditions for every (scenario, shape, seed, k) that test_gpu_special_values.py
    runs: the oracle finishes all k pivots, the table does not collapse to NaN, and each scenario
    still produces the event it is for (a NaN ratio on the first candidate at every step, pivot
    elements outside [2^-100, 2^101), ...).  Without them a generator change could leave the GPU
    comparisons passing on a NaN mask alone, or while testing nothing.
(b) The same scenarios through the host engine (smx_host_*), against the oracle.
Nothing here touches a GPU.
"""
from __future__ import annotations

import numpy as np
import pytest

import special_values as sv

CENSUS = sorted(sv.census_cases().items())


@pytest.mark.parametrize("case,mode", CENSUS,
                         ids=["{}-{}x{}-s{}-k{}".format(*c) for c, _ in CENSUS])
def test_census_conditions(case, mode):
    name, n, m, seed, k = case
    cen = sv.census(sv.scenario(name, n, m, seed), n, m, k)
    if mode == "loose":
        assert cen["done"] >= 1 and cen["nan_share"] <= 0.25, case
        return
    sv.check_census(name, n, m, k, cen, prefix=mode == "prefix")


def test_census_covers_what_the_issue_measured():
    """Every scenario is censused in full at the shapes its conditions were measured on, at both
    seeds (sprinkle: the two large shapes, less 700 x 900 with seed 6, see special_values.SKIP)."""
    full = {c for c, mode in sv.census_cases().items() if mode == "full"}
    for seed in sv.SEEDS:
        for name in sv.UNIFORM:
            for n, m, k in [(40, 40, 30), (63, 63, 30), (100, 100, 40), (130, 130, 40),
                            (200, 200, 40), (300, 260, 40), (700, 900, 50), (1023, 1023, 50)]:
                assert (name, n, m, seed, k) in full
        assert ("sprinkle", 1023, 1023, seed, 50) in full
    assert ("sprinkle", 700, 900, 5, 50) in full
    assert ("sprinkle", 700, 900, 6, 50) not in sv.census_cases()


def test_census_agrees_with_the_oracle_run():
    """The census steps pick + pivot itself: its final table, status and pivot count are those of
    smx_oracle_run, which the GPU tests compare against."""
    for name in sv.SCENARIOS:
        n, m, k = 130, 130, 40
        T, Tref, st, done, log = sv.reference(name, n, m, 5, k)
        cen = sv.census(T, n, m, k)
        assert (cen["status"], cen["done"]) == (st, done), name
        assert sv.same_bits_or_nan(cen["final"], Tref), name


@pytest.mark.parametrize("n,m", sv.FORCED)
def test_forced_update_input_keeps_its_values(n, m):
    """The forced pivots of the GPU test on the oracle: every table up to the inf element's holds
    non-finite values and at most a quarter NaN (measured: 0.02 to 0.04 before the last step), the
    2^-150 element is below the sweep's lower bound, and the inf element leaves NaN."""
    from oracle import c_oracle
    T, pivots = sv.forced_update_input(n, m)
    assert not np.isfinite(T).all() and (np.abs(T) == 5e-324).any()
    for r, c, plant in pivots:
        sv.forced_plant(T, r, c, plant)
        e = T[r, c]
        assert e != 0 and not np.isnan(e)
        assert np.isnan(T).mean() <= 0.25 and np.isinf(T).any() and np.isnan(T).any(), (r, c)
        T = c_oracle.pivot(T, r, c)
    assert [abs(p) for _, _, p in pivots[4:]] == [2.0 ** -150, np.inf]
    assert np.isnan(T).mean() > 0.9


def test_same_bits_or_nan():
    a = np.array([[0.0, -0.0, np.inf, -np.inf, np.nan, 1.5, 5e-324]])
    assert sv.same_bits_or_nan(a, a.copy())
    b = a.copy()
    b[0, 4] = -np.nan                       # NaN sign and payload are outside the contract
    b.view(np.int64)[0, 4] |= 12345
    assert np.isnan(b[0, 4]) and sv.same_bits_or_nan(b, a)
    for j, v in [(0, -0.0), (1, 0.0), (2, -np.inf), (3, np.inf), (4, 1.0), (5, np.nan),
                 (5, np.nextafter(1.5, 2.0)), (6, 0.0)]:
        b = a.copy()
        b[0, j] = v
        assert not sv.same_bits_or_nan(b, a), (j, v)
        assert sv.first_difference(b, a)[1] == (0, j)
    assert not sv.same_bits_or_nan(a[:, :3], a)
    assert sv.first_difference(a, a.copy()) is None


@pytest.mark.parametrize("name", sv.SCENARIOS)
@pytest.mark.parametrize("seed", sv.SEEDS)
def test_host_engine_vs_oracle(name, seed):
    """solve(record_history=False) on the host engine (smx_host_run, smx_host.hpp): pivot log,
    pivot count, status and table against the C oracle.  (sprinkle at this size holds few
    specials; its census conditions are for the large shapes, the comparison holds all the
    same.)"""
    import simplex
    n, m, k = sv.HOST
    T, Tref, st, done, log = sv.reference(name, n, m, seed, k)
    sm = simplex.SimplexMethod(T[:n].tolist(), T[n, :m].tolist(), device="cpu")
    assert sm.backend == "host"
    sm.solve(record_history=False, max_pivots=k, chunk=64)
    assert sm.pivots == done
    assert sm.pivot_log == [tuple(map(int, x)) for x in log]
    assert sm.status == {0: "cap", 1: "optimum", 2: "error", 3: "error"}[st]
    sv.same_table_as_oracle(sm._dev.download(), Tref, n, m, (name, seed))
