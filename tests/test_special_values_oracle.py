"""CPU: the special-value scenarios of special_values.py on the C oracle and the host engine.

(a) The census conditions for every (scenario, shape, seed, k) that test_gpu_special_values.py
    runs: the oracle finishes all k pivots, the table does not collapse to NaN, and each scenario
    still produces the event it is for (a NaN ratio on the first candidate at every step, pivot
    elements outside [2^-100, 2^101), ...).  Without them a generator change could leave the GPU
    comparisons passing on a NaN mask alone, or while testing nothing.
(b) The same scenarios through the host engine (smx_host_*), against the oracle.
(c) The row-pair sweep layout (sweep form 7), which test_gpu_block_pairs.py runs with one sweep
    workgroup per CU: the pair census (special_values.pair_census: which pairs of a wave's rows
    take the pair fast path, which go row by row, which rows are odd tails) finds what
    PAIR_CONDITIONS asks on every PAIRS case, on the fast-path edge table and on mixed_pair_table
    at 256 CUs, and the census itself is checked on a clean table, on planted values and on a
    geometry written out by hand.
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


# ----------------------------------------------------------------------------------------------
# the row-pair sweep layout: what test_gpu_block_pairs.py's tables make its pairs do
CUS = 256   # an MI355X; the GPU tests evaluate the same conditions at the device's own count


@pytest.mark.parametrize("name,n,m,seed,P", sv.PAIRS,
                         ids=["{}-{}x{}-s{}-P{}".format(*c) for c in sv.PAIRS])
def test_pair_conditions(name, n, m, seed, P):
    """PAIR_CONDITIONS for every PAIRS case, and the census's own run is the oracle's."""
    cen = sv.pair_case_census(name, n, m, seed, P, CUS)
    sv.check_pair_census(name, n, m, sv.block_k(P), cen)
    _, Tref, st, done, _ = sv.reference(name, n, m, seed, sv.block_k(P))
    assert (cen["status"], cen["done"]) == (st, done)
    assert sv.same_bits_or_nan(cen["final"], Tref)


def test_pairs_list():
    """PAIRS: every scenario at 700 x 900 with 13 and 24 pivots per sweep, the sharp ones at
    1023^2 with 20, both seeds; each has its census case in prefix mode."""
    assert len(set(sv.PAIRS)) == len(sv.PAIRS) == 6 * 2 * 2 + 3 * 2
    for seed in sv.SEEDS:
        for name in sv.SCENARIOS:
            for P in (13, 24):
                assert (name, 700, 900, seed, P) in sv.PAIRS
        for name in ("inf_b", "nan_later", "sprinkle"):
            assert (name, 1023, 1023, seed, 20) in sv.PAIRS
    cases = sv.census_cases()
    for name, n, m, seed, P in sv.PAIRS:
        assert cases[name, n, m, seed, 2 * P + 3] == "prefix"


@pytest.mark.parametrize("P", [13, 20, 24])
@pytest.mark.parametrize("n,m", [(1023, 1023), (1000, 1100)])
def test_pair_conditions_edge_table(n, m, P):
    """The fast-path edge table over 4 P + 3 pivots: the oracle runs them all to a finite table,
    fast pairs and mixed pairs both occur (and both kinds of odd tail at 1000 x 1100)."""
    T = sv.fast_path_edge_table(n, m)
    cen = sv.pair_census(T, n, m, sv.edge_chain(P), CUS)
    sv.check_pair_census("table", n, m, 4 * P + 3, cen)
    assert np.isfinite(cen["final"]).all()
    assert (len(cen["odd"]) > 0) == (n == 1000)


@pytest.mark.parametrize("P", [20, 24])
@pytest.mark.parametrize("n,m", sorted(sv.MIXED_PAIR_SEEDS))
def test_pair_conditions_mixed_pair_table(n, m, P):
    """mixed_pair_table at the seeds of MIXED_PAIR_SEEDS over 2 P + 3 pivots: both pair classes
    occur (in the ragged block of 4: the two long blocks have no free chunk and send every pair
    row by row, which is what the table is for)."""
    T = sv.mixed_pair_table(n, m, sv.MIXED_PAIR_SEEDS[n, m])
    cen = sv.pair_census(T, n, m, sv.pair_chain(P), CUS)
    sv.check_pair_census("table", n, m, 2 * P + 3, cen)
    assert [b["free_chunks"] for b in cen["blocks"][:2]] == [0, 0]
    # unbounded multipliers (flag 0) in every block: the scaled third of the 1000 rows at least,
    # less the block's pivot rows; flag-1 rows beside them in the free block
    assert all((b["flags"] == 0).sum() >= 300 for b in cen["blocks"])
    assert (cen["blocks"][2]["flags"] == 1).sum() >= 300


def test_pair_geometry_by_hand():
    """sweep_grid_lds and blk_geom_wg on small numbers, and the shapes the GPU tests use."""
    # 2 CUs, 200 columns: 2 chunks, one workgroup each, 4 waves -> stride 4
    assert sv.pair_geometry(11, 200, 2) == (2, 4)
    pairs, odd = sv.wave_pairs(11, 4)
    assert pairs == [(0, 4), (1, 5), (2, 6), (3, 7)] and odd == [8, 9, 10]
    # 4 rows per wave: two pairs, no tail; 5: an odd tail for every wave that has a fifth row
    assert sv.wave_pairs(8, 2) == ([(0, 2), (4, 6), (1, 3), (5, 7)], [])
    assert sv.wave_pairs(9, 2) == ([(0, 2), (4, 6), (1, 3), (5, 7)], [8])
    # more workgroups than rows: at most ceil(R / 4) per chunk, every row alone
    assert sv.pair_geometry(5, 100, 256) == (1, 8)
    assert sv.wave_pairs(5, 8) == ([], [0, 1, 2, 3, 4])
    # fewer CUs than chunks: one workgroup per chunk all the same
    assert sv.pair_geometry(100, 1000, 2) == (8, 4)
    assert sv.pair_geometry(701, 901, 256) == (8, 128)
    assert sv.pair_geometry(1024, 1024, 256) == (8, 128)
    assert sv.pair_geometry(1001, 1024, 256) == (8, 128)
    assert sv.pair_geometry(1001, 1101, 256) == (9, 112)
    assert sv.pair_geometry(1024, 1024, 256, 8) == (8, 1024)   # the default grid: single rows
    for R, qs in [(701, 128), (1001, 112), (1024, 128)]:
        pairs, odd = sv.wave_pairs(R, qs)
        rows = sorted([r for p in pairs for r in p] + odd)
        assert rows == list(range(R))
        assert all(b - a == qs for a, b in pairs)
        # a wave has R // qs rows, the first R % qs waves one more
        assert len(odd) == (R % qs if (R // qs) % 2 == 0 else qs - R % qs)
    assert len(sv.wave_pairs(1024, 128)[1]) == 0 and len(sv.wave_pairs(701, 128)[1]) == 67


def test_pair_census_on_a_clean_table():
    """A uniform table (every value bounded, every chunk free): the units that are not fast are
    exactly the pivot rows of each block, so a pair is mixed exactly when it holds one pivot row,
    slow when it holds two, and an odd tail is slow exactly when it is a pivot row -- in every
    chunk alike.  With 2 CUs the pairing is the one written out by hand."""
    from oracle import c_oracle
    from simplex_mi355x import lp
    n, m, blocks = 42, 300, [13, 12, 4]
    T = lp.dense_tableau("uniform", 5, n, m)
    cen = sv.pair_census(T, n, m, blocks, cus=2)
    assert cen["geometry"] == (3, 4) and cen["status"] == 0 and cen["done"] == 29
    assert cen["pairs"] == [(b + 8 * t, b + 8 * t + 4) for b in range(4) for t in range(6)
                            if b + 8 * t + 4 <= 42]
    assert cen["odd"] == [40, 41, 42]
    Tref, st, done, log = c_oracle.run(T, n, m, m, 29)
    assert np.array_equal(cen["final"].view(np.int64), Tref.view(np.int64))
    k = 0
    for P, blk in zip(blocks, cen["blocks"]):
        prows = {int(r) for r, _ in log[k:k + P]}
        k += P
        assert set(blk["pivot_rows"]) == prows
        assert blk["free_chunks"] == 3
        assert set(np.nonzero(blk["flags"] == 2)[0]) == prows
        assert ((blk["flags"] == 1) | (blk["flags"] == 2)).all()
        assert np.array_equal(blk["fast"], np.repeat((blk["flags"] == 1)[:, None], 3, axis=1))
        held = [len(prows & {a, b}) for a, b in cen["pairs"]]
        assert blk["both"] == 3 * held.count(0)
        assert blk["one"] == 3 * held.count(1)
        assert blk["neither"] == 3 * held.count(2)
        assert blk["odd_slow"] == 3 * len(prows & set(cen["odd"]))
        assert blk["odd_fast"] == 3 * len(set(cen["odd"]) - prows)
        assert held.count(1) >= 1
        assert blk["vote_a"] == blk["vote_b"] == 0
        assert blk["both_phase2"] == (blk["both"] if P > 12 else 0)
    for a in sv.PAIR_COUNTS:
        assert cen[a] == sum(b[a] for b in cen["blocks"])


def test_pair_census_sees_planted_values():
    """One block of 5 pivots on the same table with values planted beside the pivots: an inf
    input makes its one unit slow, a zero multiplier flags its row 3, an unbounded multiplier 0,
    a pivot-row value below 2^-100 takes its chunk."""
    from oracle import c_oracle
    from simplex_mi355x import lp
    n, m, P = 42, 300, 5
    T = lp.dense_tableau("uniform", 5, n, m)
    _, _, _, log = c_oracle.run(T, n, m, m, P)
    prows, pcols = {int(r) for r, _ in log}, [int(c) for _, c in log]
    free_rows = [i for i in range(n) if i not in prows]
    free_col = next(j for j in range(128, 256) if j not in pcols)
    i_inf, i_zero, i_big = free_rows[:3]
    T[i_inf, free_col] = np.inf
    T[i_zero, pcols[0]] = -0.0
    T[i_big, pcols[0]] = 2.0 ** 101
    r0 = int(log[0][0])
    tiny_col = next(j for j in range(256, 300) if j not in pcols)
    T[r0, tiny_col] = 2.0 ** -101
    cen = sv.pair_census(T, n, m, [P], cus=2)
    assert cen["status"] == 0
    blk = cen["blocks"][0]
    # none of the plants is a ratio or f-row candidate that changes the first pivots' choice
    assert blk["pivot_rows"] == [int(r) for r, _ in log]
    assert blk["flags"][i_inf] == 1 and blk["flags"][i_zero] == 3 and blk["flags"][i_big] == 0
    assert list(blk["fast"][i_inf]) == [True, False, False]
    assert not blk["fast"][i_zero].any() and not blk["fast"][i_big].any()
    assert blk["free_chunks"] == 2
    ok = [i for i in range(n + 1) if blk["flags"][i] == 1 and i != i_inf]
    assert blk["fast"][ok][:, :2].all() and not blk["fast"][:, 2].any()
    # the inf is the one input that fails a vote: counted for its pair, on its side of it
    mate = [(a, b) for a, b in cen["pairs"] if i_inf in (a, b)]
    want = [0, 0]
    if mate and blk["flags"][mate[0][0]] == blk["flags"][mate[0][1]] == 1:
        want[mate[0].index(i_inf)] = 1
    assert [blk["vote_a"], blk["vote_b"]] == want


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
