"""GPU parity of the row-pair sweep layout (smx_tune_block_form(7), blk_sweep_body_flag<P, 7> in
csrc/smx_sweep.hpp): a lane keeps two rows of its two columns, so each LDS read of a pivot's row
slice and of (e, y) feeds four chains, and the rows' multipliers arrive in phases of 12 pivots.

Bit-exact against the C oracle with pairs, odd tails and mixed pairs (rows of one pair on
different paths), against the one-row LDS layout (form 5) at 16 rows per wave, and over the
trajectory fixtures (tiny tables: the single-row tail only).

Small tables give a wave fewer than two rows under the default grid of 8 workgroups per CU, so the
oracle cases run the sweep with one workgroup per CU (smx_tune_set(-2, 1)): at n = 1000 rows and
8 or 9 column chunks a wave then owns 7-9 rows.

What exists only in the pair layout -- the one vote over a pair's four inputs, the odd last row,
the second phase's reload of both rows' multipliers, the row-by-row fallback run from inside the
pair loop's prefetch rotation -- also sees NaN, inf, denormals and 2^+-150 values here, with real
pairs, at 13, 20 and 24 pivots per sweep:
  * special_values.PAIRS, every planner: inf_b, nan_later and sprinkle put fast pairs and pairs
    with exactly one fast row side by side; nan_first, cols150 and rows150 send every pair row by
    row.  700 x 900 gives most waves two pairs and an odd tail and a ragged last chunk, 1023^2
    exactly four pairs per wave.
  * the fast-path edge table of test_gpu_block.py (rows past 2^101 and at 2^-60, columns at
    2^-99, zero and -0 blocks) at 1023^2 and 1000 x 1100, 4 P + 3 pivots;
  * mixed_pair_table at 20 and 24 pivots per sweep, and on two simulated ranks;
  * sprinkle under forms 5, 6 and 7.
Which path each pair takes is counted on the CPU by special_values.pair_census, and every test
that relies on a mix first checks PAIR_CONDITIONS at the device's own CU count, so a geometry that
moved fails by name.  At 256 CUs the census finds, as (both rows fast, exactly one, neither)
(pair, chunk) units summed over a run, seeds 5 / 6:
  nan_first, cols150, rows150  700 x 900  P = 13 and 24   0, 0, 7608 throughout
  nan_later  700 x 900   P = 13   3704, 1109, 2795 / 3650, 1105, 2853
                         P = 24   3698, 1121, 2789 / 3635, 1111, 2862
  inf_b      700 x 900   P = 13   7141, 417, 50 / 7198, 362, 48
                         P = 24   7082, 471, 55 / 7135, 424, 49
  sprinkle   700 x 900   P = 13   1992, 215, 5401 / 6280, 987, 341
                         P = 24   1708, 184, 5716 / 5982, 965, 661
  inf_b      1023^2      P = 20   11551, 668, 69 / 11608, 606, 74
  nan_later  1023^2      P = 20   4598, 1530, 6160 / 6068, 2613, 3607
  sprinkle   1023^2      P = 20   2551, 503, 9234 / 4350, 737, 7201
(700 x 900: 1608 odd-tail units per run, 46 to 1227 of them not fast in the sharp scenarios.)
Of the mixed units of the nine sharp lines, 24 to 442 per run are held off the fast path by the
vote alone through row a's inputs and 42 to 394 through row b's (a vote over one row would take
them), and 756 to 7702 fast pairs lie in blocks of more than 12 pivots (a second phase reading the
other row's multipliers would change them): PAIR_CONDITIONS asks for at least one of each.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import special_values as sv
from golden_util import trajectory_cap, trajectory_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


@pytest.fixture
def block_mode():
    """Set smx_tune_block for one test (resident loop off, so small tables take the block path)
    and restore both policies afterwards."""
    from simplex_mi355x import _lib
    prev_b = _lib.tune_block(-1)
    prev_r = _lib.tune_resident(-2)
    _lib.tune_resident(-1)
    yield _lib.tune_block
    _lib.tune_block(prev_b)
    _lib.tune_resident(prev_r)


@pytest.fixture
def sweep_form():
    from simplex_mi355x import _lib
    prev = _lib.tune_block_form(-1)
    yield _lib.tune_block_form
    _lib.tune_block_form(prev)


@pytest.fixture
def small_grid():
    """One sweep workgroup per CU (smx_tune_set(-2, 1)); the previous override afterwards."""
    from simplex_mi355x import _lib
    lib = _lib.load()
    prev = ctypes.c_int32(0)
    _lib.check(lib.smx_tune_get(None, ctypes.byref(prev), None, None, None, None), "smx_tune_get")
    _lib.check(lib.smx_tune_set(-2, 1), "smx_tune_set")
    yield
    _lib.check(lib.smx_tune_set(-2, prev.value), "smx_tune_set")


@pytest.fixture
def planner():
    """Set smx_tune_block_planner (planner, window slots) for one test."""
    from simplex_mi355x import _lib
    prev = _lib.tune_block_planner(-1, -1)
    yield _lib.tune_block_planner
    _lib.tune_block_planner(prev, 0)


def _chunks(P):
    """2 P + 3 pivots in three chains of one block each: P (two phases past 12), P - 1 (the other
    parity: one of the two is in place, the other out of place) and a ragged last block of 4."""
    return sv.pair_chain(P)


def _run_vs_oracle(T, n, m, P):
    from oracle import c_oracle
    import simplex
    sm = simplex.SimplexMethod(T[:n].tolist(), T[n, :m].tolist())
    assert sm._dev.block_plan()[1] == P
    k = 0
    for c in _chunks(P):
        sm.solve(record_history=False, max_pivots=c, chunk=c)
        k += c
    assert k == 2 * P + 3
    Tref, st, done, log = c_oracle.run(T, n, m, m, k, threads=8)
    assert done == k, "the LP must run all k pivots (no terminal outcome): change the seed"
    assert sm.pivots == done
    assert sm.pivot_log == [tuple(map(int, x)) for x in log]
    got = sm._dev.download()
    assert np.array_equal(got[:n].view(np.int64), Tref[:n].view(np.int64))
    assert np.array_equal(got[n, :m].view(np.int64), Tref[n, :m].view(np.int64))


SEED = 11


@pytest.mark.parametrize("kind", ["uniform", "degenerate", "mixed"])
@pytest.mark.parametrize("P", [8, 13, 24])
@pytest.mark.parametrize("n,m", [(1000, 1023), (1000, 1100)])
def test_pairs_vs_oracle(block_mode, sweep_form, small_grid, n, m, P, kind):
    """Pivot log and the whole table as int64 bits.  m = 1023: 8 chunks, 7-8 rows per wave (pairs
    plus odd tails); m = 1100: 9 chunks, the last one ragged.  P = 8 one phase, 13 = 12 + 1,
    24 = 12 + 12; `degenerate` and `mixed` bring zeros, flag-3 rows and phase 1."""
    from simplex_mi355x import lp
    sweep_form(7)
    block_mode(P)
    _run_vs_oracle(lp.dense_tableau(kind, SEED, n, m), n, m, P)


def mixed_pair_table(n, m):
    """special_values.mixed_pair_table at this file's seed."""
    return sv.mixed_pair_table(n, m, SEED)


def test_mixed_pairs_vs_oracle(block_mode, sweep_form, small_grid):
    sweep_form(7)
    block_mode(13)
    n, m = 1000, 1023
    _run_vs_oracle(mixed_pair_table(n, m), n, m, 13)


@pytest.mark.parametrize("m", [1023, 1100])
def test_forms_agree_on_mixed_paths(block_mode, sweep_form, small_grid, m):
    """mixed_pair_table under every sweep layout (forms 4, 5, 6, 7), 13 pivots per sweep, 2 x 13 + 3
    pivots cut as _chunks(13): the four pivot logs and the four tables' bits are equal, and form
    5's equal the C oracle's.  A wave owns 7-9 rows, so both register sets of each prefetch loop
    rotate, with an odd tail, a ragged last chunk (m = 1100) and a second pair phase of one pivot;
    the rows fall on every sweep path.  (Form 4 runs as form 5 where its wave count does not
    divide: nothing here depends on which kernel ran.)"""
    from oracle import c_oracle
    import simplex
    n, P = 1000, 13
    T = mixed_pair_table(n, m)
    block_mode(P)
    k = sum(_chunks(P))
    out = {}
    for form in (4, 5, 6, 7):
        sweep_form(form)
        sm = simplex.SimplexMethod(T[:n].tolist(), T[n, :m].tolist())
        assert sm._dev.block_plan()[1] == P
        for c in _chunks(P):
            sm.solve(record_history=False, max_pivots=c, chunk=c)
        out[form] = (sm.pivots, list(sm.pivot_log), sm._dev.download().view(np.int64).copy())
    Tref, st, done, log = c_oracle.run(T, n, m, m, k, threads=8)
    assert done == k, "the LP must run all k pivots (no terminal outcome)"
    assert out[5][0] == done
    assert out[5][1] == [tuple(map(int, x)) for x in log]
    assert np.array_equal(out[5][2][:n], Tref[:n].view(np.int64))
    assert np.array_equal(out[5][2][n, :m], Tref[n, :m].view(np.int64))
    for form in (4, 6, 7):
        assert out[form][0] == out[5][0], form
        assert out[form][1] == out[5][1], form
        assert np.array_equal(out[form][2], out[5][2]), form


def test_form7_equals_form5(block_mode, sweep_form):
    """4095 x 4095 uniform under the default grid (16 rows per wave), 24 pivots per sweep, 48
    pivots: the pair layout's table equals the one-row LDS layout's bit for bit."""
    from simplex_mi355x import lp
    from simplex_mi355x.device import DeviceTableau
    n = m = 4095
    k = 48
    T = lp.dense_tableau("uniform", 3, n, m)
    block_mode(24)
    out = {}
    for form in (5, 7):
        sweep_form(form)
        dev = DeviceTableau(T, n, m, m)
        assert dev.block_plan()[1] == 24
        dev.run(k, graph=False)
        ctl = dev.sync_state()
        assert int(ctl["npivots"]) == k
        out[form] = (dev.read_log(0, k).copy(), dev.download().view(np.int64).copy())
        dev.close()
    assert np.array_equal(out[5][0], out[7][0])
    assert np.array_equal(out[5][1], out[7][1])


def test_every_fixture_form7(block_mode, sweep_form):
    """Every trajectory fixture at 13 pivots per sweep in the pair layout (the default planner):
    the block chain equals the one-pivot chain and the reference's pivots.  The tables are tiny:
    a wave has one row at most, so every row passes through the single-row tail."""
    import simplex
    from golden_util import table_hash
    sweep_form(7)
    n_blk = 0
    for label, cons, func, rec in trajectory_cases():
        if len(func) not in (len(cons[0]) - 1, len(cons[0])) or len(func) < 2:
            continue   # the reference raises IndexError there (f() needs x1, x2)
        cap = trajectory_cap(rec)
        res = []
        for P in (13, 1):
            block_mode(P)
            sm = simplex.SimplexMethod([list(r) for r in cons], list(func))
            out = sm.solve(record_history=False, max_pivots=cap, chunk=7)
            last = out[-2] if sm.status == "error" else out[-1]
            res.append((sm.pivot_log, sm.status,
                        str(out[-1]) if sm.status == "error" else None, table_hash(last.table)))
            if P == 13:
                n_blk += sm._dev.block_plan() is not None
        assert res[0] == res[1], label
        exp = [(s["i"], s["j"]) for s in rec["steps"] if "i" in s and s["i"] is not None]
        assert res[0][0] == exp[:len(res[0][0])], label
        if rec["outcome"]["kind"] in ("optimum", "error"):
            assert res[0][3] == rec["steps"][-1]["hash"], label
    assert n_blk > 250


# ----------------------------------------------------------------------------------------------
# NaN, inf, extreme exponents and the fast path's edges with real pairs
def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _device_chain(T, n, m, P, blocks):
    """The blocks as one run / sync_state each on a DeviceTableau (one sweep per call, both
    buffer parities over the chain): (device, last control block)."""
    from simplex_mi355x.device import DeviceTableau
    dev = DeviceTableau(T, n, m, m)
    assert dev.block_plan()[1] == P
    ctl = None
    for c in blocks:
        assert c <= P
        dev.run(c, graph=False)
        ctl = dev.sync_state()
    return dev, ctl


PAIR_IDS = ["{}-{}x{}-s{}-P{}".format(*c) for c in sv.PAIRS]


@pytest.mark.parametrize("plan", [0, 2, 1], ids=["wplan", "wstep", "register"])
@pytest.mark.parametrize("name,n,m,seed,P", sv.PAIRS, ids=PAIR_IDS)
def test_pairs_special_values_vs_oracle(block_mode, sweep_form, small_grid, planner, name, n, m,
                                        seed, P, plan):
    """special_values.PAIRS in the pair layout, the row flags written by each planner: pivot log,
    pivot count and status exactly, the table under same_bits_or_nan.  PAIR_CONDITIONS first, at
    this device's CU count."""
    k = sv.block_k(P)
    sv.check_pair_census(name, n, m, k, sv.pair_case_census(name, n, m, seed, P, _cus()))
    sweep_form(7)
    block_mode(P)
    planner(plan, 0)
    _, Tref, st, done, log = sv.reference(name, n, m, seed, k)
    dev, ctl = _device_chain(sv.scenario(name, n, m, seed), n, m, P, sv.pair_chain(P))
    what = (name, n, m, seed, P, plan)
    assert int(ctl["npivots"]) == done == k, what
    assert np.array_equal(dev.read_log(0, done), log), what
    assert bool(ctl["term"]) == (st != 0), what
    sv.same_table_as_oracle(dev.download(), Tref, n, m, what)
    dev.close()


def _table_vs_oracle(T, n, m, P, blocks):
    """A finite table through the chained blocks against the C oracle: log and int64 bits, after
    PAIR_CONDITIONS["tables"] at this device's CU count."""
    from oracle import c_oracle
    k = sum(blocks)
    sv.check_pair_census("table", n, m, k, sv.pair_census(T, n, m, blocks, _cus()))
    Tref, st, done, log = c_oracle.run(T, n, m, m, k, threads=8)
    assert (st, done) == (0, k)
    dev, ctl = _device_chain(T, n, m, P, blocks)
    assert int(ctl["npivots"]) == done and not ctl["term"]
    assert np.array_equal(dev.read_log(0, done), log)
    got = dev.download()
    dev.close()
    assert np.array_equal(got[:n].view(np.int64), Tref[:n].view(np.int64)), \
        sv.first_difference(got[:n], Tref[:n])
    assert np.array_equal(got[n, :m].view(np.int64), Tref[n, :m].view(np.int64))


@pytest.mark.parametrize("P", [13, 20, 24])
@pytest.mark.parametrize("n,m", [(1023, 1023), (1000, 1100)])
def test_pairs_fast_path_edges_vs_oracle(block_mode, sweep_form, small_grid, n, m, P):
    """test_gpu_block.py's fast-path edge table with pairs (1023^2: four pairs per wave;
    1000 x 1100: odd tails and a ragged ninth chunk), 4 P + 3 pivots in five blocks."""
    sweep_form(7)
    block_mode(P)
    _table_vs_oracle(sv.fast_path_edge_table(n, m), n, m, P, sv.edge_chain(P))


@pytest.mark.parametrize("P", [20, 24])
@pytest.mark.parametrize("n,m", sorted(sv.MIXED_PAIR_SEEDS))
def test_mixed_pairs_past_one_phase_vs_oracle(block_mode, sweep_form, small_grid, n, m, P):
    """mixed_pair_table with a second pair phase of 8 and of 12 pivots (at the seeds of
    special_values.MIXED_PAIR_SEEDS, where the run holds fast and mixed pairs as well as its
    all-fallback blocks)."""
    sweep_form(7)
    block_mode(P)
    T = sv.mixed_pair_table(n, m, sv.MIXED_PAIR_SEEDS[n, m])
    _table_vs_oracle(T, n, m, P, sv.pair_chain(P))


def test_forms_agree_on_special_values(block_mode, sweep_form, small_grid):
    """sprinkle (700 x 900, seed 6) at 24 pivots per sweep under forms 5, 6 and 7: equal pivot
    logs, tables equal under same_bits_or_nan, form 5's equal to the oracle's."""
    name, n, m, seed, P = "sprinkle", 700, 900, 6, 24
    k = sv.block_k(P)
    sv.check_pair_census(name, n, m, k, sv.pair_case_census(name, n, m, seed, P, _cus()))
    block_mode(P)
    _, Tref, st, done, log = sv.reference(name, n, m, seed, k)
    out = {}
    for form in (5, 6, 7):
        sweep_form(form)
        dev, ctl = _device_chain(sv.scenario(name, n, m, seed), n, m, P, sv.pair_chain(P))
        out[form] = (int(ctl["npivots"]), dev.read_log(0, done).copy(), dev.download())
        dev.close()
    assert out[5][0] == done == k
    assert np.array_equal(out[5][1], log)
    sv.same_table_as_oracle(out[5][2], Tref, n, m, name)
    for form in (6, 7):
        assert out[form][0] == out[5][0], form
        assert np.array_equal(out[form][1], out[5][1]), form
        assert sv.same_bits_or_nan(out[form][2], out[5][2]), \
            (form, sv.first_difference(out[form][2], out[5][2]))


@pytest.mark.parametrize("light", [False, True])
def test_sharded_mixed_pairs_vs_oracle(sweep_form, small_grid, light):
    """mixed_pair_table(2000, 1023) on 2 simulated ranks in the pair layout: 1000 rows and the
    f-row each, 7 to 8 rows per wave; 13 pivots per sweep as blocks of 13, 12 and 4.  Every rank's
    log and the assembled table against the unsharded oracle."""
    from oracle import c_oracle
    from test_gpu_block_sharded import _backends, _lockstep, _result
    n, m, P, world = 2000, 1023, 13, 2
    k = sv.block_k(P)
    T = mixed_pair_table(n, m)
    Tref, st, done, log = c_oracle.run(T, n, m, m, k, threads=8)
    assert (st, done) == (0, k)
    sweep_form(7)
    bes = _backends(T, n, m, world, P)
    for c in sv.pair_chain(P):
        _lockstep(bes, c, P, light)
    states, logs, tables, full = _result(bes)
    for s, lg in zip(states, logs):
        assert s["npivots"] == done and not s["term"]
        assert np.array_equal(lg, log)
    for t in tables[1:]:   # every f-row replica identical
        assert np.array_equal(t[-1, :m].view(np.int64), tables[0][-1, :m].view(np.int64))
    assert np.array_equal(full[:n].view(np.int64), Tref[:n].view(np.int64)), \
        sv.first_difference(full[:n], Tref[:n])
    assert np.array_equal(full[n, :m].view(np.int64), Tref[n, :m].view(np.int64))
