"""GPU parity of the row-pair sweep layout (smx_tune_block_form(7), blk_sweep_body_flag<P, 7> in
csrc/smx_sweep.hpp): a lane keeps two rows of its two columns, so each LDS read of a pivot's row
slice and of (e, y) feeds four chains, and the rows' multipliers arrive in phases of 12 pivots.

Bit-exact against the C oracle with pairs, odd tails and mixed pairs (rows of one pair on
different paths), against the one-row LDS layout (form 5) at 16 rows per wave, and over the
trajectory fixtures (tiny tables: the single-row tail only).

Small tables give a wave fewer than two rows under the default grid of 8 workgroups per CU, so the
oracle cases run the sweep with one workgroup per CU (smx_tune_set(-2, 1)): at n = 1000 rows and
8 or 9 column chunks a wave then owns 7-9 rows.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

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


def _chunks(P):
    """2 P + 3 pivots in three chains of one block each: P (two phases past 12), P - 1 (the other
    parity: one of the two is in place, the other out of place) and a ragged last block of 4."""
    return [P, P - 1, 4]


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
    """A uniform table whose adjacent rows of a wave fall on different sweep paths: every third
    constraint row scaled past 2^101 (inputs and multipliers out of the fast path's bounds),
    exact zeros in every fifth column of every seventh row and negative zeros in every fifth
    column of every eleventh (zero multipliers wherever such a column is a pivot's: flag-3 rows)."""
    from simplex_mi355x import lp
    T = lp.dense_tableau("uniform", SEED, n, m)
    T[0:n:3] *= 2.0 ** 102
    T[1:n:7, 0:m:5] = 0.0
    T[2:n:11, 0:m:5] = -0.0
    return T


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
