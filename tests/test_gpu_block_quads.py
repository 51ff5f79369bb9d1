"""GPU parity of the row-quad sweep layout (smx_tune_block_form(8), blk_sweep_body_flag<P, 8> in
csrc/smx_sweep.hpp): a lane keeps four rows of its two columns, so each LDS read of a pivot's row
slice feeds eight chains; the four rows' multipliers and the pivots' (e, y) arrive as scalar
operands in phases of 6 pivots.  Form 8 exists from 13 pivots per sweep on: a shorter block (the
ragged block of 4 of every chain here, the block of 12 after one of 13) runs form 5's kernel.

Every test is bit-exact against the C oracle, with form 8 forced and one sweep workgroup per CU
(smx_tune_set(-2, 1)), so that a wave owns 5-9 rows: at 256 CUs a quad and a tail of 1-2 at
700 x 900, a quad and a tail of 3 at 895 x 900, exactly two quads at 1023^2, two quads and a tail
of 1 at 1000 x 1100 (9 chunks, stride 112).  What exists only in the quad layout -- the one vote
over a quad's eight inputs, the tail of 1-3 rows, every later phase's reload of four rows'
multipliers and of (e, y), the row-by-row fallback run from inside the quad loop's prefetch
rotation -- sees NaN, inf, denormals and 2^+-150 values, the fast path's edges and mixed quads.

Which path each quad takes is counted on the CPU by quad_util.quad_census, and every test first
checks QUAD_CONDITIONS at the device's own CU count, so a geometry that moved fails by name.  The
counts at 256 CUs are in test_quad_census.py's docstring.
"""
from __future__ import annotations

import numpy as np
import pytest

import quad_util as qu
import special_values as sv
# the pair layout's fixtures and chain driver, unchanged: smx_tune_block with the resident loop
# off, smx_tune_block_form, one sweep workgroup per CU, smx_tune_block_planner
from test_gpu_block_pairs import (_cus, _device_chain, _need_gpu, block_mode,  # noqa: F401
                                  planner, small_grid, sweep_form)

pytestmark = pytest.mark.gpu


def test_form8_is_accepted(sweep_form):
    """smx_tune_block_form takes 8 and reports it back; 9 is refused and changes nothing."""
    sweep_form(8)
    assert sweep_form(-1) == 8
    sweep_form(9)
    assert sweep_form(-1) == 8


QUAD_IDS = ["{}-{}x{}-s{}-P{}".format(*c) for c in qu.QUADS]


@pytest.mark.parametrize("plan", [0, 2, 1], ids=["wplan", "wstep", "register"])
@pytest.mark.parametrize("name,n,m,seed,P", qu.QUADS, ids=QUAD_IDS)
def test_quads_special_values_vs_oracle(block_mode, sweep_form, small_grid, planner, name, n, m,
                                        seed, P, plan):
    """quad_util.QUADS in the quad layout, the row flags written by each planner, as chains of P,
    P - 1 and a ragged block of 4 (in place and out of place): pivot log, pivot count and status
    exactly, the table under same_bits_or_nan.  QUAD_CONDITIONS first, at this device's CU count."""
    k = sv.block_k(P)
    qu.check_quad_census(name, n, m, k, P, qu.quad_case_census(name, n, m, seed, P, _cus()))
    sweep_form(8)
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


def _table_vs_oracle(kind, T, n, m, P, blocks):
    """A finite table through the chained blocks against the C oracle: log and int64 bits, after
    QUAD_CONDITIONS[kind] at this device's CU count."""
    from oracle import c_oracle
    k = sum(blocks)
    qu.check_quad_census(kind, n, m, k, P, qu.quad_census(T, n, m, blocks, _cus()))
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
def test_quads_fast_path_edges_vs_oracle(block_mode, sweep_form, small_grid, n, m, P):
    """test_gpu_block.py's fast-path edge table with quads (1023^2: two quads per wave;
    1000 x 1100: tails and a ragged ninth chunk), 4 P + 3 pivots in five blocks: the rows past
    2^101 and at 2^-60 sit in quads beside ordinary rows, the 2^-99 columns take their chunks, the
    zero and -0 blocks flag their rows."""
    sweep_form(8)
    block_mode(P)
    _table_vs_oracle("edge_table", sv.fast_path_edge_table(n, m), n, m, P, sv.edge_chain(P))


@pytest.mark.parametrize("P", [20, 24])
@pytest.mark.parametrize("n,m", sorted(sv.MIXED_PAIR_SEEDS))
def test_mixed_table_quads_vs_oracle(block_mode, sweep_form, small_grid, n, m, P):
    """mixed_pair_table at 20 and 24 pivots per sweep: no chunk of a long block is free, so every
    quad is handed row by row to the window-tracked and exact paths from inside the quad loop."""
    sweep_form(8)
    block_mode(P)
    T = sv.mixed_pair_table(n, m, sv.MIXED_PAIR_SEEDS[n, m])
    _table_vs_oracle("mixed_table", T, n, m, P, sv.pair_chain(P))


@pytest.mark.parametrize("m", [1023, 1100])
def test_forms_5_7_8_agree_on_mixed_table(block_mode, sweep_form, small_grid, m):
    """mixed_pair_table (seed 11) at 13 pivots per sweep, 2 x 13 + 3 pivots as pair_chain(13), under
    forms 5, 7 and 8: one pivot log and one table from all three, form 5's equal to the oracle's."""
    from oracle import c_oracle
    n, P = 1000, 13
    T = sv.mixed_pair_table(n, m, 11)
    blocks = sv.pair_chain(P)
    k = sum(blocks)
    qu.check_quad_census("mixed_table", n, m, k, P, qu.quad_census(T, n, m, blocks, _cus()))
    block_mode(P)
    out = {}
    for form in (5, 7, 8):
        sweep_form(form)
        dev, ctl = _device_chain(T, n, m, P, blocks)
        out[form] = (int(ctl["npivots"]), dev.read_log(0, k).copy(),
                     dev.download().view(np.int64).copy())
        dev.close()
    Tref, st, done, log = c_oracle.run(T, n, m, m, k, threads=8)
    assert (st, done) == (0, k)
    assert out[5][0] == done
    assert np.array_equal(out[5][1], log)
    assert np.array_equal(out[5][2][:n], Tref[:n].view(np.int64))
    assert np.array_equal(out[5][2][n, :m], Tref[n, :m].view(np.int64))
    for form in (7, 8):
        assert out[form][0] == out[5][0], form
        assert np.array_equal(out[form][1], out[5][1]), form
        assert np.array_equal(out[form][2], out[5][2]), form


@pytest.mark.parametrize("light", [False, True])
def test_sharded_mixed_table_quads_vs_oracle(sweep_form, small_grid, light):
    """mixed_pair_table(2000, 1023) on 2 simulated ranks in the quad layout: 1000 rows and the
    f-row each, 7 to 8 rows per wave; 13 pivots per sweep as blocks of 13, 12 and 4.  Every rank's
    log and the assembled table against the unsharded oracle."""
    from oracle import c_oracle
    from test_gpu_block_sharded import _backends, _lockstep, _result
    n, m, P, world = 2000, 1023, 13, 2
    k = sv.block_k(P)
    T = sv.mixed_pair_table(n, m, 11)
    Tref, st, done, log = c_oracle.run(T, n, m, m, k, threads=8)
    assert (st, done) == (0, k)
    sweep_form(8)
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
