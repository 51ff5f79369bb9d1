"""GPU: first-index selections whose winner sits past the first wave, workgroup, strided pass,
sweep chunk and rank, through every pivot path (launch chain, resident loop, block pivots with
each planner and sweep form, the three batch kernels, one-pivot and block shards on simulated
ranks) against the C oracle: pivot log, pivot count, status and the table by bits.

The seeded tables the rest of the suite runs never put the first "-b" < 0, the first positive
entry of that row or the first f[j] < 0 past index 32 (the testing section), so the
merges of those searches across lanes, waves, loop passes, workgroups, chunks and ranks only ever
saw a winner at the front.  The tables of late_index.py move the winners: embedded live blocks
(every pivot inside rows and columns >= 1026 of an 1100 x 1300 table, in both phases), steep
f-rows (every entering column in the last columns of a dense table) and planted single decisions
at rows and columns 0, 62, 63, 64, 255, 256, 1023, 1024 and the last one, the class-0 tie with
its two rows in different lanes, waves, workgroups and ranks and in one lane of a 1024-stride
loop (r2 = r1 + 1024).  test_late_index_oracle.py checks on the CPU that every chain used here
keeps its pivots where they are meant to be.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import late_index as li
import solution_util as su
import special_values as sv
from batch_util import solve as _solve

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


@pytest.fixture
def knobs():
    """Set smx_tune_resident / smx_tune_block for one test; both policies restored afterwards."""
    from simplex_mi355x import _lib
    prev_b = _lib.tune_block(-1)
    prev_r = _lib.tune_resident(-2)

    def set_(resident, block=None):
        _lib.tune_resident(resident)
        if block is not None:
            _lib.tune_block(block)
    yield set_
    _lib.tune_block(prev_b)
    _lib.tune_resident(prev_r)


@pytest.fixture
def planner():
    """Set smx_tune_block_planner (planner, window slots) for one test."""
    from simplex_mi355x import _lib
    prev = _lib.tune_block_planner(-1, -1)
    yield _lib.tune_block_planner
    _lib.tune_block_planner(prev, 0)


@pytest.fixture
def sweep_form():
    from simplex_mi355x import _lib
    prev = _lib.tune_block_form(-1)
    yield _lib.tune_block_form
    _lib.tune_block_form(prev)


@pytest.fixture
def grid():
    """smx_tune_set(-2, workgroups per CU) for the block sweep; the previous override afterwards.
    One workgroup per CU gives a wave several rows, so forms 7 and 8 sweep real pairs and quads."""
    from simplex_mi355x import _lib
    lib = _lib.load()
    prev = ctypes.c_int32(0)
    _lib.check(lib.smx_tune_get(None, ctypes.byref(prev), None, None, None, None), "smx_tune_get")
    yield lambda bpc: _lib.check(lib.smx_tune_set(-2, bpc), "smx_tune_set")
    _lib.check(lib.smx_tune_set(-2, prev.value), "smx_tune_set")


@pytest.fixture
def fused_knob():
    from simplex_mi355x import _lib
    prev = _lib.load().smx_tune_fused(-1)
    yield _lib.load().smx_tune_fused
    _lib.load().smx_tune_fused(prev)


def _device(T, n, m, flen):
    from simplex_mi355x.device import DeviceTableau
    return DeviceTableau(np.array(T), n, m, flen)


def _run_chain(name, graph=True, check=None):
    n, m = li.dims(name)
    ref = li.reference(name)
    dev = _device(ref[0], n, m, m)
    if check is not None:
        check(dev)
    dev.run(li.CASES[name][2], graph=graph)
    li.same_as_oracle(dev, ref, n, m, name)
    dev.close()
    return dev


# ----------------------------------------------------------------------------------------------
# the launch chain: k_reset, k_select / k_finalize / update, the fused look-ahead
FORMS = [(g, f) for g in (True, False) for f in (1, 0)]
FORM_IDS = ["{}-{}".format("graph" if g else "eager", "fused" if f else "unfused")
            for g, f in FORMS]


def _no_plans(dev):
    assert dev.resident_plan() is None and dev.block_plan() is None


def _resident(dev):
    assert dev.resident_plan() is not None


@pytest.mark.parametrize("graph,fused", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("name", ["chain_u", "chain_m", "chain_steep"])
def test_launch_chain_vs_oracle(knobs, fused_knob, name, graph, fused):
    """Every pivot at rows and columns >= 1026 (embedded), every entering column >= 1100
    (steep): the fifth 256-row select workgroup, the second pass of the 1024-stride scans, the
    update kernels' atomicMin into the next step's first-negative slots from their last waves."""
    knobs(-1, 1)
    fused_knob(fused)
    _run_chain(name, graph, _no_plans)


@pytest.mark.parametrize("kind", li.KINDS)
def test_launch_chain_planted_decisions(knobs, fused_knob, kind):
    """Every planted table of the kind at 1100 x 1300: the pick alone (k_select + k_finalize), then
    one pick and at most one pivot in all four forms of the chain (one tableau object per form,
    the tables uploaded in turn)."""
    n, m = 1100, 1300
    knobs(-1, 1)
    cases = [c for c in li.planted_cases(n, m) if c[0] == kind]
    assert cases
    devs = {}
    for _, at in cases:
        ref = li.planted_reference(kind, n, m, at)
        want, flen = ref[6], ref[1]
        assert (ref[3], ref[4]) == (want[0], int(want[0] == 0))
        if want[0] == 0:
            assert tuple(ref[5][0]) == want[1:]
        for graph, fused in [("pick", 0)] + FORMS:
            fused_knob(fused)
            dev = devs.get((graph, fused, flen))
            if dev is None:
                dev = devs[graph, fused, flen] = _device(ref[0], n, m, flen)
                _no_plans(dev)
            else:
                dev.upload(ref[0])
            if graph == "pick":
                st, r, c = dev.pick()[:3]
                assert st == want[0], (kind, at, st)
                assert (r == want[1] or want[1] < 0) and (c == want[2] or want[2] < 0), \
                    (kind, at, r, c)
                continue
            dev.run(1, graph=graph)
            li.same_as_oracle(dev, ref, n, m, (kind, at, graph, fused))
    for dev in devs.values():
        dev.close()


# ----------------------------------------------------------------------------------------------
# the resident loop
@pytest.mark.parametrize("name", ["chain_u", "chain_m", "chain_steep"])
def test_resident_vs_oracle(knobs, name):
    """The automatic grid: 5 or 6 rows per workgroup, the live rows in the last workgroups."""
    knobs(0)
    dev = _run_chain(name, check=_resident)
    assert dev.resident_fallbacks == 0


@pytest.mark.parametrize("ovl", [0, 1], ids=["round3", "overlapped"])
@pytest.mark.parametrize("name", ["chain_m", "chain_steep"])
def test_resident_overlap_settings(knobs, name, ovl):
    """Both forms of the resident loop (smx_tune_resident_overlap): the ballots and the per-wave
    LDS atomicMin for the next step's first negatives with the winners in the last workgroups."""
    from simplex_mi355x import _lib
    knobs(0)
    prev = _lib.tune_resident_overlap(-1)
    try:
        _lib.tune_resident_overlap(ovl)
        dev = _run_chain(name, check=_resident)
    finally:
        _lib.tune_resident_overlap(prev)
    assert dev.resident_fallbacks == 0


@pytest.mark.parametrize("wg", [1, 7, 256])
@pytest.mark.parametrize("name", ["res_m", "res_steep"])
def test_resident_workgroup_counts(knobs, name, wg):
    """100 x 120: one workgroup holds the whole table, 7 hold 15 rows each (the live rows 60 to
    99 in the last three), 100 one row each."""
    n, m = li.dims(name)
    knobs(wg)

    def check(dev):
        G, rpw = dev.resident_plan()[1][:2]
        assert G <= wg and G * rpw >= n > (G - 1) * rpw
    dev = _run_chain(name, check=check)
    assert dev.resident_fallbacks == 0


@pytest.mark.parametrize("n,m,wg", [(1100, 1300, 0), (100, 120, 1), (100, 120, 7),
                                     (100, 120, 256)])
@pytest.mark.parametrize("kind", ["phase1", "tie"])
def test_resident_planted_decisions(knobs, kind, n, m, wg):
    knobs(wg)
    dev = None
    for _, at in [c for c in li.planted_cases(n, m) if c[0] == kind]:
        ref = li.planted_reference(kind, n, m, at)
        if dev is None:
            dev = _device(ref[0], n, m, m)
            _resident(dev)
        else:
            dev.upload(ref[0])
        dev.run(1)
        li.same_as_oracle(dev, ref, n, m, (kind, at, wg))
        assert dev.resident_fallbacks == 0
    dev.close()


# ----------------------------------------------------------------------------------------------
# block pivots
# (pivots per sweep, sweep form, sweep workgroups per CU or 0 for the default grid): every P and
# every form, forms 7 and 8 with real pairs and quads
SWEEPS = [(8, 0, 0), (20, 5, 0), (24, 7, 1), (8, 8, 1), (20, 8, 1)]
# smx_tune_block_planner's settings, and "shard1": the same table, pivots per sweep, sweep form
# and grid as ONE rank of the row-sharded block chain, the planner every sharded chain runs (the
# sharded cases below keep a rank within one planner workgroup; here its row pass has winners in
# late lanes, waves and workgroups)
PLANS = [0, 2, 1, "shard1"]
PLAN_IDS = ["wplan", "wstep", "register", "shard1"]


def _run_shard1(ref, n, m, k, P, what):
    from test_gpu_block_sharded import _one_rank_vs_oracle
    assert ref[1] == m
    _one_rank_vs_oracle(ref[0], n, m, k, P, ref[2:6], what)


def _run_block(knobs, planner, sweep_form, grid, name, plan, P, form, bpc):
    knobs(-1, P)
    sweep_form(form)
    if bpc:
        grid(bpc)
    n, m = li.dims(name)
    ref = li.reference(name, sv.block_k(P))
    if plan == "shard1":
        _run_shard1(ref, n, m, sv.block_k(P), P, (name, plan, P, form))
        return ref
    planner(plan, 0)
    dev = _device(ref[0], n, m, m)
    assert dev.block_plan()[1] == P
    dev.run(sv.block_k(P))
    li.same_as_oracle(dev, ref, n, m, (name, plan, P, form))
    dev.close()
    return ref


@pytest.mark.parametrize("P,form,bpc", SWEEPS, ids=["P{}-form{}-bpc{}".format(*s) for s in SWEEPS])
@pytest.mark.parametrize("plan", PLANS, ids=PLAN_IDS)
@pytest.mark.parametrize("name", ["blk_m", "blk_u", "blk_steep"])
def test_block_vs_oracle(knobs, planner, sweep_form, grid, name, plan, P, form, bpc):
    """1025 x 1300, a 128 x 128 live block as the tail of the table (rows 897 on, columns 1172
    on), two whole blocks and a ragged one of 3 at the default window: the planners' first-index
    reductions and ballots with every winner in the last waves and the last sweep chunks."""
    _run_block(knobs, planner, sweep_form, grid, name, plan, P, form, bpc)


@pytest.mark.parametrize("nwin", [2, 17])
@pytest.mark.parametrize("plan", [0, 2], ids=["wplan", "wstep"])
@pytest.mark.parametrize("name", ["blk_m", "blk_u"])
def test_block_small_window_vs_oracle(knobs, planner, name, plan, nwin):
    """The window planner with a window of a few columns: the out-of-window fallbacks for
    entering, phase-1 and pivot columns at 1172 and past it."""
    n, m = li.dims(name)
    P = 8
    knobs(-1, P)
    planner(plan, nwin)
    ref = li.reference(name, sv.block_k(P))
    dev = _device(ref[0], n, m, m)
    assert dev.block_plan()[1] == P
    dev.run(sv.block_k(P))
    li.same_as_oracle(dev, ref, n, m, (name, plan, nwin))
    dev.close()


@pytest.mark.parametrize("P,form,bpc", [(24, 7, 1), (20, 8, 1), (8, 5, 0)])
@pytest.mark.parametrize("plan", PLANS, ids=PLAN_IDS)
def test_block_live_rows_from_an_odd_row(knobs, planner, sweep_form, grid, plan, P, form, bpc):
    """The live block from row 895 (odd, 895 % 4 == 3): its first row closes a row pair and a
    row quad of the table, the rest starts new ones."""
    _run_block(knobs, planner, sweep_form, grid, "blk_m_odd", plan, P, form, bpc)


@pytest.mark.parametrize("P,form,bpc", [(8, 0, 0), (20, 5, 0), (24, 8, 1)])
@pytest.mark.parametrize("plan", PLANS, ids=PLAN_IDS)
def test_block_chain_ends_inside_a_block(knobs, planner, sweep_form, grid, plan, P, form, bpc):
    """A 9 x 9 live block in rows 1015 on: NOT_CONVERGE after 12 pivots -- inside the second
    block of 8, inside the first of 20 and of 24 -- published from the last rows' waves."""
    ref = _run_block(knobs, planner, sweep_form, grid, "blk_end", plan, P, form, bpc)
    assert (ref[3], ref[4]) == (li.NOT_CONVERGE, 12)


@pytest.mark.parametrize("P,form,bpc", [(8, 0, 0), (24, 7, 1), (8, 8, 1)])
@pytest.mark.parametrize("plan", PLANS, ids=PLAN_IDS)
@pytest.mark.parametrize("kind", ["phase1", "tie"])
def test_block_planted_decisions(knobs, planner, sweep_form, grid, kind, plan, P, form, bpc):
    """One block of P pivots from every planted phase-1 and tie table at 1025 x 1300: the block's
    first decision is the planted one (the tie's rows in two lanes, waves and workgroups and at
    rows 0 and 1024), the rest whatever the oracle makes of the table."""
    from oracle import c_oracle
    n, m = 1025, 1300
    knobs(-1, P)
    sweep_form(form)
    if bpc:
        grid(bpc)
    if plan != "shard1":
        planner(plan, 0)
    dev = None
    for _, at in [c for c in li.planted_cases(n, m) if c[0] == kind]:
        T, flen, want = li.planted(kind, n, m, at)
        Tref, st, done, log = c_oracle.run(T, n, m, flen, P, threads=8)
        assert done >= 1 and tuple(log[0]) == want[1:], (kind, at)
        if plan == "shard1":
            _run_shard1((T, flen, Tref, st, done, log), n, m, P, P, (kind, at, plan, P, form))
            continue
        if dev is None:
            dev = _device(T, n, m, flen)
            assert dev.block_plan()[1] == P
        else:
            dev.upload(T)
        dev.run(P)
        li.same_as_oracle(dev, (T, flen, Tref, st, done, log), n, m, (kind, at, plan, P, form))
    if dev is not None:
        dev.close()


# ----------------------------------------------------------------------------------------------
# the batch kernels
def _planted_members(n, m, cap):
    """[(n, m, reference at the launch's cap)] of every planted table of the shape: the first
    pick is the planted one, the pivots after it whatever the oracle makes of the table."""
    from oracle import c_oracle
    out = []
    for kind, at in li.planted_cases(n, m):
        T, flen, want = li.planted(kind, n, m, at)
        Tref, st, done, log = c_oracle.run(T, n, m, flen, cap)
        if want[0] == 0:
            assert tuple(log[0]) == want[1:], (kind, at)
        else:
            assert (st, done) == (want[0], 0), (kind, at)
        out.append((n, m, (T, flen, Tref, st, done, log)))
    return out


def _batch(names, kernel, planted_shapes=(), **kw):
    """The chains `names` (one cap) and every planted table of `planted_shapes` in one launch
    (padded to the largest member) with solution=True: tables, logs and statuses by bits, and x,
    the duals, the objective and the labels through solution_util."""
    cap = li.CASES[names[0]][2]
    members = []
    for name in names:
        assert li.CASES[name][2] == cap
        members.append((*li.dims(name), li.reference(name)))
    for shape in planted_shapes:
        members += _planted_members(*shape, cap)
    out = _solve([(ref[0], n, m, ref[1]) for n, m, ref in members], cap, kernel=kernel,
                 solution=True, **kw)
    for q, (n, m, ref) in enumerate(members):
        li.batch_member_same_as_oracle(out, q, n, m, ref, (kernel, q))
        exp = su.expected(ref[2], ref[5], n, m, ref[0][n])
        su.same_arrays(out, q, n, m, exp, (kernel, q), nan_aware=True)
    return members


def test_batch_wave_vs_oracle():
    """k_batch at 63 x 63, the live block in lanes 40 to 62, with the planted tables of the shape
    (rows 0, 61, 62) in the same launch."""
    members = _batch(["wave_m", "wave_u"], "wave", [(63, 63)])
    assert len(members) > 20


def test_batch_workgroup_vs_oracle():
    """k_batch_wg at 130 x 130: candidates and winners in the second and third wave; the planted
    tables of 130 x 130 and, inside the launch's padding, of 100 x 120."""
    from simplex_mi355x.batch import wg_lds_bytes
    assert wg_lds_bytes(131, 131) >= 0
    _batch(["wg_m", "wg_u", "wg_steep"], "workgroup", [(130, 130), (100, 120)])


def test_batch_global_vs_oracle():
    """k_batch_gm at 200 x 200, past the LDS edge."""
    from simplex_mi355x.batch import wg_lds_bytes
    assert wg_lds_bytes(201, 201) == -1
    _batch(["gm_m", "gm_u", "gm_steep"], "global", [(200, 200)])


def test_batch_global_wide_vs_oracle():
    """k_batch_gm at 130 x 1100, the live columns from 1030 on, past one pass of 1024 threads,
    with the planted tables of the shape (columns 1023, 1024 and 1099 among them)."""
    from simplex_mi355x.batch import gm_fits
    assert gm_fits(131, 1101)
    _batch(["gm_wide_m", "gm_wide_u"], "global", [(130, 1100)])


# ----------------------------------------------------------------------------------------------
# simulated ranks
SHARD_KINDS = ("phase1", "incorrect", "fneg", "notconv", "tie", "zero_neg", "nan_first")


def _shards_same_as_oracle(states, logs, tables, full, ref, n, m, what):
    Tref, st, done, log = ref[2:6]
    for s, lg in zip(states, logs):
        assert s["npivots"] == done, (what, s)
        assert np.array_equal(lg, log), (what, lg.tolist(), log.tolist())
        assert bool(s["term"]) == (st != 0), (what, s)
        if st != 0:
            assert s["status"] == st, (what, s)
    for t in tables[1:]:   # every f-row replica identical
        assert sv.same_bits_or_nan(t[-1, :m], tables[0][-1, :m]), what
    sv.same_table_as_oracle(full, Tref, n, m, what)


def _modes():
    from test_gpu_sharded import MODES
    return list(MODES)


@pytest.mark.parametrize("mode", ["fused", "unfused"])
@pytest.mark.parametrize("name", sorted(li.SHARDED))
def test_hip_shards_vs_oracle(name, mode):
    """The one-pivot shard chain: the live rows owned by the last rank (gnegb / owner_b of the
    merged decision never rank 0's) and straddling two ranks (the owner changes along the
    chain)."""
    from test_gpu_sharded import _simulate
    assert mode in _modes() and len(_modes()) == 2
    args, world, k, _ = li.SHARDED[name]
    n, m = args[1:3]
    ref = li.reference(name)
    states, logs, tables, full, _ = _simulate(np.array(ref[0]), n, m, k, world, mode)
    _shards_same_as_oracle(states, logs, tables, full, ref, n, m, (name, mode))


@pytest.mark.parametrize("mode", ["fused", "unfused"])
@pytest.mark.parametrize("world", [2, 4])
def test_hip_shards_planted_decisions(world, mode):
    """The planted tables at 300 x 260 on ranks of 150 and of 75 rows: the tie with r1 and r2 on
    different ranks, INCORRECT and the lone negative "-b" at rows of every rank."""
    from test_gpu_sharded import _simulate
    n, m = 300, 260
    cases = [c for c in li.planted_cases(n, m) if c[0] in SHARD_KINDS]
    assert any(li.owner_of(at[0], n, world) != li.owner_of(at[1], n, world)
               for kind, at in cases if kind == "tie")
    assert any(li.owner_of(at[0], n, world) != 0 for kind, at in cases if kind == "incorrect")
    for kind, at in cases:
        ref = li.planted_reference(kind, n, m, at)
        states, logs, tables, full, _ = _simulate(ref[0], n, m, 1, world, mode)
        _shards_same_as_oracle(states, logs, tables, full, ref, n, m, (kind, at, world, mode))


@pytest.mark.parametrize("light", [False, True], ids=["full", "light"])
@pytest.mark.parametrize("name", sorted(li.SHARDED))
def test_block_shards_vs_oracle(name, light):
    """Block pivots on row shards, 5 per sweep, both exchanges."""
    from test_gpu_block_sharded import _backends, _lockstep, _result
    args, world, k, _ = li.SHARDED[name]
    n, m = args[1:3]
    P = 5
    ref = li.reference(name)
    bes = _backends(np.array(ref[0]), n, m, world, P)
    _lockstep(bes, k, P, light)
    _shards_same_as_oracle(*_result(bes), ref, n, m, (name, light))


@pytest.mark.parametrize("light", [False, True], ids=["full", "light"])
@pytest.mark.parametrize("world", [2, 4])
def test_block_shards_planted_decisions(world, light):
    """The planted tie (r1 and r2 on different ranks among the pairs) and INCORRECT at every row
    position as the first decision of a block of 3."""
    from test_gpu_block_sharded import _backends, _lockstep, _result
    n, m = 300, 260
    for kind, at in [c for c in li.planted_cases(n, m) if c[0] in ("tie", "incorrect")]:
        ref = li.planted_reference(kind, n, m, at)
        bes = _backends(np.array(ref[0]), n, m, world, 3)
        _lockstep(bes, 1, 3, light)
        _shards_same_as_oracle(*_result(bes), ref, n, m, (kind, at, world, light))
