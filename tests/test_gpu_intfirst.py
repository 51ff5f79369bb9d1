"""The int first-pivot zero fix past 256 columns and 4096 rows, on the device (``-m gpu``):
k_int_first_fix through the C ABI (smx_int_first_fix) at the shapes, pitches and forms of
intfirst_util.py, where its column stride (C > 256), its row stride (rows > 4096), a padded
`ld` and `ldm`, a mask index past 255 and the rank that does not hold the pivot row all run; then
the engine paths that reach it (eager, lazy history replay, the three chained loops, row shards)
on tables whose first pivot lies past one wave.  Everything compares with oracle/restated.py on
the caller's Python ints, bit for bit, signed zeros included; test_intfirst.py holds the census
that keeps these comparisons from being vacuous.
"""
from __future__ import annotations

import math

import numpy as np
import pytest

import intfirst_util as iu
import solution_util as su
from late_index import owner_of

pytestmark = pytest.mark.gpu

GUARD = 64
POISON = 7.0
IDS = [iu.case_id(c) for c in iu.CASES]
INVALID = 1                                         # hipErrorInvalidValue


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def _guarded(torch, count, dtype, poison):
    """A device buffer of `count` elements between two poisoned guard bands -> (whole, view)."""
    whole = torch.full((count + 2 * GUARD,), poison, dtype=dtype, device="cuda")
    return whole, whole[GUARD:GUARD + count]


def _enqueue(torch, a):
    """smx_int_first_fix on the arrays of intfirst_util.arguments(), on torch's current stream,
    without a synchronisation.  T1 and its padding stand between guard bands.  -> what _finish
    needs."""
    from simplex_mi355x import _lib
    rows, ld, ldm, r = a["rows"], a["ld"], a["ldm"], a["r_local"]
    T0 = torch.from_numpy(a["T0"]).cuda()
    whole, T1 = _guarded(torch, rows * ld, torch.float64, POISON)
    T1.copy_(torch.from_numpy(a["T1"].reshape(-1)))
    mask = None if a["mask"] is None else torch.from_numpy(a["mask"]).cuda()
    prow = None if a["prow"] is None else torch.from_numpy(a["prow"]).cuda()
    maskr = None if a["maskr"] is None else torch.from_numpy(a["maskr"]).cuda()
    p_prow = T0.data_ptr() + r * ld * 8 if prow is None else prow.data_ptr()
    p_maskr = None if mask is None else (mask.data_ptr() + r * ldm if maskr is None
                                         else maskr.data_ptr())
    err = _lib.load().smx_int_first_fix(
        T0.data_ptr(), T1.data_ptr(), ld, rows, a["C"], r, a["c"], p_prow,
        None if mask is None else mask.data_ptr(), ldm, p_maskr,
        torch.cuda.current_stream().cuda_stream)
    return err, T0, whole, T1, (mask, prow, maskr)


def _finish(a, run, what):
    """After the synchronisation: the result by bits, padding and guard bands untouched, T0
    unchanged, and the device's bytes equal to the host twin's."""
    err, T0, whole, T1, _ = run
    assert err == 0, (what, err)
    h = whole.cpu().numpy()
    assert (h[:GUARD] == POISON).all() and (h[-GUARD:] == POISON).all(), (what, "guard band")
    out = h[GUARD:-GUARD].reshape(a["rows"], a["ld"])
    iu.check_result(a, out, what)
    assert np.array_equal(su.bits(T0.cpu().numpy()), su.bits(a["T0"])), (what, "T0")
    rc, host = iu.host_fix(a)
    assert rc == 0 and host.tobytes() == out.tobytes(), (what, "host twin")
    return out


@pytest.mark.parametrize("variant", iu.VARIANTS)
@pytest.mark.parametrize("case", iu.CASES, ids=IDS)
def test_kernel(case, variant):
    """Every pitch and form of a case is enqueued, then one synchronisation."""
    import torch
    T0, T1, expected, mask = iu.variant_data(case, variant)
    r, c = case[3]
    C = T0.shape[1]
    pitches = iu.pitches(C) if mask is not None else [(C, C), (C + 7, C)]
    runs = []
    for ld, ldm in pitches:
        for form in iu.FORMS:
            a = iu.arguments(T0, T1, expected, mask, r, c, form, ld, ldm)
            runs.append((a, _enqueue(torch, a), (iu.case_id(case), variant, form, ld, ldm)))
    torch.cuda.synchronize()
    outs = {}
    for a, run, what in runs:
        outs[what[2:]] = _finish(a, run, what)
    if variant == "int_ones":                       # a mask of ones is the NULL form
        for ld, ldm in pitches:
            for form in iu.FORMS:
                b = iu.arguments(T0, T1, expected, None, r, c, form, ld, ldm)
                assert iu.host_fix(b)[1].tobytes() == outs[(form, ld, ldm)].tobytes()


def test_kernel_only_zeros_and_never_the_pivot_column():
    import torch
    T0, T1, mask, r, c, expected = iu.sentinel_case()
    runs = []
    for ld, ldm in iu.pitches(T0.shape[1])[:2]:
        a = iu.arguments(T0, T1, expected, mask, r, c, "owner", ld, ldm)
        runs.append((a, _enqueue(torch, a), ("sentinel", ld, ldm)))
    torch.cuda.synchronize()
    for a, run, what in runs:
        _finish(a, run, what)


@pytest.mark.parametrize("name", iu.REFUSALS)
def test_kernel_refusals(name):
    """hipErrorInvalidValue, nothing launched: T1 (all zeros, which a fix that ran would
    rewrite) and its guard bands come back as they were."""
    import torch
    from simplex_mi355x import _lib
    rows, C, ld, ldm = 6, 9, 11, 10
    t = iu.planted(iu.table(rows - 1, C - 1, 3, "int"), 2, 3, -3)
    T0 = torch.from_numpy(iu.padded(iu.as_f64(t), ld, iu.PAD)).cuda()
    whole, T1 = _guarded(torch, rows * ld, torch.float64, POISON)
    T1.zero_()
    mask = torch.ones((rows, ldm), dtype=torch.uint8, device="cuda")
    before = whole.cpu().numpy().copy()
    args = iu.refusal_args(name, T0.data_ptr(), T1.data_ptr(), T0.data_ptr() + 2 * ld * 8,
                           mask.data_ptr())
    err = _lib.load().smx_int_first_fix(*args, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert err == INVALID, (name, err)
    assert whole.cpu().numpy().tobytes() == before.tobytes(), name


@pytest.mark.parametrize("kind", iu.KINDS)
@pytest.mark.parametrize("case", [("wide", 5, 1099, (2, 256), -3), ("tall", 9000, 3, (4096, 1), -3),
                                  ("both", 300, 260, (299, 259), -3)],
                         ids=["wide", "tall", "both"])
def test_fix_after_the_devices_own_update(case, kind):
    """T1 from the device's update kernel (DeviceTableau.forced) at the tableau's padded `ld`,
    then DeviceTableau.int_first_fix: the fix is right after the regular fp64 pivot of any
    engine, not only after the CPU's."""
    import torch
    from simplex_mi355x.device import DeviceTableau
    assert case in iu.CASES
    T0, T1, expected, mask = iu.case_data(case, kind)
    _, n, m, (r, c), _ = case
    dev = DeviceTableau(T0.copy(), n, m, m + 1, device="cuda:0", ld_extra=8)
    assert dev.ld >= dev.C + 8
    dev.forced(r, c)
    with torch.cuda.stream(dev.stream):
        raw = dev.cur().cpu().numpy()
    assert np.array_equal(su.bits(raw[:, :dev.C]), su.bits(T1)), "the device's fp64 pivot"
    dev.int_first_fix(None if kind == "int" else mask.copy(), r, c)
    with torch.cuda.stream(dev.stream):
        full = dev.cur().cpu().numpy()
    iu.same_table_bits(full[:, :dev.C], expected, (case, kind))
    # (the update kernels may write the padding, zeros of either sign; the fix must not)
    assert np.array_equal(su.bits(full[:, dev.C:]), su.bits(raw[:, dev.C:])), "padding"
    dev.close()


# ---- engine paths ------------------------------------------------------------------------------

ENGINE = list(iu.ENGINE_CASES)


@pytest.mark.parametrize("name", ENGINE)
def test_engine_get_solution_eager(name):
    import simplex
    cons, func = iu.engine_input(name)
    sm = simplex.SimplexMethod(cons, func, device="cuda:0")
    assert sm.backend == "hip"
    iu.check_solution(sm.get_solution(max_pivots=iu.ENGINE_PIVOTS, lazy=False), name, simplex)


@pytest.mark.parametrize("name", ENGINE)
def test_engine_get_solution_lazy(name):
    """Every step's table goes through History.table: the fix runs on the replay scratch, at the
    tableau's padded ld.  Checkpoints every 3 pivots, so steps 1, 2 and 4 are replays."""
    import simplex
    cons, func = iu.engine_input(name)
    sm = simplex.SimplexMethod(cons, func, device="cuda:0")
    assert sm._dev.ld > sm._dev.C
    got = sm.get_solution(max_pivots=iu.ENGINE_PIVOTS, lazy=True, chunk=3)
    hist = got[0]._history
    assert sorted(hist.ckpt) == [s for s in range(0, sm.pivots + 1, 3)], sorted(hist.ckpt)
    iu.check_solution(got, name, simplex)


@pytest.mark.parametrize("path", ["launch", "resident", "block"])
@pytest.mark.parametrize("name", ENGINE)
def test_engine_chained_solve_paths(name, path):
    """Every shape here admits all three paths (asserted)."""
    import simplex
    from simplex_mi355x import _lib
    cons, func = iu.engine_input(name)
    prev_r = _lib.tune_resident(0 if path == "resident" else -1)
    prev_b = _lib.tune_block(4 if path == "block" else 1)
    try:
        sm = simplex.SimplexMethod(cons, func, device="cuda:0")
        assert (sm._dev.block_plan() is not None) == (path == "block")
        assert (sm._dev.resident_plan() is not None) == (path == "resident")
        out = sm.solve(record_history=False, max_pivots=iu.ENGINE_PIVOTS, chunk=3)
        iu.check_final(sm, out, name, simplex)
    finally:
        _lib.tune_resident(prev_r)
        _lib.tune_block(prev_b)


# (case, world) -> the rank that holds the first pivot's row (row_range: n // world rows each).
# late_row: the last rank, so every other rank takes the r_local = -1 form; the others: the first
# rank or an inner one, but for tall_int on two ranks (the ratio test of these tall tables picks
# a late row).
OWNERS = {("wide_int", 2): 0, ("wide_int", 4): 1, ("wide_mixed", 2): 0, ("wide_mixed", 4): 1,
          ("tall_int", 2): 1, ("tall_int", 4): 2, ("tall_mixed", 2): 0, ("tall_mixed", 4): 1,
          ("late_row", 2): 1, ("late_row", 4): 3}


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("name", ["wide_int", "wide_mixed", "tall_int", "tall_mixed", "late_row"])
def test_engine_row_sharded(name, world):
    """Row blocks on `world` ranks of one device: eager get_solution and chained solve."""
    import simplex
    r = iu.engine_reference(name)[1][0]
    cons, func = iu.engine_input(name)
    sm = simplex.SimplexMethod(cons, func, devices=["cuda:0"] * world)
    assert sm.backend == "sharded"
    assert sm._dev._owner(r)[0] == owner_of(r, len(cons), world) == OWNERS[name, world]
    last = name == "late_row" or (name, world) == ("tall_int", 2)
    assert (OWNERS[name, world] == world - 1) == last
    iu.check_solution(sm.get_solution(max_pivots=iu.ENGINE_PIVOTS, lazy=False), name, simplex)
    cons, func = iu.engine_input(name)
    sm2 = simplex.SimplexMethod(cons, func, devices=["cuda:0"] * world)
    out = sm2.solve(record_history=False, max_pivots=iu.ENGINE_PIVOTS, chunk=3)
    iu.check_final(sm2, out, name, simplex)


@pytest.mark.parametrize("leg", ["eager", "lazy", "chained"])
def test_engine_x1_is_the_fixed_zero(leg):
    """x1_zero: x1 after the first pivot is -0 / e of an int 0, -0.0 in the reference's ints and
    +0.0 in fp64, so the step's x1 must come from the fixed table.  On the lazy leg the engine
    takes each step's (x1, x2) from the device's x-ring, whose slot of pivot 0 was written
    before the fix: that step is read from the table again (asserted here by its sign)."""
    import simplex
    snaps = iu.engine_reference("x1_zero")[0]
    want = snaps[1]
    assert want["x1"] == 0 and math.copysign(1.0, want["x1"]) == -1.0
    cons, func = iu.engine_input("x1_zero")
    sm = simplex.SimplexMethod(cons, func, device="cuda:0")
    if leg == "chained":
        out = sm.solve(record_history=False, max_pivots=1, chunk=3)
        step = out[1]
    else:
        got = sm.get_solution(max_pivots=1, lazy=(leg == "lazy"), chunk=3)
        step = got[1]
    assert sm.pivot_log == [(snaps[0]["i"], snaps[0]["j"])]
    for key in ("x1", "x2", "optimum"):
        assert iu.same_number(getattr(step, key), want[key]), (leg, key, getattr(step, key))
    assert step.x1 == 0 and math.copysign(1.0, step.x1) == -1.0
    iu.same_table_bits(step.table, want["table"], leg)
