"""The int first-pivot zero fix past 256 columns and 4096 rows, on the CPU: the host twin
(smx_host_int_first_fix, the same int_first_value and the same loops as k_int_first_fix without
its two strides) through the C ABI, and the host engine, against oracle/restated.py on the
caller's Python ints -- bit for bit, signed zeros included.  intfirst_util.py holds the inputs,
the restatement and the census; test_gpu_intfirst.py runs the same cases through the kernel.
test_intzero.py holds the same semantics to the reference solver's recorded tables at small sizes.
"""
from __future__ import annotations

import random
import warnings

import numpy as np
import pytest

import intfirst_util as iu
import solution_util as su

IDS = [iu.case_id(c) for c in iu.CASES]


def test_the_inputs_keep_their_case():
    """Every region a case is named for holds at least NEED zeros whose sign the fix must change
    (and T1 differs from the restatement in nothing else), so no comparison below is vacuous."""
    mixed = {}
    for case in iu.CASES:
        for kind in iu.KINDS:
            cen = iu.census(*iu.case_data(case, kind), *case[3])
            iu.check_census((iu.case_id(case), kind), cen, iu.case_need(case, kind), e=case[4])
            if kind == "mixed":
                mixed[case] = cen
    iu.check_rule_b(mixed)
    for name in iu.ENGINE_CASES:
        iu.check_engine_census(name)


def test_census_regions_are_all_named():
    """Each region of the two strides is asked of some case: the second and the later column
    passes, the second and the third row pass, the pivot row at late columns."""
    asked = {key for case in iu.CASES for kind in iu.KINDS for key in iu.case_need(case, kind)}
    assert {"prow", "prow_only", "prow_col256", "other", "col256", "col512", "row4096", "row8192",
            "rule_a", "e_neg", "e_pos"} <= asked


@pytest.mark.parametrize("variant", iu.VARIANTS)
@pytest.mark.parametrize("case", iu.CASES, ids=IDS)
def test_host_twin(case, variant):
    T0, T1, expected, mask = iu.variant_data(case, variant)
    r, c = case[3]
    C = T0.shape[1]
    pitches = iu.pitches(C) if mask is not None else [(C, C), (C + 7, C)]
    for ld, ldm in pitches:
        for form in iu.FORMS:
            what = (iu.case_id(case), variant, form, ld, ldm)
            a = iu.arguments(T0, T1, expected, mask, r, c, form, ld, ldm)
            t0_before = a["T0"].copy()
            rc, out = iu.host_fix(a)
            assert rc == 0, what
            iu.check_result(a, out, what)
            assert np.array_equal(su.bits(a["T0"]), su.bits(t0_before)), (what, "T0")
            if variant == "int_ones":              # a mask of ones is the NULL form
                b = iu.arguments(T0, T1, expected, None, r, c, form, ld, ldm)
                assert iu.host_fix(b)[1].tobytes() == out.tobytes(), (what, "NULL form")


def test_host_only_zeros_and_never_the_pivot_column():
    T0, T1, mask, r, c, expected = iu.sentinel_case()
    for ld, ldm in iu.pitches(T0.shape[1])[:2]:
        a = iu.arguments(T0, T1, expected, mask, r, c, "owner", ld, ldm)
        rc, out = iu.host_fix(a)
        assert rc == 0
        iu.check_result(a, out, ("sentinel", ld, ldm))


def _refusal_buffers():
    rows, C, ld, ldm = 6, 9, 11, 10
    t = iu.planted(iu.table(rows - 1, C - 1, 3, "int"), 2, 3, -3)
    T0 = iu.padded(iu.as_f64(t), ld, iu.PAD)
    T1 = np.zeros((rows, ld))                      # all zeros: a fix that ran would rewrite them
    mask = np.ones((rows, ldm), dtype=np.uint8)
    return T0, T1, mask, T0[2].copy()


def test_host_refusal_base_call_is_valid():
    """The call the refusals vary is accepted and writes, so a refusal that wrote would show."""
    from simplex_mi355x import _lib
    T0, T1, mask, prow = _refusal_buffers()
    before = T1.copy()
    args = iu.refusal_args(None, T0.ctypes.data, T1.ctypes.data, prow.ctypes.data,
                           mask.ctypes.data)
    assert _lib.load().smx_host_int_first_fix(*args) == 0
    assert (su.bits(T1) != su.bits(before))[:, :9].sum() >= 20
    assert np.array_equal(su.bits(T1[:, 9:]), su.bits(before[:, 9:]))


@pytest.mark.parametrize("name", iu.REFUSALS)
def test_host_refusals(name):
    from simplex_mi355x import _lib
    T0, T1, mask, prow = _refusal_buffers()
    before = T1.copy()
    args = iu.refusal_args(name, T0.ctypes.data, T1.ctypes.data, prow.ctypes.data,
                           mask.ctypes.data)
    assert _lib.load().smx_host_int_first_fix(*args) == -1, name
    assert T1.tobytes() == before.tobytes(), name


# ---- the host engine ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(iu.ENGINE_CASES))
def test_host_engine_get_solution(name):
    import simplex
    cons, func = iu.engine_input(name)
    sm = simplex.SimplexMethod(cons, func, device="cpu")
    assert sm.backend == "host"
    iu.check_solution(sm.get_solution(max_pivots=iu.ENGINE_PIVOTS), name, simplex)


@pytest.mark.parametrize("name", list(iu.ENGINE_CASES))
def test_host_engine_chained_solve(name):
    import simplex
    cons, func = iu.engine_input(name)
    sm = simplex.SimplexMethod(cons, func, device="cpu")
    out = sm.solve(record_history=False, max_pivots=iu.ENGINE_PIVOTS, chunk=3)
    iu.check_final(sm, out, name, simplex)


def test_host_engine_x1_is_the_fixed_zero():
    """x1_zero: x1 after the first pivot is -0 / e of an int 0: -0.0 in the reference's ints,
    +0.0 in fp64.  The step's x1 is read from the fixed table."""
    import math
    import simplex
    snaps = iu.engine_reference("x1_zero")[0]
    assert snaps[1]["x1"] == 0 and math.copysign(1.0, snaps[1]["x1"]) == -1.0
    cons, func = iu.engine_input("x1_zero")
    fl = simplex.SimplexMethod([[float(x) for x in row] for row in cons], [float(x) for x in func],
                               device="cpu").get_solution(max_pivots=1)
    assert fl[1].x1 == 0 and math.copysign(1.0, fl[1].x1) == 1.0   # what fp64 alone gives
    cons, func = iu.engine_input("x1_zero")
    got = simplex.SimplexMethod(cons, func, device="cpu").get_solution(max_pivots=1)
    assert got[1].x1 == 0 and math.copysign(1.0, got[1].x1) == -1.0


def test_host_engine_largest_exact_ints():
    """Ints of magnitude 2^26 - 1, the largest `_int_entries` takes without its warning: every
    product (< 2^52) and difference (< 2^53) of the first pivot is exact in fp64, so the pivot
    equals Python's int arithmetic in every bit, and no warning is raised."""
    import simplex
    from oracle import restated
    B = (1 << 26) - 1
    rnd = random.Random(26)
    cons = [[rnd.choice([B, -B, B - 1, 1 - B, 0, 1, -1, 3]) for _ in range(6)]
            + [rnd.choice([0, 1, B])] for _ in range(6)]
    func = [rnd.choice([-B, -1, 0, 2]) for _ in range(6)] + [B]
    assert max(abs(x) for row in cons + [func] for x in row) == B
    st = restated.pick(cons + [func], 6, 6, 7)
    assert st[0] == "pivot"
    want = restated.pivot([list(row) for row in cons] + [list(func)], st[1], st[2])
    assert abs(cons[st[1]][st[2]]) >= B - 1        # the pivot element itself is that large
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        sm = simplex.SimplexMethod([list(row) for row in cons], list(func), device="cpu")
        got = sm.get_solution(max_pivots=1)
    assert (got[0].i, got[0].j) == (st[1], st[2])
    iu.same_table_bits(got[1].table, want, "2^26 - 1")
