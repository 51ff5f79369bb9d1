"""The int first-pivot zero fix (csrc/smx_intfirst.hpp) past one pass of its geometry: inputs, the
restatement they are compared with, and a census of where the fix has work to do.  Shared by
test_intfirst.py (the host twin and the host engine, CPU) and test_gpu_intfirst.py (the kernel and
the device engine paths).

k_int_first_fix runs one workgroup of 256 threads per row, lanes striding over the columns, and a
grid of min(rows, 4096) workgroups striding over the rows.  tests/golden/intzero.json ends at
65 x 65, so neither stride, no padded pitch and no mask index past 255 ran before these cases.

table(n, m, seed, kind) is a caller's table of Python objects ((n + 1) rows of (m + 1), the f-row
at full length so that every element has a reference value); planted() sets the pivot element.
restate() gives, for a pivot (r, c): `expected`, oracle/restated.pivot on the caller's objects
(Python ints are exact: the high-precision reference, held to the reference solver's recorded
tables by test_intzero.py); T0, the table as fp64; T1, the fp64 pivot of T0 with every operation
rounded on its own (dual_util.pivot), which is what every engine leaves before the fix; and the
uint8 mask of the int entries.  T1 and `expected` are equal by value and differ by bits only in
the sign of zeros -- asserted for every case -- and census() counts those zeros by the pass of the
kernel's two strides that reaches them.  CONDITIONS / check_census hold what a case named for a
region must keep producing (at least NEED such zeros there), so a generator change that emptied a
region fails on the CPU by name instead of leaving a comparison that cannot fail.
"""
from __future__ import annotations

import ctypes
import functools
import random

import numpy as np

import dual_util
import solution_util as su

POOL = [0, 0, 0, 1, -1, 2, -2, 3, 4, -5]          # int_large of tests/golden/make_intzero.py
FLOATS = [0.0, -0.0, 1.5, -2.5, 0.25]
P_FLOAT = 0.35
NEED = 8
WG, GRID = 256, 4096                               # threads per row, workgroups per launch
PAD = -777.0                                       # fills the padding of T0 and T1


# ---------------------------------------------------------------------------------------------
# inputs
def table(n, m, seed, kind):
    """(n + 1) rows of (m + 1) Python objects: "int" from POOL; "mixed" a float of FLOATS with
    probability P_FLOAT, else an int of POOL."""
    if kind not in ("int", "mixed"):
        raise ValueError(kind)
    rnd = random.Random(seed)

    def entry():
        if kind == "mixed" and rnd.random() < P_FLOAT:
            return rnd.choice(FLOATS)
        return rnd.choice(POOL)
    return [[entry() for _ in range(m + 1)] for _ in range(n + 1)]


def planted(t, r, c, e):
    """t with the int e as its element (r, c)."""
    assert isinstance(e, int) and e != 0
    t[r][c] = e
    return t


def as_f64(t):
    return np.array([[float(x) for x in row] for row in t], dtype=np.float64)


def int_mask(t):
    return np.array([[isinstance(x, int) for x in row] for row in t], dtype=np.uint8)


def restate(t, r, c):
    """(T0, T1, expected, mask) of the caller's table t and the pivot (r, c), read-only."""
    from oracle import restated
    expected = as_f64(restated.pivot(t, r, c))
    T0 = as_f64(t)
    T1 = dual_util.pivot(T0, r, c)
    mask = int_mask(t)
    for a in (T0, T1, expected, mask):
        a.setflags(write=False)
    return T0, T1, expected, mask


def differing(T1, expected):
    """Where T1 and expected hold zeros of opposite sign, after asserting that they differ
    nowhere else: equal by value everywhere, unequal bits only where both hold a zero."""
    assert np.array_equal(T1, expected)
    diff = su.bits(T1) != su.bits(expected)
    assert ((T1 == 0.0) & (expected == 0.0))[diff].all()
    return diff


def value(t, e, pr, pc, rowr, mij, mrc, mrj, mic):
    """int_first_value of csrc/smx_intfirst.hpp in Python floats (one rounding per operation)."""
    t, e, pr, pc = float(t), float(e), float(pr), float(pc)
    if rowr:
        return (0.0 if (mij and t == 0.0) else -t) / e
    a = t * e
    b = pr * pc
    if mij and mrc and a == 0.0:
        a = 0.0
    if mrj and mic and b == 0.0:
        b = 0.0
    return (a - b) / e


def _rule_needed(T0, expected, mask, r, c, diff):
    """For the differing zeros outside the pivot row: at how many the result is the reference's
    only with the `mij && mrc` rule on t*e, and only with the `mrj && mic` rule on pr*pc."""
    e = T0[r, c]
    M = mask != 0
    with np.errstate(all="ignore"):
        a = T0 * e
        b = np.multiply.outer(T0[:, c], T0[r])
        af = np.where(M & M[r, c] & (a == 0.0), 0.0, a)
        bf = np.where(M[r][None, :] & M[:, c][:, None] & (b == 0.0), 0.0, b)
        without_a = (a - bf) / e
        without_b = (af - b) / e
        both = (af - bf) / e
    other = diff.copy()
    other[r] = False
    other[:, c] = False
    want = su.bits(expected)
    assert (su.bits(both) == want)[other].all()
    return (int((su.bits(without_a) != want)[other].sum()),
            int((su.bits(without_b) != want)[other].sum()))


def census(T0, T1, expected, mask, r, c):
    """The zeros whose sign the fix must change, counted by where the kernel reaches them."""
    diff = differing(T1, expected)
    assert not diff[:, c].any()                    # the pivot column and element never differ
    rows, C = diff.shape
    other = diff.copy()
    other[r] = False
    rule_a, rule_b = _rule_needed(T0, expected, mask, r, c, diff)
    return {
        "all": int(diff.sum()), "prow": int(diff[r].sum()), "other": int(other.sum()),
        "prow_col256": int(diff[r, WG:].sum()),
        "col0": int(other[:, :WG].sum()), "col256": int(other[:, WG:2 * WG].sum()),
        "col512": int(other[:, 2 * WG:].sum()),
        "row0": int(other[:GRID].sum()), "row4096": int(other[GRID:2 * GRID].sum()),
        "row8192": int(other[2 * GRID:].sum()),
        "row64": int(other[64:].sum()), "col256up": int(other[:, WG:].sum()),
        "rule_a": rule_a, "rule_b": rule_b,
    }


CONDITIONS = {
    "prow": "at least NEED differing zeros in the pivot row",
    "prow_only": "the same, and none in any other row (an all-int table with e > 0)",
    "prow_col256": "at least NEED of the pivot row's at columns >= 256",
    "other": "at least NEED in the other rows",
    "col256 / col512": "at least NEED in other rows at columns 256..511 / 512 and up (the second "
                       "and the later passes of a row's 256 threads)",
    "row4096 / row8192": "at least NEED in other rows at rows 4096..8191 / 8192 and up (the "
                         "second and the third pass of the 4096 workgroups)",
    "row64 / col256up": "at least NEED in other rows at rows >= 64 / columns >= 256 (engine "
                        "cases)",
    "rule_a / rule_b": "mixed tables: at least NEED zeros outside the pivot row that are right "
                       "only with the `mij && mrc` rule on t*e / the `mrj && mic` rule on pr*pc "
                       "(rule_b: in at least one case of every group, check_rule_b)",
    "e_neg / e_pos": "the pivot element is a negative / positive int",
}


def check_census(name, cen, need, e=None):
    """Assert CONDITIONS on a census: "the input no longer makes the case"."""
    what = ("the input no longer makes the case", name, need, cen)
    for key in need:
        if key == "prow_only":
            assert cen["prow"] >= NEED and cen["other"] == 0, what
        elif key == "e_neg":
            assert isinstance(e, int) and e < 0, what
        elif key == "e_pos":
            assert isinstance(e, int) and e > 0, what
        else:
            assert cen[key] >= NEED, what


# ---------------------------------------------------------------------------------------------
# the cases of the C ABI tests: (group, n, m, (r, c), e).  The smallest shapes at which each
# stride exists, and both sides of its edge: C = m + 1 of 255, 256 and 257 columns, rows = n + 1 of
# 4095, 4096 and 4097.
def _cases():
    out = []
    for m in (254, 255, 256, 512, 1099):
        out.append(("wide", 5, m, (0, 0), 3))
        out.append(("wide", 5, m, (4, m - 1), -3))
        if m > 256:
            out.append(("wide", 5, m, (2, 256), -3))
    for n in (4094, 4095, 4096, 9000):
        out.append(("tall", n, 3, (0, 0), -3))
        out.append(("tall", n, 3, (n - 1, 2), -3))
        if n > 4096:
            out.append(("tall", n, 3, (4096, 1), -3))
    out.append(("both", 300, 260, (299, 259), -3))
    return out


CASES = _cases()
KINDS = ("int", "mixed")


def case_id(case):
    group, n, m, (r, c), e = case
    return f"{group}-{n}x{m}-r{r}c{c}-e{e}"


def case_need(case, kind):
    """The regions a case is named for.  A region enters only where the shape can hold NEED
    positions in it: the 257th column of six rows (5 x 256) and the 4097th row of four columns
    (4096 x 3) are edges, run and compared like every other case but named for no region."""
    group, n, m, (r, c), e = case
    rows, C = n + 1, m + 1
    need = ["e_pos" if e > 0 else "e_neg"]
    if e > 0:
        need.append("prow_only" if kind == "int" else "prow")
        if C >= 2 * WG:
            need.append("prow_col256")
        return need                                # (a mixed table's few other zeros: no region)
    need += ["prow", "other"] if C > NEED else ["other"]
    if C >= WG + 4:
        need.append("col256")
    if C >= 2 * WG + 4:
        need.append("col512")
    if rows >= GRID + 100:
        need += ["row4096", "row8192"]
    if kind == "mixed":
        need.append("rule_a")
    return need


def check_rule_b(censuses):
    """The `mrj && mic` rule decides a zero only where t*e is a float's -0.0 and pr*pc an int
    product of zero, which depends on the pivot row drawn and not on the shape: so it is asked of
    each group, not of each case.  censuses: {case: census of its mixed table}."""
    for group in ("wide", "tall", "both"):
        best = max(cen["rule_b"] for case, cen in censuses.items() if case[0] == group)
        assert best >= NEED, ("the input no longer makes the case", group, "rule_b", best)


@functools.cache
def case_data(case, kind):
    """(T0, T1, expected, mask) of a CASES entry, computed once and shared (read-only)."""
    group, n, m, (r, c), e = case
    t = planted(table(n, m, 1000 + n + m, kind), r, c, e)
    return restate(t, r, c)


# ---------------------------------------------------------------------------------------------
# the call: buffers at a pitch, the three forms, the host twin
FORMS = ("owner", "owner_prow", "nonowner")
VARIANTS = ("int_null", "int_ones", "mixed")


def variant_data(case, variant):
    """(T0, T1, expected, mask or None) of a case under a variant of VARIANTS."""
    T0, T1, expected, mask = case_data(case, "mixed" if variant == "mixed" else "int")
    if variant == "int_null":
        return T0, T1, expected, None
    if variant == "int_ones":
        assert mask.all()
    return T0, T1, expected, mask


def padded(A, ld, fill):
    """A in a buffer of pitch ld, the padding filled with `fill`."""
    out = np.full((A.shape[0], ld), fill, dtype=A.dtype)
    out[:, :A.shape[1]] = A
    return out


def arguments(T0, T1, expected, mask, r, c, form, ld, ldm):
    """The arrays of one call: dict(T0, T1, mask, prow, maskr: contiguous arrays or None; rows, C,
    r_local, c; expected [rows][C]).  owner: the whole table, prow the row of T0 itself (prow
    None); owner_prow: the same with prow and maskr separate copies; nonowner: the table without
    its pivot row, r_local = -1, prow and maskr the owner's.  Padding: PAD in T0 and T1, 1 in the
    mask (an int entry: a read at the wrong pitch lands on it or on a neighbouring row)."""
    rows, C = T0.shape
    keep = np.arange(rows) != r if form == "nonowner" else np.ones(rows, dtype=bool)
    a = {"T0": padded(T0[keep], ld, PAD), "T1": padded(T1[keep], ld, PAD),
         "mask": None if mask is None else padded(mask[keep], ldm, 1),
         "prow": None, "maskr": None, "rows": int(keep.sum()), "C": C, "c": c, "ld": ld,
         "ldm": ldm, "r_local": -1 if form == "nonowner" else r, "expected": expected[keep]}
    if form != "owner":
        a["prow"] = T0[r].copy()
        a["maskr"] = None if mask is None else mask[r].copy()
    return a


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def host_fix(a):
    """smx_host_int_first_fix on the arrays of arguments() -> (return code, T1 buffer after)."""
    from simplex_mi355x import _lib
    T1 = a["T1"].copy()
    prow = a["T0"][a["r_local"]] if a["prow"] is None else a["prow"]
    maskr = a["maskr"]
    if maskr is None and a["mask"] is not None and a["prow"] is None:
        maskr = a["mask"][a["r_local"]]
    rc = _lib.load().smx_host_int_first_fix(_p(a["T0"]), _p(T1), a["ld"], a["rows"], a["C"],
                                            a["r_local"], a["c"], _p(prow), _p(a["mask"]),
                                            a["ldm"], _p(maskr))
    return int(rc), T1


def check_result(a, T1_after, what):
    """The table of a call by bits against the restatement, and its padding untouched."""
    C = a["C"]
    got, want = su.bits(T1_after[:, :C]), su.bits(a["expected"])
    bad = np.argwhere(got != want)
    assert not len(bad), (what, len(bad), [(int(i), int(j)) for i, j in bad[:4]])
    assert (T1_after[:, C:] == PAD).all(), (what, "padding")


def pitches(C):
    """(ld, ldm) pairs: both tight, both padded, and each padded alone."""
    return [(C, C), (C + 7, C + 5), (C + 7, C), (C, C + 5)]


# ---------------------------------------------------------------------------------------------
# only zeros, and never the pivot column
SENTINEL = 7.0


def sentinel_case():
    """(T0, T1, mask, r, c, expected): a mixed 4200 x 300 table whose T1 is SENTINEL everywhere but
    at chosen positions, which hold +0.0 or -0.0 -- in the first and in late columns and rows,
    in the pivot row, and in the pivot column (which the fix must leave alone).  expected: T1 with
    value() of T0 at every zero outside the pivot column."""
    n, m, r, c = 4200, 300, 4100, 290
    t = planted(table(n, m, 77, "mixed"), r, c, -3)
    T0, mask = as_f64(t), int_mask(t)
    T1 = np.full(T0.shape, SENTINEL)
    rnd = random.Random(78)
    spots = {(0, 0), (0, m), (n, 0), (n, m), (r, 0), (r, 255), (r, 256), (r, m), (4095, 255),
             (4096, 256), (4097, 299), (63, 64), (5, c), (4150, c), (r, c)}
    while len(spots) < 400:
        spots.add((rnd.randrange(n + 1), rnd.randrange(m + 1)))
    expected = T1.copy()
    e = T0[r, c]
    for k, (i, j) in enumerate(sorted(spots)):
        z = -0.0 if k % 2 or (i, j) == (5, c) else 0.0
        T1[i, j] = z
        if j == c:
            expected[i, j] = z
        else:
            expected[i, j] = value(T0[i, j], e, T0[r, j], T0[i, c], i == r, mask[i, j] != 0,
                                   mask[r, c] != 0, mask[r, j] != 0, mask[i, c] != 0)
    assert sum(1 for i, j in spots if j == c) >= 3 and (expected != SENTINEL).sum() > 100
    return T0, T1, mask, r, c, expected


# ---------------------------------------------------------------------------------------------
# refusals: every branch of int_first_args_ok.  Each entry changes one argument of a valid call.
REFUSALS = ("null_T0", "null_T1", "null_prow", "same_T0_T1", "rows_0", "rows_neg", "C_0", "ld_lt_C",
            "c_neg", "c_eq_C", "r_lt_m1", "r_eq_rows", "ldm_lt_C")


def refusal_args(name, T0p, T1p, prowp, maskp, rows=6, C=9, ld=11, ldm=10):
    """The argument tuple (without a stream) of a refused call: pointers as ints or None."""
    a = dict(T0=T0p, T1=T1p, ld=ld, rows=rows, C=C, r=2, c=3, prow=prowp, mask=maskp, ldm=ldm,
             maskr=None)
    change = {"null_T0": ("T0", None), "null_T1": ("T1", None), "null_prow": ("prow", None),
              "same_T0_T1": ("T0", T1p), "rows_0": ("rows", 0), "rows_neg": ("rows", -3),
              "C_0": ("C", 0), "ld_lt_C": ("ld", C - 1), "c_neg": ("c", -1), "c_eq_C": ("c", C),
              "r_lt_m1": ("r", -2), "r_eq_rows": ("r", rows), "ldm_lt_C": ("ldm", C - 1),
              None: ("c", 3)}[name]                # None: the valid call itself
    a[change[0]] = change[1]
    return (a["T0"], a["T1"], a["ld"], a["rows"], a["C"], a["r"], a["c"], a["prow"], a["mask"],
            a["ldm"], a["maskr"])


# ---------------------------------------------------------------------------------------------
# engine cases: tables whose first pivot the rule itself picks
def engine_table(n, m, seed, kind):
    """table() with the constants of the constraint rows drawn from [0, 1, 2, 3]: the run starts
    in the ratio test.  -> (constraints, function), the function at length m + 1."""
    t = table(n, m, seed, kind)
    rnd = random.Random(seed + 5000)
    for i in range(n):
        t[i][m] = rnd.choice([0, 1, 2, 3])
    return t[:n], t[n]


def late_row_table(n, m, seed):
    """A mixed engine_table whose only negative constant is the int -2 of the last constraint row,
    and that row's only positive entry the int 2 in the last column: the first pivot is
    (n - 1, m - 1)."""
    cons, func = engine_table(n, m, seed, "mixed")
    row = cons[n - 1]
    for j in range(m):
        if row[j] > 0:
            row[j] = -row[j]
    row[m - 1] = 2
    row[m] = -2
    return cons, func


def x1_table(n, m, seed, r):
    """An int engine_table whose first pivot is (r, 0) on e = -5 at a row whose constant is the
    int 0: f[0] = -1 is the first negative f entry, row r's ratio is 0 / -5, every other row's
    is positive or its column entry 0.  Then x1 after that pivot is -0 / e: +0.0 in fp64, -0.0
    in the reference's ints."""
    cons, func = engine_table(n, m, seed, "int")
    func[0] = -1
    for i in range(n):
        cons[i][0] = abs(cons[i][0])
        if cons[i][0] and cons[i][m] == 0:
            cons[i][m] = 1
    cons[r][0], cons[r][m] = -5, 0
    return cons, func


# name -> (maker, its arguments, the first pivot it must give or None, census regions)
ENGINE_CASES = {
    "wide_int": (engine_table, (40, 300, 16, "int"), (11, 1), ("e_neg", "col256up")),
    "wide_mixed": (engine_table, (40, 300, 21, "mixed"), (17, 3),
                   ("e_neg", "col256up", "rule_a", "rule_b")),
    "tall_int": (engine_table, (300, 40, 15, "int"), (189, 1), ("e_neg", "row64")),
    "tall_mixed": (engine_table, (300, 40, 14, "mixed"), (142, 3),
                   ("e_neg", "row64", "rule_a", "rule_b")),
    "late_row": (late_row_table, (130, 300, 15), (129, 299),
                 ("e_pos", "row64", "col256up", "rule_b")),
    "x1_zero": (x1_table, (40, 300, 16, 37), (37, 0), ("e_neg", "col256up")),
}
ENGINE_PIVOTS = 4


def engine_input(name):
    """A fresh (constraints, function) of an ENGINE_CASES entry (the engine keeps the caller's
    lists, so every run gets its own)."""
    maker, args = ENGINE_CASES[name][:2]
    return maker(*args)


@functools.cache
def engine_reference(name):
    """restated.Solver on the caller's objects over ENGINE_PIVOTS pivots: the first pivot in
    Python ints, the rest in Python floats -> (snapshots, first pivot (r, c), census of it)."""
    from oracle import restated
    cons, func = engine_input(name)
    snaps = restated.Solver([list(r) for r in cons], list(func)).get_solution(ENGINE_PIVOTS)
    r, c = snaps[0]["i"], snaps[0]["j"]
    cons, func = engine_input(name)
    cen = census(*restate(cons + [func], r, c), r, c)
    return snaps, (r, c), cen


def check_engine_census(name):
    snaps, rc, cen = engine_reference(name)
    want, need = ENGINE_CASES[name][2:]
    cons, func = engine_input(name)
    if want is not None:
        assert rc == want, ("the input no longer makes the case", name, rc, want)
    infos = [s for s in snaps if s["kind"] == "info"]
    assert len(infos) == ENGINE_PIVOTS + 1, ("the input no longer makes the case", name,
                                             [s["kind"] for s in snaps])
    check_census(name, cen, need, e=(cons + [func])[rc[0]][rc[1]])


def same_number(got, exp):
    from golden_util import same_value
    return same_value(got, exp, signed_zero=True)


def check_solution(got, name, simplex, tables=True):
    """A get_solution list against engine_reference: every step's (i, j), table, x1, x2 and
    optimum, zeros by sign; the list ends as the restatement's (cap, or its error message)."""
    from golden_util import same_table
    snaps = engine_reference(name)[0]
    steps = [s for s in snaps if s["kind"] == "info"]
    infos = [g for g in got if not isinstance(g, simplex.Error)]
    assert len(infos) == len(steps), (name, len(infos), len(steps))
    for k, (g, s) in enumerate(zip(infos, steps)):
        assert (g.i, g.j) == (s["i"], s["j"]), (name, k, (g.i, g.j), (s["i"], s["j"]))
        if tables and k == 0:
            assert same_table(g.table, s["table"], signed_zero=True), (name, k)
        elif tables:
            same_table_bits(g.table, s["table"], (name, k))
        for key in ("x1", "x2", "optimum"):
            assert same_number(getattr(g, key), s[key]), (name, k, key, getattr(g, key), s[key])
    if snaps[-1]["kind"] == "error":
        assert isinstance(got[-1], simplex.Error) and str(got[-1]) == snaps[-1]["message"], name
    else:
        assert not isinstance(got[-1], simplex.Error), name


def same_table_bits(got, exp, what):
    a, b = np.array(got, dtype=np.float64), np.array(exp, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.argwhere(su.bits(a) != su.bits(b))
    assert not len(bad), (what, len(bad), [(int(i), int(j)) for i, j in bad[:4]])


def check_final(sm, out, name, simplex):
    """solve(record_history=False) against engine_reference: the final table, its x1, x2 and
    optimum, the first Info's (i, j) and the pivot log."""
    snaps = engine_reference(name)[0]
    steps = [s for s in snaps if s["kind"] == "info"]
    assert sm.pivot_log == [(s["i"], s["j"]) for s in steps[:-1]], (name, sm.pivot_log)
    assert (out[0].i, out[0].j) == (steps[0]["i"], steps[0]["j"]), name
    same_table_bits(out[1].table, steps[-1]["table"], (name, "final"))
    for key in ("x1", "x2", "optimum"):
        assert same_number(getattr(out[1], key), steps[-1][key]), (name, key)
