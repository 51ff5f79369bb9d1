"""Tables whose "first index" winners sit past the first wave, workgroup, strided pass, sweep chunk
and rank: the constructed tables, a census of where the C oracle's pivots land on them, and the
comparison that test_late_index_oracle.py (CPU) and test_gpu_late_index.py (GPU) share.

Every selection of the engine is a first-index search (the first "-b" < 0, the first T[r][j] > 0
of that row, the first f[j] < 0, the first ratio candidate) followed by a merge across lanes,
waves, strided loop passes, workgroups, column chunks and ranks.  On the seeded tables of
lp.dense_tableau the winner of the first three searches is never past index 32 (the
testing section, holds the count), so a merge that is wrong for any other winner passes there.
Three kinds of table move the winners:

embedded   a dense live LP in rows [r0, r0 + tr) and columns [c0, c0 + tc) of a larger table.
           Live rows are exactly 0.0 in every other column; every other row is 0.0 in the live
           columns, dense elsewhere, with "-b" > 0; the f-row is positive outside the live
           columns.  Then every pivot stays inside the live block for ever, in both phases: an
           outer row has a pivot-column entry of +-0, so it is no ratio candidate and its "-b"
           keeps its sign ((x e - p 0) / e has the sign of x); an outer column of a live row
           stays +-0 (the pivot row's entry there is +-0); an outer f entry stays positive.
steep      a fully dense uniform table whose f-row is U(50, 100) on the first m - tc columns and
           U(-1, 1) on the last tc: no zero shortcuts, and the entering column stays in the last
           tc columns for the chain lengths used here (census-checked).
planted    one decision whose answer is known by construction: the only negative "-b" at row r*
           and the only positive entry of that row at c*; no positive entry (INCORRECT); the
           only negative f at c*; none (OPTIMUM); the only one at j >= flen (FSHORT); an entering
           column of +-0 (NOT_CONVERGE); two rows with exactly equal largest negative ratios (the
           later one wins); two zero-ratio rows, one of them -0.0 (the first wins); a NaN ratio
           on the first candidate (it sticks) and on a later one (ignored).  The positions come
           from POSITIONS as the shape allows: both sides of the wave edge (62, 63, 64), of the
           256-row workgroup edge, of the 1024 stride of the strided loops, and the last index.

census() walks the oracle's own pivots (c_oracle.pick / c_oracle.pivot) and counts where they
land; CONDITIONS / check_census hold what each case must keep producing, so a generator change
that moved the winners back to the front fails on the CPU by name.
"""
from __future__ import annotations

import functools

import numpy as np

import special_values as sv

nan = float("nan")
PIVOT, OPTIMUM, INCORRECT, NOT_CONVERGE, FSHORT = 0, 1, 2, 3, 4

POSITIONS = (0, 62, 63, 64, 255, 256, 1023, 1024)
# (r1, r2) of the two-row decisions: two lanes of one wave, two waves, two 256-row workgroups,
# both sides of 1024, and one lane of a 1024-stride loop twice (r2 = r1 + 1024); "last" is n - 1
ROW_PAIRS = ((62, 63), (63, 64), (0, 64), (255, 256), (64, 1023), (1023, 1024), (0, 1024),
             (62, 1086), (256, "last"), (0, "last"))


# ---------------------------------------------------------------------------------------------
# chains
def embedded(seed, n, m, r0, c0, tr, tc, mixed):
    """The embedded table described above; the live LP is lp.dense_tableau("mixed" | "uniform",
    seed, tr, tc)."""
    from simplex_mi355x import lp
    assert 0 <= r0 and r0 + tr <= n and 0 <= c0 and c0 + tc <= m
    rng = np.random.default_rng([seed, 91])
    live = lp.dense_tableau("mixed" if mixed else "uniform", seed, tr, tc)
    T = np.zeros((n + 1, m + 1))
    T[:n, :m] = rng.uniform(-1.0, 1.0, size=(n, m))
    T[:n, m] = rng.uniform(0.1, 1.0, size=n)
    T[n, :m] = rng.uniform(0.1, 1.0, size=m)
    T[:n, c0:c0 + tc] = 0.0
    T[r0:r0 + tr, :m] = 0.0
    T[r0:r0 + tr, c0:c0 + tc] = live[:tr, :tc]
    T[r0:r0 + tr, m] = live[:tr, tc]
    T[n, c0:c0 + tc] = live[tr, :tc]
    return T


def steep(seed, n, m, tc):
    """lp.dense_tableau("uniform", seed, n, m) with the f-row U(50, 100) on the first m - tc
    columns (the last tc keep the generator's U(-1, 1))."""
    from simplex_mi355x import lp
    T = lp.dense_tableau("uniform", seed, n, m)
    rng = np.random.default_rng([seed, 93])
    T[n, :m - tc] = rng.uniform(50.0, 100.0, size=m - tc)
    return T


# name -> (generator, its arguments, pivots asked, what the census must find besides the
# generator's own condition).  "end": the chain ends by itself inside the k asked.
#
# Shapes: 1100 x 1300 with the live block at rows and columns >= 1026 is past every 1024 edge; the
# resident loop's workgroup counts need a table one workgroup's LDS holds (100 x 120, the live
# rows in the last row blocks); the block pivots run 1025 x 1300 with a 128 x 128 live block as
# the tail of the table, once more from r0 = 895 (odd, r0 % 4 == 3: the block starts inside a row
# pair and a row quad) and once with a 9 x 9 live block whose chain ends in NOT_CONVERGE inside a
# block; the batch tiers 63 x 63 (lanes 40 to 62), 130 x 130, 200 x 200 and 130 x 1100.
E, S = "embedded", "steep"
CASES = {
    "chain_u": (E, (11, 1100, 1300, 1026, 1026, 74, 274, False), 40, ("enter1024",)),
    "chain_m": (E, (11, 1100, 1300, 1026, 1026, 74, 274, True), 40, ("p1row1024", "p1col1024")),
    "chain_steep": (S, (11, 300, 1300, 200), 40, ("enter1024",)),
    "res_m": (E, (11, 100, 120, 60, 70, 40, 50, True), 40, ()),
    "res_steep": (S, (11, 100, 120, 40), 40, ()),
    "blk_u": (E, (11, 1025, 1300, 897, 1172, 128, 128, False), 51, ("enter1024",)),
    "blk_m": (E, (11, 1025, 1300, 897, 1172, 128, 128, True), 51, ("p1col1024",)),
    "blk_m_odd": (E, (12, 1025, 1300, 895, 1170, 128, 128, True), 51, ("p1col1024",)),
    "blk_steep": (S, (11, 1025, 1300, 200), 51, ("enter1024",)),
    "blk_end": (E, (2, 1025, 1300, 1015, 1290, 9, 9, False), 51, ("end", "enter1024")),
    "wave_u": (E, (11, 63, 63, 40, 40, 23, 23, False), 30, ()),
    "wave_m": (E, (11, 63, 63, 40, 40, 23, 23, True), 30, ()),
    "wg_u": (E, (11, 130, 130, 70, 70, 60, 60, False), 40, ()),
    "wg_m": (E, (11, 130, 130, 70, 70, 60, 60, True), 40, ()),
    "wg_steep": (S, (11, 130, 130, 40), 40, ()),
    "gm_u": (E, (11, 200, 200, 120, 120, 80, 80, False), 40, ()),
    "gm_m": (E, (11, 200, 200, 120, 120, 80, 80, True), 40, ()),
    "gm_steep": (S, (11, 200, 200, 60), 40, ()),
    "gm_wide_m": (E, (11, 130, 1100, 60, 1030, 70, 70, True), 40, ("p1col1024",)),
    "gm_wide_u": (E, (11, 130, 1100, 60, 1030, 70, 70, False), 40, ("enter1024",)),
}
# Row shards of 300 x 260 (row_range: n // world rows each): the live rows owned by the last rank
# alone, and straddling two ranks.  The phase-1 rows of a mixed live block stay within its first
# ten rows or so, so a straddling block starts three rows above the rank boundary (150 of world
# 2, 225 of world 4): then the phase-1 owner changes along the chain.
# name -> (case arguments, world, pivots, straddles)
SHARDED = {
    "w2_last_m": ((11, 300, 260, 200, 150, 80, 100, True), 2, 24, False),
    "w2_straddle_m": ((11, 300, 260, 147, 150, 80, 100, True), 2, 24, True),
    "w2_straddle_u": ((11, 300, 260, 110, 150, 80, 100, False), 2, 24, True),
    "w4_last_m": ((11, 300, 260, 230, 150, 70, 100, True), 4, 24, False),
    "w4_last_u": ((11, 300, 260, 230, 150, 70, 100, False), 4, 24, False),
    "w4_straddle_m": ((11, 300, 260, 222, 150, 70, 100, True), 4, 24, True),
}

CONDITIONS = {
    "embedded": "every step has r0 <= r < r0 + tr and c0 <= c < c0 + tc (derivable, so asserted "
                "for all steps); mixed: at least one phase-1 step; uniform: at least one phase-2 "
                "step; the final table finite",
    "steep": "every step is phase 2 and every entering column is >= m - tc; the final table "
             "finite",
    "all": "all k pivots done (an \"end\" case: NOT_CONVERGE after at least 2 and fewer than k "
           "pivots), at least 2 distinct pivot rows and 2 distinct pivot columns",
    "p1row1024 / p1col1024 / enter1024": "at least one phase-1 row / phase-1 column / phase-2 "
                                         "entering column at or past 1024",
    "sharded": "at least one phase-1 (mixed) or pivot-row (uniform) owner that is not rank 0; "
               "straddling cases: the owner changes at least once along the chain",
}


def table(name):
    kind, args = CASES[name][:2]
    return embedded(*args) if kind == E else steep(*args)


def dims(name):
    """(n, m) of a CASES entry."""
    return CASES[name][1][1:3]


def owner_of(r, n, world):
    """The rank whose row_range(n, rank, world) = [rank n // world, (rank + 1) n // world) holds
    row r."""
    return next(p for p in range(world) if (p + 1) * n // world > r)


def census(T, n, m, k, flen=None, world=None):
    """k steps of the oracle (c_oracle.pick / c_oracle.pivot), counted on the oracle's tables
    alone: per step the phase, r and c; over the chain the steps with r or c at or past 64 and
    at or past 1024, the distinct rows and columns, and for `world` ranks the owner of each
    step's row with the number of times it changes."""
    from oracle import c_oracle
    flen = m if flen is None else flen
    cur = np.ascontiguousarray(T, dtype=np.float64).copy()
    steps, status = [], 0
    with np.errstate(all="ignore"):
        for _ in range(k):
            st, r, c = c_oracle.pick(cur, n, m, flen)
            if st != 0:
                status = st
                break
            steps.append((1 if (cur[:n, m] < 0).any() else 2, int(r), int(c)))
            cur = c_oracle.pivot(cur, r, c, threads=4)
    out = dict(status=status, done=len(steps), steps=steps, final=cur,
               late64=sum(r >= 64 or c >= 64 for _, r, c in steps),
               late1024=sum(r >= 1024 or c >= 1024 for _, r, c in steps),
               rows=len({r for _, r, _ in steps}), cols=len({c for _, _, c in steps}),
               p1_rows=[r for p, r, _ in steps if p == 1],
               p1_cols=[c for p, _, c in steps if p == 1],
               enter=[c for p, _, c in steps if p == 2])
    if world:
        out["owners"] = [owner_of(r, n, world) for _, r, _ in steps]
        out["p1_owners"] = [owner_of(r, n, world) for p, r, _ in steps if p == 1]
        out["owner_changes"] = sum(a != b for a, b in zip(out["owners"], out["owners"][1:]))
    return out


def check_census(kind, args, k, cen, need=(), world=None, straddles=False):
    """Assert CONDITIONS on a census of k steps of a case (generator kind, its arguments)."""
    what = (kind, args, k, {a: b for a, b in cen.items() if a != "final"})
    n, m = args[1:3]
    steps = cen["steps"]
    if "end" in need:
        assert cen["status"] == NOT_CONVERGE and 2 <= cen["done"] < k, what
    else:
        assert cen["status"] == 0 and cen["done"] == k, what
    assert cen["rows"] >= 2 and cen["cols"] >= 2, what
    body = np.concatenate([cen["final"][:n].ravel(), cen["final"][n, :m]])
    assert np.isfinite(body).all(), what
    if kind == E:
        _, _, _, r0, c0, tr, tc, mixed = args
        assert all(r0 <= r < r0 + tr and c0 <= c < c0 + tc for _, r, c in steps), what
        assert len(cen["p1_rows"] if mixed else cen["enter"]) >= 1, what
    elif kind == S:
        tc = args[3]
        assert not cen["p1_rows"] and all(c >= m - tc for c in cen["enter"]), what
    else:
        raise ValueError(kind)
    if "p1row1024" in need:
        assert max(cen["p1_rows"]) >= 1024, what
    if "p1col1024" in need:
        assert max(cen["p1_cols"]) >= 1024, what
    if "enter1024" in need:
        assert max(cen["enter"]) >= 1024, what
    if world:
        owners = cen["p1_owners"] if args[-1] else cen["owners"]
        assert any(o != 0 for o in owners), what
        if straddles:
            assert cen["owner_changes"] >= 1, what


@functools.cache
def reference(name, k=None):
    """(T, flen, oracle final table, status, pivots, log) of a CASES or SHARDED entry over k
    pivots (default: the entry's own), computed once and shared (read-only)."""
    from oracle import c_oracle
    if name in SHARDED:
        args, _, k0, _ = SHARDED[name]
        T = embedded(*args)
        n, m = args[1:3]
    else:
        T, k0 = table(name), CASES[name][2]
        n, m = dims(name)
    Tref, st, done, log = c_oracle.run(T, n, m, m, k0 if k is None else k, threads=8)
    for a in (T, Tref, log):
        a.setflags(write=False)
    return T, m, Tref, st, done, log


# ---------------------------------------------------------------------------------------------
# planted single decisions
def places(size):
    """POSITIONS inside [0, size) and the last index."""
    return sorted({p for p in POSITIONS if p < size} | {size - 1})


def row_pairs(n):
    """ROW_PAIRS inside n rows ("last" = n - 1), and the last two rows."""
    out = []
    for a, b in ROW_PAIRS + ((n - 2, n - 1),):
        b = n - 1 if b == "last" else b
        if 0 <= a < b < n and (a, b) not in out:
            out.append((a, b))
    return out


@functools.lru_cache(maxsize=4)
def _quiet(n, m):
    """A table with nothing to select: A ~ U(-1, 1), "-b" and the f-row ~ U(0.1, 1)."""
    rng = np.random.default_rng([n, m, 92])
    T = np.zeros((n + 1, m + 1))
    T[:n, :m] = rng.uniform(-1.0, 1.0, size=(n, m))
    T[:n, m] = rng.uniform(0.1, 1.0, size=n)
    T[n, :m] = rng.uniform(0.1, 1.0, size=m)
    T.setflags(write=False)
    return T


KINDS = ("phase1", "incorrect", "fneg", "optimum", "fshort", "notconv", "tie", "zero",
         "zero_neg", "nan_first", "nan_later")


def planted(kind, n, m, at):
    """(T, flen, (status, r, c)): the table of one planted decision and the pick it must give,
    in the oracles' convention (INCORRECT: (r, -1); NOT_CONVERGE: (-1, c); OPTIMUM, FSHORT:
    (-1, -1)).

    phase1     at = (r, c): "-b"[r] = -0.5 is the only negative, row r is negative but for
               T[r][c] = 0.75
    incorrect  at = (r,): the same row with no positive entry (a few are +-0)
    fneg       at = (r, c): f[c] = -0.5 is the only negative; column c is positive (positive
               ratios, never chosen) but for T[r][c] = -1
    optimum    at = (): the quiet table
    fshort     at = (j, flen), j >= flen < m: f[j] = -0.5 is the only negative
    notconv    at = (c,): f[c] < 0 and column c is +0.0 and -0.0 by turns
    tie        at = (r1, r2, c): ratios 1 / -4 at r1 and 0.5 / -2 at r2, -0.3 or less in every
               fifth other row, positive elsewhere: r2 wins
    zero       at = (z1, z2, c): "-b" = 0.0 at z1 (ratio +0.0) and -0.0 at z2 (ratio -0.0), every
               other ratio positive: z1 wins
    zero_neg   the same with the -0.0 ratio at z1 (0.0 / a negative entry)
    nan_first  at = (r1, r2, c): column c is 0.0 above r1, "-b"[r1] = NaN, and r2 holds the
               best ordinary ratio: r1 wins
    nan_later  at = (rn, rw, c): "-b"[rn] = NaN on a row that is not the first candidate, rw the
               only negative ratio: rw wins
    """
    T = _quiet(n, m).copy()
    flen = m
    if kind == "phase1" or kind == "incorrect":
        r = at[0]
        T[r, :m] = -np.abs(T[r, :m]) - 0.1
        T[r, m] = -0.5
        if kind == "phase1":
            T[r, at[1]] = 0.75
            return T, flen, (PIVOT, r, at[1])
        T[r, 0:m:7] = 0.0
        T[r, 3:m:7] = -0.0
        return T, flen, (INCORRECT, r, -1)
    if kind == "optimum":
        return T, flen, (OPTIMUM, -1, -1)
    if kind == "fshort":
        j, flen = at
        assert 2 <= flen <= j < m
        T[n, j] = -0.5
        return T, flen, (FSHORT, -1, -1)
    c = at[-1]
    T[n, c] = -0.5
    col = T[:n, c]
    if kind == "notconv":
        col[0::2], col[1::2] = 0.0, -0.0
        return T, flen, (NOT_CONVERGE, -1, c)
    col[:] = np.abs(col) + 0.1
    if kind == "fneg":
        col[at[0]] = -1.0
        return T, flen, (PIVOT, at[0], c)
    a, b = at[:2]
    if kind == "tie":
        col[2::5] = -1.0
        T[2:n:5, m] = np.maximum(T[2:n:5, m], 0.3)
        col[a], T[a, m] = -4.0, 1.0
        col[b], T[b, m] = -2.0, 0.5
        return T, flen, (PIVOT, b, c)
    if kind == "zero":
        T[a, m], T[b, m] = 0.0, -0.0
        return T, flen, (PIVOT, a, c)
    if kind == "zero_neg":
        col[a], T[a, m] = -col[a], 0.0
        T[b, m] = 0.0
        return T, flen, (PIVOT, a, c)
    if kind == "nan_first":
        col[:a] = 0.0
        T[a, m] = nan
        col[b] = -1.0
        return T, flen, (PIVOT, a, c)
    if kind == "nan_later":
        assert a != 0
        T[a, m] = nan
        col[b] = -1.0
        return T, flen, (PIVOT, b, c)
    raise ValueError(kind)


def planted_cases(n, m):
    """[(kind, at)] for an n x m table: every row position with a column position taken from the
    other end of its list, every row pair in both roles with the columns in turn."""
    R, C = places(n), places(m)
    out = [("optimum", ())]
    for i, r in enumerate(R):
        c = C[-1 - i % len(C)]
        out += [("phase1", (r, c)), ("fneg", (r, c)), ("incorrect", (r,))]
    out += [("notconv", (c,)) for c in C]
    out += [("fshort", (j, j)) for j in C if 2 <= j < m] + [("fshort", (m - 1, 2))]
    for i, (a, b) in enumerate(row_pairs(n)):
        c = C[i % len(C)]
        out += [("tie", (a, b, c)), ("zero", (a, b, c)), ("zero_neg", (a, b, c)),
                ("nan_first", (a, b, c)), ("nan_later", (b, a, c))]
        if a != 0:
            out.append(("nan_later", (a, b, c)))
    return out


def planted_id(case):
    kind, at = case
    return "-".join([kind] + [str(x) for x in at])


def planted_reference(kind, n, m, at):
    """(T, flen, oracle table after at most one pivot, status, pivots, log, planted pick)."""
    from oracle import c_oracle
    T, flen, want = planted(kind, n, m, at)
    Tref, st, done, log = c_oracle.run(T, n, m, flen, 1, threads=4)
    return T, flen, Tref, st, done, log, want


# ---------------------------------------------------------------------------------------------
# the comparison
def same_as_oracle(dev, ref, n, m, what):
    """A tableau object (DeviceTableau, or the host engine's HostTableau) after its run against a
    reference tuple: pivot count, log, terminal status and the table by bits (NaN positions equal
    where a planted NaN is in it: special_values.same_table_as_oracle)."""
    Tref, st, done, log = ref[2:6]
    ctl = dev.sync_state()
    assert int(ctl["npivots"]) == done, (what, int(ctl["npivots"]), done)
    got = dev.read_log(0, done)
    assert np.array_equal(got, log), (what, got.tolist(), log.tolist())
    assert bool(ctl["term"]) == (st != 0), what
    if st != 0:
        assert int(ctl["sel_status"]) == st, (what, int(ctl["sel_status"]), st)
    sv.same_table_as_oracle(dev.download(), Tref, n, m, what)


def batch_member_same_as_oracle(out, q, n, m, ref, what):
    """Member q of a solve_batch_arrays launch against a reference tuple."""
    sv.batch_same_as_oracle(out, q, n, m, (ref[0],) + tuple(ref[2:6]), what)


# ---------------------------------------------------------------------------------------------
# the reference's own answers on small tables (tests/golden/late.json, made by make_late.py)
# (name, "embedded" | "planted", arguments, pivot cap)
LATE_CASES = [
    ("emb_u", E, (5, 40, 40, 26, 27, 12, 12, False), 30),
    ("emb_m", E, (5, 40, 40, 26, 27, 12, 12, True), 30),
    ("emb_u_wide", E, (6, 38, 44, 25, 30, 12, 14, False), 30),
    ("emb_m_wide", E, (6, 38, 44, 25, 30, 12, 14, True), 30),
    ("phase1", "planted", ("phase1", 40, 40, (39, 38)), 2),
    ("incorrect", "planted", ("incorrect", 40, 40, (37,)), 2),
    ("fneg", "planted", ("fneg", 40, 40, (38, 39)), 2),
    ("fshort", "planted", ("fshort", 40, 40, (39, 39)), 2),
    ("notconv", "planted", ("notconv", 40, 40, (39,)), 2),
    ("tie", "planted", ("tie", 40, 40, (21, 38, 37)), 2),
    ("zero", "planted", ("zero", 40, 40, (30, 39, 36)), 2),
    ("zero_neg", "planted", ("zero_neg", 40, 40, (30, 39, 36)), 2),
    ("nan_first", "planted", ("nan_first", 40, 40, (33, 38, 35)), 2),
    ("nan_later", "planted", ("nan_later", 40, 40, (38, 33, 35)), 2),
]


def late_table(kind, args):
    """(T, n, m, flen) of a LATE_CASES entry."""
    if kind == E:
        return embedded(*args), args[1], args[2], args[2]
    pk, n, m, at = args
    T, flen, _ = planted(pk, n, m, tuple(at))
    return T, n, m, flen
