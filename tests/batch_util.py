"""What the GPU tests of the batch kernels share: seeded cases with their C-oracle answer, one
launch through solve_batch_arrays, and the bit-for-bit comparisons."""
from __future__ import annotations

import functools
from collections import defaultdict

import numpy as np

from golden_util import dec, same_table, same_value, table_hash, trajectory_cap, trajectory_cases

OUTCOME = {0: "cap", 1: "optimum", 2: "incorrect", 3: "not_converge"}


@functools.lru_cache(maxsize=None)
def case(kind, n, m, seed, cap, flen):
    """(T, flen, oracle final table, status, pivots, log), computed once and shared."""
    from oracle import c_oracle
    from simplex_mi355x import lp
    T = lp.dense_tableau(kind, seed, n, m)
    Tref, st, done, log = c_oracle.run(T, n, m, flen, cap)
    for a in (T, Tref, log):
        a.setflags(write=False)
    return T, flen, Tref, st, done, log


def solve(cases, cap, Rmax=None, ldb=None, **kw):
    """cases: [(T, n, m, flen)] -> solve_batch_arrays output of one launch."""
    from simplex_mi355x.batch import solve_batch_arrays
    Rmax = Rmax or max(n for _, n, _, _ in cases) + 1
    ldb = ldb or max(m for _, _, m, _ in cases) + 1
    tabs = np.zeros((len(cases), Rmax, ldb))
    dims = np.zeros((len(cases), 3), dtype=np.int32)
    for q, (T, n, m, flen) in enumerate(cases):
        tabs[q, :n + 1, :m + 1] = T
        dims[q] = (n, m, flen)
    return solve_batch_arrays(tabs, dims, cap, **kw)


def same_as_oracle(out, q, n, m, ref, what):
    _, _, Tref, st, done, log = ref
    assert int(out["status"][q]) == st, what
    assert int(out["npivots"][q]) == done, what
    assert np.array_equal(out["rc"][q, :done], log), what
    got = np.ascontiguousarray(out["final"][q, :n + 1, :m + 1])
    assert np.array_equal(got.view(np.int64), Tref[:n + 1].view(np.int64)), what


def same_solution(got, exp, what):
    import simplex
    assert len(got) == len(exp), what
    for g, e in zip(got, exp):
        if isinstance(e, simplex.Error):
            assert isinstance(g, simplex.Error) and str(g) == str(e), what
            continue
        assert (g.row, g.column, g.i, g.j) == (e.row, e.column, e.i, e.j), what
        assert same_table(g.table, e.table), what
        for key in ("x1", "x2", "optimum"):
            assert same_value(getattr(g, key), getattr(e, key)), (what, key)


def no_fallback(monkeypatch):
    from simplex_mi355x import batch

    def boom(*a, **k):
        raise AssertionError("a problem left the batch kernels")
    monkeypatch.setattr(batch, "_fallback", boom)


def label_places(log):
    """Where the labels 'x1', 'x2' stand after the pivots of `log` (simplex.py:152):
    {0: (side, at), 1: (side, at)} with side "row" (basic, in row `at`) or "col"."""
    where = {0: ("col", 0), 1: ("col", 1)}
    for r, c in log:
        for lab, (side, at) in list(where.items()):
            if side == "col" and at == c:
                where[lab] = ("row", int(r))
            elif side == "row" and at == r:
                where[lab] = ("col", int(c))
    return where


def xv_follows_the_labels(out, refs, m):
    """x1, x2 after the last pivot: the "-b" entry of the row that holds the label, else 0."""
    for q, (T, flen, Tref, st, done, log) in enumerate(refs):
        where = label_places(log)
        for lab in (0, 1):
            side, at = where[lab]
            want = Tref[at, m] if side == "row" else 0.0
            assert same_value(float(out["xv"][q, done - 1, lab]), float(want)), (q, lab)


def trajectory_fixtures_through(kernel, monkeypatch):
    """Every capped trajectory fixture the batch kernels can take, forced through `kernel`:
    per-step table hashes, (i, j), x1 / x2 / optimum, final labels and the outcome -- the
    NaN-first rule, the ties and the signed zeros of ties.json / edge.json."""
    from simplex_mi355x.batch import route, solve_batch
    import simplex
    no_fallback(monkeypatch)
    groups = defaultdict(list)
    for label, cons, func, rec in trajectory_cases():
        if route(cons, func) != "single":
            groups[trajectory_cap(rec)].append((label, cons, func, rec))
    checked = 0
    for cap, cases in groups.items():
        results, statuses = solve_batch([(c, f) for _, c, f, _ in cases], max_pivots=cap,
                                        history=True, kernel=kernel)
        for (label, cons, func, rec), got, st in zip(cases, results, statuses):
            outcome = rec["outcome"]
            assert outcome["kind"] != "exception", label     # route sends those to "single"
            infos = [g for g in got if isinstance(g, simplex.Info)]
            assert [table_hash(i.table) for i in infos] == [s["hash"] for s in rec["steps"]], label
            for i, s in zip(infos, rec["steps"]):
                assert (i.i, i.j) == (s.get("i"), s.get("j")), label
                for key in ("x1", "x2", "optimum"):
                    assert same_value(getattr(i, key), dec(s[key])), (label, key)
            if outcome["kind"] == "error":
                assert str(got[-1]) == outcome["message"] and st == "error"
            elif outcome["kind"] == "optimum":
                assert st == "optimum"
            else:
                assert st == "cap"
            assert infos[-1].row == rec["row"] and infos[-1].column == rec["column"]
            checked += 1
    assert checked > 200
