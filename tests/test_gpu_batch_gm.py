"""GPU: batched LPs past one CU's LDS (one workgroup per LP, tableau in global memory) bit for bit
against the C oracle, the reference's fixtures and SimplexMethod."""
from __future__ import annotations

import functools
import random
from collections import Counter, defaultdict

import numpy as np
import pytest

from golden_util import dec, same_table, same_value, table_hash, trajectory_cap, trajectory_cases

pytestmark = pytest.mark.gpu

OUTCOME = {0: "cap", 1: "optimum", 2: "incorrect", 3: "not_converge"}

# kind, n, m, cap, the C oracle's outcomes over seeds 0..15 (run on the CPU when this file was
# written; every final table finite, every shape past the LDS kernel's envelope)
SHAPES = [
    ("uniform", 141, 141, 8192, {"optimum": 11, "not_converge": 5}),   # 3075..5085 pivots
    ("uniform", 200, 120, 4096, {"optimum": 16}),
    ("uniform", 120, 200, 4096, {"not_converge": 16}),
    ("uniform", 600, 40, 2048, {"optimum": 16}),
    ("uniform", 40, 600, 2048, {"not_converge": 16}),
    ("uniform", 1100, 20, 2048, {"optimum": 16}),          # more rows than threads
    ("uniform", 20, 1100, 512, {"not_converge": 16}),      # one row wider than the workgroup
    ("mixed", 3000, 8, 1024, {"incorrect": 16}),
    ("mixed", 1100, 20, 512, {"incorrect": 13, "cap": 3}),
    ("mixed", 141, 141, 96, {"cap": 16}),
    ("degenerate_mixed", 141, 141, 96, {"cap": 16}),       # integer-valued entries: ties, +-0
]
SEEDS = range(16)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def _flen(kind, n, m, seed):
    """Half the uniform 141 x 141 LPs carry len(function) = m + 1 (the last entry is the
    generator's "-b" slot of the f-row)."""
    return m + 1 if (kind, n, m) == ("uniform", 141, 141) and seed % 2 else m


@functools.lru_cache(maxsize=None)
def _case(kind, n, m, seed, cap):
    """(T, flen, oracle final table, status, pivots, log), computed once and shared."""
    from oracle import c_oracle
    from simplex_mi355x import lp
    T = lp.dense_tableau(kind, seed, n, m)
    flen = _flen(kind, n, m, seed)
    Tref, st, done, log = c_oracle.run(T, n, m, flen, cap)
    for a in (T, Tref, log):
        a.setflags(write=False)
    return T, flen, Tref, st, done, log


def _solve(cases, cap, Rmax=None, ldb=None, **kw):
    """cases: [(T, n, m, flen)] -> solve_batch_arrays output of one launch of k_batch_gm."""
    from simplex_mi355x.batch import solve_batch_arrays
    Rmax = Rmax or max(n for _, n, _, _ in cases) + 1
    ldb = ldb or max(m for _, _, m, _ in cases) + 1
    tabs = np.zeros((len(cases), Rmax, ldb))
    dims = np.zeros((len(cases), 3), dtype=np.int32)
    for q, (T, n, m, flen) in enumerate(cases):
        tabs[q, :n + 1, :m + 1] = T
        dims[q] = (n, m, flen)
    return solve_batch_arrays(tabs, dims, cap, kernel="global", **kw)


def _same_as_oracle(out, q, n, m, ref, what):
    _, _, Tref, st, done, log = ref
    assert int(out["status"][q]) == st, what
    assert int(out["npivots"][q]) == done, what
    assert np.array_equal(out["rc"][q, :done], log), what
    got = np.ascontiguousarray(out["final"][q, :n + 1, :m + 1])
    assert np.array_equal(got.view(np.int64), Tref[:n + 1].view(np.int64)), what


@pytest.mark.parametrize("kind,n,m,cap,expect", SHAPES,
                         ids=[f"{k}-{n}x{m}-cap{c}" for k, n, m, c, _ in SHAPES])
def test_shapes_bitwise_vs_oracle(kind, n, m, cap, expect):
    from simplex_mi355x.batch import wg_lds_bytes
    refs = [_case(kind, n, m, s, cap) for s in SEEDS]
    seen = Counter(OUTCOME[r[3]] for r in refs)
    assert seen == expect                                    # the generator still makes the case
    assert all(np.isfinite(r[2]).all() for r in refs)
    assert wg_lds_bytes(n + 1, m + 1) == -1                  # past the LDS kernel
    if (kind, n, m) == ("uniform", 141, 141):
        assert sorted({r[1] for r in refs}) == [m, m + 1]
    out = _solve([(r[0], n, m, r[1]) for r in refs], cap)
    for s, ref in zip(SEEDS, refs):
        _same_as_oracle(out, s, n, m, ref, (kind, n, m, s))
    assert Counter(OUTCOME[int(v)] for v in out["status"]) == expect


@pytest.mark.parametrize("threads,mirrors,unroll", [(1024, 1, 4), (1024, 0, 1), (1024, 1, 8),
                                                    (512, 1, 1), (512, 0, 4), (256, 0, 8)])
def test_measurement_variants_give_the_same_bits(threads, mirrors, unroll):
    """smx_tune_batch_gm's workgroup sizes, the kernel without its LDS mirrors and without its
    loads ahead (the A/B of tools/bench_batch_gm.py) against the oracle: ties and +-0 ratios at
    141 x 141, more rows than threads at 1100 x 20, a row wider than the workgroup at 20 x 1100."""
    from simplex_mi355x import _lib
    L = _lib.load()
    prev = L.smx_tune_batch_gm(threads, mirrors, unroll)
    try:
        assert L.smx_tune_batch_gm(-1, -1, -1) == threads | mirrors << 16 | unroll << 20
        for kind, n, m, cap in (("degenerate_mixed", 141, 141, 96), ("uniform", 1100, 20, 2048),
                                ("uniform", 20, 1100, 512)):
            refs = [_case(kind, n, m, s, cap) for s in range(4)]
            out = _solve([(r[0], n, m, r[1]) for r in refs], cap)
            for s, ref in enumerate(refs):
                _same_as_oracle(out, s, n, m, ref, (kind, threads, mirrors, unroll, s))
    finally:
        L.smx_tune_batch_gm(prev & 0xffff, (prev >> 16) & 0xf, prev >> 20)
    assert L.smx_tune_batch_gm(-1, -1, -1) == prev          # what was set before is back


def test_shape_table_holds_all_four_outcomes():
    seen = set()
    for kind, n, m, cap, _ in SHAPES:
        seen |= {OUTCOME[_case(kind, n, m, s, cap)[3]] for s in SEEDS}
    assert seen == {"optimum", "incorrect", "not_converge", "cap"}


def test_mixed_dims_in_one_launch():
    """141 x 141, 600 x 40 and 20 x 1100 would pad to 601 x 1101, outside the envelope; 141 x 141,
    200 x 120 and 120 x 200 pad to 201 x 201 and run, each LP's own n, m inside the padding."""
    picks = [("uniform", 141, 141, 8192), ("uniform", 600, 40, 2048), ("uniform", 20, 1100, 512)]
    cases = []
    for kind, n, m, cap in picks:
        ref = _case(kind, n, m, 0, cap)
        cases.append((ref[0], n, m, ref[1]))
    with pytest.raises(ValueError, match="envelope"):
        _solve(cases, 64, Rmax=601, ldb=1101)
    picks = [("uniform", 141, 141, 8192), ("uniform", 200, 120, 4096), ("uniform", 120, 200, 4096)]
    cases, refs = [], []
    for s in range(4):
        for kind, n, m, cap in picks:
            ref = _case(kind, n, m, s, cap)
            refs.append((n, m, ref))
            cases.append((ref[0], n, m, ref[1]))
    out = _solve(cases, 8192, Rmax=201, ldb=201)
    assert out["final"].shape[1:] == (201, 201)
    for q, (n, m, ref) in enumerate(refs):
        _same_as_oracle(out, q, n, m, ref, q)
    assert {OUTCOME[int(v)] for v in out["status"]} == {"optimum", "not_converge"}


def _no_fallback(monkeypatch):
    from simplex_mi355x import batch

    def boom(*a, **k):
        raise AssertionError("a problem left the batch kernels")
    monkeypatch.setattr(batch, "_fallback", boom)


def test_trajectory_fixtures_through_global_kernel(monkeypatch):
    """Every capped trajectory fixture the batch kernels can take, forced through k_batch_gm:
    per-step table hashes, (i, j), x1 / x2 / optimum, final labels and the outcome -- the
    NaN-first rule, the ties and the signed zeros of ties.json / edge.json on the new code."""
    from simplex_mi355x.batch import route, solve_batch
    import simplex
    _no_fallback(monkeypatch)
    groups = defaultdict(list)
    for label, cons, func, rec in trajectory_cases():
        if route(cons, func) != "single":
            groups[trajectory_cap(rec)].append((label, cons, func, rec))
    checked = 0
    for cap, cases in groups.items():
        results, statuses = solve_batch([(c, f) for _, c, f, _ in cases], max_pivots=cap,
                                        history=True, kernel="global")
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


def test_history_snapshots_replay_the_oracle_log():
    from oracle import c_oracle
    refs = [_case("uniform", 141, 141, s, 40) for s in range(8)]
    out = _solve([(r[0], 141, 141, r[1]) for r in refs], 40, history=True)
    assert out["snaps"].shape[1:] == (142, 142)
    for q, (T, flen, Tref, st, done, log) in enumerate(refs):
        _same_as_oracle(out, q, 141, 141, refs[q], q)
        snaps = out["snaps"][out["snap_off"][q]:out["snap_off"][q + 1]]
        assert len(snaps) == done == 40
        cur = np.array(T)
        for k, (r, c) in enumerate(log):
            cur = c_oracle.pivot(cur, int(r), int(c))
            assert np.array_equal(snaps[k].view(np.int64), cur.view(np.int64)), (q, k)


def _same_solution(got, exp, what):
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


@functools.lru_cache(maxsize=None)
def _routing_problems():
    rng = np.random.default_rng(7)
    probs = []
    for _ in range(6):
        A = rng.uniform(-50, 50, size=(3, 2))
        b = rng.uniform(-100, 400, size=3)
        probs.append(([list(map(float, A[i])) + [float(b[i])] for i in range(3)],
                      list(map(float, rng.uniform(-3, 3, size=2)))))
    for s in range(3):
        T = _case("uniform", 141, 141, s, 40)[0]
        probs.append((T[:141].tolist(), T[141, :141].tolist()))
    from simplex_mi355x import lp
    for s in range(2):
        T = lp.dense_tableau("uniform", s, 65, 65)
        probs.append((T[:65].tolist(), T[65, :65].tolist()))
    probs.append(([[1, 2, -3], [2, 1, 4], [-1, 1, 2]], [-1, -2]))            # int entries
    probs.append(([[1.0, 2.0], [-2.0, 1.0]], [-1.0]))                          # IndexError
    random.Random(3).shuffle(probs)
    return probs


@functools.lru_cache(maxsize=None)
def _routing_expected(history):
    """SimplexMethod's answer per problem (None where the reference raises IndexError)."""
    import simplex
    exp = []
    for cons, func in _routing_problems():
        try:
            sm = simplex.SimplexMethod([list(r) for r in cons], list(func))
            sol = (sm.get_solution(max_pivots=24) if history else
                   sm.solve(record_history=False, max_pivots=24))
            exp.append((sol, sm.status))
        except IndexError:
            exp.append(None)
    return exp


@pytest.mark.parametrize("min_batch", [1, 4])
@pytest.mark.parametrize("history", [True, False])
def test_solve_batch_routes_and_keeps_order(monkeypatch, history, min_batch):
    """Wave, workgroup, global, int-entry and IndexError problems shuffled into one call: results
    come back in input order and equal SimplexMethod's, problem by problem.  With GM_MIN_BATCH at
    1 the three global problems run on k_batch_gm; above 3 they go through _fallback."""
    from simplex_mi355x import batch
    cap = 24
    probs = _routing_problems()
    routes = [batch.route(c, f) for c, f in probs]
    assert Counter(routes) == {"wave": 6, "workgroup": 2, "global": 3, "single": 2}
    monkeypatch.setattr(batch, "GM_MIN_BATCH", min_batch)
    fell, launched = [], []
    real_fallback, real_arrays = batch._fallback, batch.solve_batch_arrays

    def fallback(cons, func, *a, **k):
        fell.append(len(cons))
        return real_fallback(cons, func, *a, **k)

    def arrays(*a, **k):
        launched.append(k["kernel"])
        return real_arrays(*a, **k)
    monkeypatch.setattr(batch, "_fallback", fallback)
    monkeypatch.setattr(batch, "solve_batch_arrays", arrays)
    results, statuses = batch.solve_batch(probs, max_pivots=cap, history=history)
    if min_batch == 1:
        assert sorted(launched) == ["global", "wave", "workgroup"] and 141 not in fell
    else:
        assert sorted(launched) == ["wave", "workgroup"] and fell.count(141) == 3
    assert len(results) == len(probs)
    raised = 0
    for k, (exp, got) in enumerate(zip(_routing_expected(history), results)):
        if exp is None:
            assert isinstance(got, IndexError) and statuses[k] == "exception"
            raised += 1
            continue
        _same_solution(got, exp[0], k)
        assert statuses[k] == exp[1], k
    assert raised == 1


def test_xv_follows_the_labels():
    """x1, x2 after the last pivot: the "-b" entry of the row that holds the label, else 0."""
    cap = 8192
    refs = [_case("uniform", 141, 141, s, cap) for s in SEEDS]
    out = _solve([(r[0], 141, 141, r[1]) for r in refs], cap)
    assert out["final"].shape == (16, 142, 142)
    assert out["rc"].shape == (16, cap, 2) and out["xv"].shape == (16, cap, 2)
    assert [int(v) for v in out["npivots"]] == [r[4] for r in refs]
    for q, (T, flen, Tref, st, done, log) in enumerate(refs):
        where = {0: ("col", 0), 1: ("col", 1)}               # labels 'x1', 'x2' (simplex.py:152)
        for r, c in log:
            for lab, (side, at) in list(where.items()):
                if side == "col" and at == c:
                    where[lab] = ("row", int(r))
                elif side == "row" and at == r:
                    where[lab] = ("col", int(c))
        for lab in (0, 1):
            side, at = where[lab]
            want = Tref[at, 141] if side == "row" else 0.0
            assert same_value(float(out["xv"][q, done - 1, lab]), float(want)), (q, lab)
