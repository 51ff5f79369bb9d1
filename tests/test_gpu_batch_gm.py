"""GPU: batched LPs past one CU's LDS (one workgroup per LP, tableau in global memory) bit for bit
against the C oracle, the reference's fixtures and SimplexMethod."""
from __future__ import annotations

import functools
import random
from collections import Counter

import numpy as np
import pytest

from batch_util import (OUTCOME, case, same_as_oracle as _same_as_oracle,
                        same_solution as _same_solution, solve, trajectory_fixtures_through,
                        xv_follows_the_labels)

pytestmark = pytest.mark.gpu

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


def _case(kind, n, m, seed, cap):
    return case(kind, n, m, seed, cap, _flen(kind, n, m, seed))


def _solve(cases, cap, **kw):
    """One launch of k_batch_gm."""
    return solve(cases, cap, kernel="global", **kw)


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


def test_trajectory_fixtures_through_global_kernel(monkeypatch):
    """batch_util.trajectory_fixtures_through on k_batch_gm."""
    trajectory_fixtures_through("global", monkeypatch)


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
    xv_follows_the_labels(out, refs, 141)
