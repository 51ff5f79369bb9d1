"""GPU: batched mid-sized LPs (one workgroup per LP, tableau in LDS) bit for bit against the C
oracle, the reference's fixtures and SimplexMethod."""
from __future__ import annotations

import random
from collections import Counter

import numpy as np
import pytest

from batch_util import (OUTCOME, case, no_fallback as _no_fallback,
                        same_as_oracle as _same_as_oracle, same_solution as _same_solution,
                        solve as _solve, trajectory_fixtures_through, xv_follows_the_labels)
from golden_util import dec, dec_input, dec_table, load, same_table, same_value

pytestmark = pytest.mark.gpu

# kind, n, m, cap, the C oracle's outcomes over seeds 0..15 (run on the CPU when this file was
# written; every final table finite)
SHAPES = [
    ("uniform", 65, 65, 1024, {"optimum": 9, "not_converge": 7}),
    ("uniform", 300, 40, 1024, {"optimum": 16}),
    ("uniform", 40, 300, 1024, {"not_converge": 16}),
    ("mixed", 120, 8, 1024, {"incorrect": 16}),
    ("mixed", 70, 5, 1024, {"incorrect": 16}),
    ("mixed", 65, 65, 96, {"cap": 16}),
    ("degenerate_mixed", 65, 65, 96, {"cap": 16}),     # integer-valued entries: ties, +-0 ratios
    ("uniform", 64, 2, 64, {"optimum": 16}),           # 65 rows: first shape past one wave
    ("uniform", 3, 64, 64, {"not_converge": 16}),      # 65 columns
]
SEEDS = range(16)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def _flen(kind, n, m, seed):
    """Half the LPs of the first launch carry len(function) = m + 1 (the last entry is the
    generator's "-b" slot of the f-row)."""
    return m + 1 if (kind, n, m) == ("uniform", 65, 65) and seed % 2 else m


def _case(kind, n, m, seed, cap):
    return case(kind, n, m, seed, cap, _flen(kind, n, m, seed))


@pytest.mark.parametrize("kind,n,m,cap,expect", SHAPES,
                         ids=[f"{k}-{n}x{m}-cap{c}" for k, n, m, c, _ in SHAPES])
def test_shapes_bitwise_vs_oracle(kind, n, m, cap, expect):
    refs = [_case(kind, n, m, s, cap) for s in SEEDS]
    seen = Counter(OUTCOME[r[3]] for r in refs)
    assert seen == expect                                    # the generator still makes the case
    assert all(np.isfinite(r[2]).all() for r in refs)
    if (kind, n, m) == ("uniform", 65, 65):
        assert sorted({r[1] for r in refs}) == [m, m + 1]
    out = _solve([(r[0], n, m, r[1]) for r in refs], cap)
    for s, ref in zip(SEEDS, refs):
        _same_as_oracle(out, s, n, m, ref, (kind, n, m, s))
    assert Counter(OUTCOME[int(v)] for v in out["status"]) == expect


def test_shape_table_holds_all_four_outcomes():
    seen = set()
    for kind, n, m, cap, _ in SHAPES:
        seen |= {OUTCOME[_case(kind, n, m, s, cap)[3]] for s in SEEDS}
    assert seen == {"optimum", "incorrect", "not_converge", "cap"}


def test_mixed_dims_in_one_launch():
    """65 x 65, 70 x 5 and 120 x 8 together: Rmax = 121, ldb = 66, each LP's own n, m inside the
    launch's padding."""
    picks = [("uniform", 65, 65, 1024), ("mixed", 70, 5, 1024), ("mixed", 120, 8, 1024)]
    cases, refs = [], []
    for s in range(5):
        for kind, n, m, cap in picks:
            ref = _case(kind, n, m, s, cap)
            refs.append((n, m, ref))
            cases.append((ref[0], n, m, ref[1]))
    out = _solve(cases, 1024, Rmax=121, ldb=66)
    assert out["final"].shape[1:] == (121, 66)
    for q, (n, m, ref) in enumerate(refs):
        _same_as_oracle(out, q, n, m, ref, q)
    assert {OUTCOME[int(v)] for v in out["status"]} == {"optimum", "not_converge", "incorrect"}


def test_envelope_edge():
    """The largest square the library admits runs; one more row and column is refused."""
    from oracle import c_oracle
    from simplex_mi355x import lp
    from simplex_mi355x.batch import solve_batch_arrays, wg_lds_bytes
    n = 64
    while wg_lds_bytes(n + 2, n + 2) >= 0:
        n += 1
    assert 65 < n < 1000 and wg_lds_bytes(n + 1, n + 1) >= 0
    cases = [(lp.dense_tableau("uniform", s, n, n), n, n, n) for s in range(4)]
    out = _solve(cases, 64)
    for q, (T, _, _, _) in enumerate(cases):
        Tref, st, done, log = c_oracle.run(T, n, n, n, 64)
        _same_as_oracle(out, q, n, n, (T, n, Tref, st, done, log), (n, q))
    tabs = np.zeros((1, n + 2, n + 2))
    tabs[0, :, :] = lp.dense_tableau("uniform", 0, n + 1, n + 1)
    dims = np.array([[n + 1, n + 1, n + 1]], dtype=np.int32)
    for kernel in ("auto", "workgroup"):
        with pytest.raises(ValueError, match="envelope"):
            solve_batch_arrays(tabs, dims, 64, kernel=kernel)


def test_trajectory_fixtures_through_workgroup_kernel(monkeypatch):
    """batch_util.trajectory_fixtures_through on k_batch_wg."""
    trajectory_fixtures_through("workgroup", monkeypatch)


def test_examples_through_workgroup_kernel(monkeypatch):
    """The examples.json cases without int entries (today each of the seven holds one, so each
    routes "single" and this runs none; a float-only example added later is checked in full)."""
    from simplex_mi355x.batch import route, solve_batch
    import simplex
    _no_fallback(monkeypatch)
    ex = load("examples.json")
    names = [k for k in ex if route(*dec_input(ex[k]["input"])) != "single"]
    probs = [dec_input(ex[k]["input"]) for k in names]
    results, statuses = solve_batch(probs, max_pivots=50, history=True, kernel="workgroup")
    for name, got in zip(names, results):
        exp = ex[name]["solution"]
        assert len(got) == len(exp), name
        for g, e in zip(got, exp):
            if e["kind"] == "error":
                assert isinstance(g, simplex.Error) and str(g) == e["message"]
                continue
            assert (g.row, g.column, g.i, g.j) == (e["row"], e["column"], e["i"], e["j"])
            assert same_table(g.table, dec_table(e["table"]), signed_zero=True), name
            for key in ("x1", "x2", "optimum"):
                assert same_value(getattr(g, key), dec(e[key]), signed_zero=True)


def test_history_snapshots_replay_the_oracle_log():
    from oracle import c_oracle
    refs = [_case("uniform", 65, 65, s, 40) for s in range(8)]
    out = _solve([(r[0], 65, 65, r[1]) for r in refs], 40, history=True)
    assert out["snaps"].shape[1:] == (66, 66)
    for q, (T, flen, Tref, st, done, log) in enumerate(refs):
        _same_as_oracle(out, q, 65, 65, refs[q], q)
        snaps = out["snaps"][out["snap_off"][q]:out["snap_off"][q + 1]]
        assert len(snaps) == done == 40
        cur = np.array(T)
        for k, (r, c) in enumerate(log):
            cur = c_oracle.pivot(cur, int(r), int(c))
            assert np.array_equal(snaps[k].view(np.int64), cur.view(np.int64)), (q, k)


@pytest.mark.parametrize("history", [True, False])
def test_solve_batch_routes_and_keeps_order(history):
    """Wave, workgroup, int-entry and IndexError problems shuffled into one call: results come
    back in input order and equal SimplexMethod's, problem by problem."""
    from simplex_mi355x import lp
    from simplex_mi355x.batch import route, solve_batch
    import simplex
    cap = 24
    rng = np.random.default_rng(7)
    probs = []
    for _ in range(6):
        A = rng.uniform(-50, 50, size=(3, 2))
        b = rng.uniform(-100, 400, size=3)
        probs.append(([list(map(float, A[i])) + [float(b[i])] for i in range(3)],
                      list(map(float, rng.uniform(-3, 3, size=2)))))
    for s in range(3):
        T = _case("uniform", 65, 65, s, 40)[0]
        probs.append((T[:65].tolist(), T[65, :65].tolist()))
    T = _case("mixed", 70, 5, 0, 1024)[0]
    probs.append((T[:70].tolist(), T[70, :5].tolist()))
    probs.append(([[1, 2, -3], [2, 1, 4], [-1, 1, 2]], [-1, -2]))            # int entries
    probs.append(([[1.0, 2.0], [-2.0, 1.0]], [-1.0]))                          # IndexError
    random.Random(3).shuffle(probs)
    assert Counter(route(c, f) for c, f in probs) == {"wave": 6, "workgroup": 4, "single": 2}
    results, statuses = solve_batch(probs, max_pivots=cap, history=history)
    assert len(results) == len(probs)
    raised = 0
    for k, ((cons, func), got) in enumerate(zip(probs, results)):
        try:
            sm = simplex.SimplexMethod([list(r) for r in cons], list(func))
            exp = (sm.get_solution(max_pivots=cap) if history else
                   sm.solve(record_history=False, max_pivots=cap))
        except IndexError:
            assert isinstance(got, IndexError) and statuses[k] == "exception"
            raised += 1
            continue
        _same_solution(got, exp, k)
        assert statuses[k] == sm.status, k
    assert raised == 1


def test_arrays_api_takes_66_by_66():
    """[16][66][66] was outside the envelope before the workgroup kernel existed."""
    refs = [_case("uniform", 65, 65, s, 1024) for s in SEEDS]
    out = _solve([(r[0], 65, 65, r[1]) for r in refs], 1024)
    assert out["final"].shape == (16, 66, 66)
    assert out["rc"].shape == (16, 1024, 2) and out["xv"].shape == (16, 1024, 2)
    assert [int(v) for v in out["npivots"]] == [r[4] for r in refs]
    xv_follows_the_labels(out, refs, 65)
