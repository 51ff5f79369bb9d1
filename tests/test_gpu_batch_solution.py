"""GPU: every LP's whole solution formed on the device (k_batch_solution) after each of the three
batch kernels, solve_batch_arrays(solution=True, tables=False), solve_batch_solutions and
SimplexMethod.solution() on the device backends -- against solution_util on the C oracle's final
tables and logs, by bit pattern."""
from __future__ import annotations

import random
from collections import Counter

import numpy as np
import pytest

import solution_util as su
import special_values as sv
from batch_util import OUTCOME, case, solve as _solve
from golden_util import dec_input, load

pytestmark = pytest.mark.gpu

TIERS = ("wave", "workgroup", "global")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def _run(members, cap, kernel, **kw):
    """members: [(kind, n, m, seed, flen)] -> (refs, solve_batch_arrays(solution=True) output)."""
    refs = [case(kind, n, m, seed, cap, flen) for kind, n, m, seed, flen in members]
    out = _solve([(r[0], n, m, flen) for r, (_, n, m, _, flen) in zip(refs, members)], cap,
                 kernel=kernel, solution=True, **kw)
    return refs, out


def _check(members, refs, out, what, nan_aware=False):
    for q, ((_, n, m, _, _), ref) in enumerate(zip(members, refs)):
        assert int(out["status"][q]) == ref[3], (what, q)
        su.same_arrays(out, q, n, m, su.of_case(ref, n, m), (what, q), nan_aware)


def test_the_inputs_keep_their_edge():
    su.check_sharp_cases()


# ----------------------------------------------------------------------------------------------
# wave tier
WAVE_MIX = [("uniform", 3, 2, 0, 2), ("uniform", 5, 1, 0, 1), ("uniform", 63, 63, 0, 63),
            ("mixed", 20, 20, 0, 20), ("uniform", 40, 7, 1, 8), ("mixed", 9, 33, 2, 33)]


def test_wave_mixed_shapes_in_one_launch():
    """3 x 2 (optimum after one pivot), m == 1, 63 x 63 (the whole envelope), the sharp
    20 x 20 and two more shapes in one [6][64][64] launch: every LP's own n, m inside the
    padding."""
    refs, out = _run(WAVE_MIX, 64, "wave")
    assert (OUTCOME[refs[0][3]], refs[0][4]) == ("optimum", 1)
    assert out["x"].shape == (6, 63) and out["duals"].shape == (6, 63)
    assert out["basis"].shape == (6, 63) and out["nonbasis"].shape == (6, 63)
    assert out["objective"].shape == (6,) and out["final"].shape == (6, 64, 64)
    _check(WAVE_MIX, refs, out, "wave mix")
    assert su.replay(refs[3][5], 20, 20)[2] == su.SHARP[2][5]


@pytest.mark.parametrize("B", [1, 5, 257])
def test_wave_batch_sizes(B):
    """One LP, a block and a bit, and 65 blocks with the last one partly filled (four LPs per
    block), shapes cycling so that padding differs from neighbour to neighbour."""
    shapes = [("uniform", 3, 2), ("uniform", 7, 4), ("mixed", 6, 9), ("uniform", 12, 3)]
    members = [(*shapes[q % 4], q, shapes[q % 4][2]) for q in range(B)]
    refs, out = _run(members, 24, "wave")
    _check(members, refs, out, ("wave", B))
    if B == 257:
        assert len({OUTCOME[r[3]] for r in refs}) >= 2


# ----------------------------------------------------------------------------------------------
# workgroup tier
WG_LAUNCHES = {
    "65x65": ([("uniform", 65, 65, 0, 65), ("uniform", 65, 65, 1, 66)], 1024),
    "100x100": ([("uniform", 100, 100, 0, 100), ("uniform", 100, 100, 1, 100)], 256),
    "300x40": ([("uniform", 300, 40, 0, 40)], 1024),
    "40x300": ([("uniform", 40, 300, 0, 300)], 1024),
}


@pytest.mark.parametrize("name", list(WG_LAUNCHES))
def test_workgroup_shapes(name):
    members, cap = WG_LAUNCHES[name]
    refs, out = _run(members, cap, "workgroup")
    _check(members, refs, out, name)
    if name == "100x100":
        assert [r[4] for r in refs] == [256, 256]            # both at the cap
        assert float(out["objective"][0]).hex() == su.SHARP_OBJECTIVE_0


def test_global_141_by_141():
    """One LP past the LDS edge, the table in global memory, at cap 64."""
    from simplex_mi355x.batch import wg_lds_bytes
    assert wg_lds_bytes(142, 142) < 0
    members = [("uniform", 141, 141, 0, 141)]
    refs, out = _run(members, 64, "global")
    assert refs[0][4] > 0
    _check(members, refs, out, "global 141")


# ----------------------------------------------------------------------------------------------
# all three tiers
def _edge(name):
    cons, func = dec_input(load("edge.json")[name]["input"])
    T = np.zeros((len(cons) + 1, len(cons[0])))
    T[:-1] = cons
    T[-1, :len(func)] = func
    return T, len(cons), len(cons[0]) - 1, len(func)


@pytest.fixture(scope="module")
def small_bag():
    """[(T, n, m, flen)] and each one's oracle answer at cap 16: a plain LP, len(function) ==
    m + 1, an LP that is optimal as it stands (no pivot), an `incorrect` and a `not_converge`
    edge fixture."""
    from oracle import c_oracle
    from simplex_mi355x import lp
    plain = lp.dense_tableau("uniform", 0, 6, 4)
    longf = lp.dense_tableau("uniform", 1, 5, 5)
    bag = [(plain, 6, 4, 4), (longf, 5, 5, 6), (np.abs(plain), 6, 4, 4),
           _edge("incorrect_system"), _edge("unbounded")]
    refs = []
    for T, n, m, flen in bag:
        Tref, st, done, log = c_oracle.run(T, n, m, flen, 16)
        refs.append((T, flen, Tref, st, done, log))
    assert [OUTCOME[r[3]] for r in refs][2:] == ["optimum", "incorrect", "not_converge"]
    assert refs[2][4] == 0 and refs[0][4] > 0 and refs[1][4] > 0
    return bag, refs


@pytest.mark.parametrize("kernel", TIERS)
def test_small_bag_through_each_tier(small_bag, kernel):
    bag, refs = small_bag
    out = _solve(bag, 16, kernel=kernel, solution=True)
    for q, ((T, n, m, flen), ref) in enumerate(zip(bag, refs)):
        assert int(out["status"][q]) == ref[3], (kernel, q)
        su.same_arrays(out, q, n, m, su.of_case(ref, n, m), (kernel, q))
    n, m = bag[2][1:3]                                       # no pivot: identity labels
    assert out["basis"][2, :n].tolist() == list(range(m, m + n))
    assert out["nonbasis"][2, :m].tolist() == list(range(m))


@pytest.mark.parametrize("kernel", TIERS)
def test_max_pivots_zero_gives_identity_labels(small_bag, kernel):
    bag, _ = small_bag
    out = _solve(bag, 0, kernel=kernel, solution=True)
    for q, (T, n, m, flen) in enumerate(bag):
        exp = su.expected(T, np.zeros((0, 2), dtype=np.int32), n, m, T[n])
        assert exp.basis.tolist() == list(range(m, m + n)) and not su.bits(exp.x).any()
        su.same_arrays(out, q, n, m, exp, (kernel, q))
        assert np.array_equal(su.bits(out["final"][q, :n + 1, :m + 1]), su.bits(T)), (kernel, q)


# (at 130 x 130 the NaN of nan_first reaches x on the workgroup tier too; at 100 x 100 it does not)
SPECIAL = {"wave": sv.WAVE[0], "workgroup": sv.WORKGROUP[1], "global": sv.GLOBAL[0]}


@pytest.mark.parametrize("name", ["nan_first", "inf_b"])
@pytest.mark.parametrize("kernel", TIERS)
def test_nan_and_inf_tables(kernel, name):
    """NaN positions follow the table, every other element by its bits (the signs of infs and
    zeros count)."""
    n, m, k = SPECIAL[kernel]
    T, Tref, st, done, log = sv.reference(name, n, m, sv.SEEDS[0], k)
    exp = su.expected(Tref, log, n, m, T[n])
    if name == "nan_first":                                  # a NaN x, so a NaN objective
        assert np.isnan(exp.x).any() and not np.isnan(exp.x).all() and np.isnan(exp.objective)
    else:                                                    # infs stay in rows labelled y:
        assert np.isinf(Tref).any() and np.isfinite(exp.x).all()   # x, duals finite beside them
    out = _solve([(T, n, m, m)], k, kernel=kernel, solution=True)
    assert int(out["npivots"][0]) == done == k
    su.same_arrays(out, 0, n, m, exp, (kernel, name), nan_aware=True)


# ----------------------------------------------------------------------------------------------
# the kernel alone, through the C ABI: corners the solvers never hand it
def test_kernel_contract_corners():
    """Hand-made inputs around the oracle's 20 x 20 table and log, padded to 23 x 24: inf, -inf,
    -0.0 and NaN in the entries that become x and duals, log entries outside r < n, c < m
    (skipped), npivots past max_pivots and below 0 (clamped), and dims outside the block (padding
    only, objective +0.0).  Every output starts poisoned, so an element left unwritten shows."""
    import torch
    from simplex_mi355x import _lib
    n = m = 20
    T, _, Tref, _, done, log = case("mixed", n, m, 0, 64, m)
    Rmax, ldb = 23, 24
    basis, nonbasis, _ = su.replay(log, n, m)
    poked = np.array(Tref)
    pool = [np.inf, -np.inf, -0.0, np.nan, 5e-324]
    for t, i in enumerate(np.nonzero(basis < m)[0]):
        poked[i, m] = pool[t % 5]
    for t, j in enumerate(np.nonzero(nonbasis >= m)[0]):
        poked[n, j] = pool[(t + 2) % 5]
    junk = np.array([[n, 0], [0, m], [-1, 3], [5, -2], [1000, 1000]], dtype=np.int32)
    mixed_log = np.concatenate([junk[:2], log[:10], junk[2:4], log[10:], junk[4:]])
    P = len(mixed_log)
    lps = [(Tref, log, done + 100, (n, m)), (poked, log, done, (n, m)),
           (Tref, mixed_log, P, (n, m)), (Tref, log, -5, (n, m)), (Tref, log, done, (Rmax + 5, 5)),
           (Tref, log, done, (n, ldb)), (Tref, log, done, (0, 3)), (Tref, log, done, (Rmax, m)),
           (Tref, log, done, (3, -1))]
    B = len(lps)
    final = np.zeros((B, Rmax, ldb))
    func = np.full((B, ldb), 9.0)
    rc = np.full((B, P, 2), 1 << 20, dtype=np.int32)
    npiv = np.zeros(B, dtype=np.int32)
    dims = np.zeros((B, 3), dtype=np.int32)
    for q, (tab, lg, cnt, (nn, mm)) in enumerate(lps):
        final[q, :n + 1, :m + 1] = tab
        func[q, :m] = T[n, :m]
        rc[q, :len(lg)] = lg
        npiv[q] = cnt
        dims[q] = (nn, mm, mm)
    dev = torch.device("cuda")
    d_in = [torch.from_numpy(a).to(dev) for a in (final, dims, rc, npiv, func)]
    d_x = torch.full((B, ldb), 7.0, dtype=torch.float64, device=dev)
    d_du = torch.full((B, Rmax), 7.0, dtype=torch.float64, device=dev)
    d_obj = torch.full((B,), 7.0, dtype=torch.float64, device=dev)
    d_ba = torch.full((B, Rmax), 12345, dtype=torch.int32, device=dev)
    d_nb = torch.full((B, ldb), 12345, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().smx_batch_solution(
        d_in[0].data_ptr(), d_in[1].data_ptr(), B, Rmax, ldb, P, d_in[2].data_ptr(),
        d_in[3].data_ptr(), d_in[4].data_ptr(), d_x.data_ptr(), d_du.data_ptr(), d_obj.data_ptr(),
        d_ba.data_ptr(), d_nb.data_ptr(), torch.cuda.current_stream().cuda_stream),
        "smx_batch_solution")
    out = {"x": d_x.cpu().numpy(), "duals": d_du.cpu().numpy(), "objective": d_obj.cpu().numpy(),
           "basis": d_ba.cpu().numpy(), "nonbasis": d_nb.cpu().numpy(), "npivots": npiv}
    exp_poked = su.expected(poked, log, n, m, T[n])
    assert np.isinf(exp_poked.x).any() and np.isnan(exp_poked.x).any()
    assert np.isinf(exp_poked.duals).any()
    assert np.signbit(exp_poked.duals[exp_poked.duals == 0]).any()             # a -0.0 dual
    wants = [su.expected(Tref, log, n, m, T[n])._replace(pivots=done + 100),
             exp_poked,
             su.expected(Tref, mixed_log, n, m, T[n]),
             su.expected(Tref, log[:0], n, m, T[n])._replace(pivots=-5)]
    assert np.array_equal(wants[2].basis, wants[0].basis)    # the junk entries change nothing
    for q, exp in enumerate(wants):
        su.same_arrays(out, q, n, m, exp, q, nan_aware=True)
    for q in range(len(wants), B):                           # outside the block: padding only
        assert (out["basis"][q] == -1).all() and (out["nonbasis"][q] == -1).all(), q
        assert not su.bits(out["x"][q]).any() and not su.bits(out["duals"][q]).any(), q
        assert su.same_floats(out["objective"][q], 0.0), q


# ----------------------------------------------------------------------------------------------
# the batch surface
@pytest.mark.parametrize("kernel", ["wave", "workgroup"])
def test_tables_false_returns_the_same_answer_without_the_tables(kernel):
    members = WAVE_MIX if kernel == "wave" else WG_LAUNCHES["100x100"][0]
    cap = 64 if kernel == "wave" else 256
    refs, full = _run(members, cap, kernel)
    _, lean = _run(members, cap, kernel, tables=False)
    assert "final" in full and "final" not in lean
    assert set(full) - {"final"} == set(lean)
    for key in ("status", "npivots", "rc", "basis", "nonbasis"):
        assert np.array_equal(full[key], lean[key]), key
    for key in ("x", "duals", "objective"):
        assert su.same_floats(full[key], lean[key]), key
    _check(members, refs, lean, ("tables=False", kernel))


def test_defaults_return_todays_dict():
    refs, out = _run(WAVE_MIX[:2], 64, "wave")
    plain = _solve([(r[0], n, m, flen) for r, (_, n, m, _, flen) in zip(refs, WAVE_MIX[:2])], 64,
                   kernel="wave")
    assert list(plain) == ["final", "rc", "xv", "status", "npivots"]
    assert list(out)[:5] == list(plain)


def test_solve_batch_solutions_routes_and_keeps_order():
    """Wave, workgroup, int-entry and IndexError problems shuffled into one call: the solutions
    come back in input order and equal SimplexMethod(...).solution(), problem by problem."""
    from simplex_mi355x import Solution
    from simplex_mi355x.batch import route, solve_batch_solutions
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
        T = case("uniform", 65, 65, s, 1024, 65 + s % 2)[0]
        probs.append((T[:65].tolist(), T[65, :65].tolist()))
    T = case("mixed", 20, 20, 0, 64, 20)[0]
    probs.append((T[:20].tolist(), T[20, :21].tolist()))                     # len(function) = m + 1
    probs.append(([[1, 2, -3], [2, 1, 4], [-1, 1, 2]], [-1, -2]))            # int entries
    probs.append(([[1.0, 2.0], [-2.0, 1.0]], [-1.0]))                          # IndexError
    random.Random(3).shuffle(probs)
    assert Counter(route(c, f) for c, f in probs) == {"wave": 7, "workgroup": 3, "single": 2}
    sols, statuses = solve_batch_solutions(probs, max_pivots=cap)
    assert len(sols) == len(probs)
    raised = 0
    for k, ((cons, func), got) in enumerate(zip(probs, sols)):
        try:
            sm = simplex.SimplexMethod([list(r) for r in cons], list(func))
            sm.solve(record_history=False, max_pivots=cap)
            exp = sm.solution()
        except IndexError:
            assert isinstance(got, IndexError) and statuses[k] == "exception"
            raised += 1
            continue
        assert isinstance(got, Solution) and sm.backend == "hip"
        assert got.x.shape == (len(cons[0]) - 1,) and got.duals.shape == (len(cons),)
        su.same_solution(got, su.Expected(*exp), k)
        assert statuses[k] == sm.status, k
    assert raised == 1
    assert {"optimum", "cap", "error"} <= set(statuses)


def test_simplexmethod_solution_on_device_backends_equals_host():
    """One 40 x 30 LP: the HIP backend and two row shards on device 0 against the host engine,
    and all of them against the C oracle's table."""
    from oracle import c_oracle
    from simplex_mi355x import lp
    import simplex
    n, m, cap = 40, 30, 60
    T = lp.dense_tableau("uniform", 3, n, m)
    Tref, st, done, log = c_oracle.run(T, n, m, m, cap)
    assert done > 5 and su.replay(log, n, m)[2] > 0
    exp = su.expected(Tref, log, n, m, T[n])
    sols = {}
    for name, kw in (("host", {"device": "cpu"}), ("hip", {}), ("sharded", {"devices": [0, 0]})):
        sm = simplex.SimplexMethod(T[:n].tolist(), T[n, :m].tolist(), **kw)
        assert sm.backend == name
        first = sm.solution()                                # the pristine table: all zeros
        assert not su.bits(first.x).any() and not su.bits(first.duals).any()
        sm.solve(record_history=False, max_pivots=cap)
        sols[name] = sm.solution()
        su.same_solution(sols[name], exp, name)
    for name in ("hip", "sharded"):
        su.same_solution(sols[name], su.Expected(*sols["host"]), name)
