"""GPU: every LP's sensitivity ranges formed on the device (k_batch_ranging) after each of the
three batch kernels, solve_batch_arrays(solution=True, ranging=True), the kernel alone through the
C ABI at its tile and wave edges and on the hand-made tables, solve_batch_ranges and
SimplexMethod.ranging() on the device backend -- against ranging_util on the C oracle's final
tables and logs, by bit pattern."""
from __future__ import annotations

import random
from collections import Counter

import numpy as np
import pytest

import ranging_util as ru
import solution_util as su
import special_values as sv
from batch_util import case, solve as _solve

pytestmark = pytest.mark.gpu

# The launches of test_gpu_batch_solution.py: (kind, n, m, seed, flen).
WAVE_MIX = [("uniform", 3, 2, 0, 2), ("uniform", 5, 1, 0, 1), ("uniform", 63, 63, 0, 63),
            ("mixed", 20, 20, 0, 20), ("uniform", 40, 7, 1, 8), ("mixed", 9, 33, 2, 33)]
WG_LAUNCHES = {
    "65x65": ([("uniform", 65, 65, 0, 65), ("uniform", 65, 65, 1, 66)], 1024),
    "100x100": ([("uniform", 100, 100, 0, 100), ("uniform", 100, 100, 1, 100)], 256),
    "300x40": ([("uniform", 300, 40, 0, 40)], 1024),
    "40x300": ([("uniform", 40, 300, 0, 300)], 1024),
}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def _run(members, cap, kernel, **kw):
    """members: [(kind, n, m, seed, flen)] -> (refs, solve_batch_arrays(ranging=True) output)."""
    refs = [case(kind, n, m, seed, cap, flen) for kind, n, m, seed, flen in members]
    out = _solve([(r[0], n, m, flen) for r, (_, n, m, _, flen) in zip(refs, members)], cap,
                 kernel=kernel, solution=True, ranging=True, **kw)
    return refs, out


def _check(members, refs, out, what, nan_aware=False):
    for q, ((_, n, m, _, _), ref) in enumerate(zip(members, refs)):
        assert int(out["status"][q]) == ref[3], (what, q)
        su.same_arrays(out, q, n, m, su.of_case(ref, n, m), (what, q), nan_aware)
        ru.same_arrays(out, q, n, m, ru.of_case(ref, n, m), (what, q), nan_aware)


def test_the_inputs_keep_their_edge():
    ru.check_sharp_cases()


# ----------------------------------------------------------------------------------------------
# wave tier
def test_wave_mixed_shapes_in_one_launch():
    refs, out = _run(WAVE_MIX, 64, "wave")
    assert out["rhs_lo"].shape == out["rhs_hi"].shape == (6, 63)
    assert out["cost_lo"].shape == out["cost_hi"].shape == (6, 63)
    assert out["final"].shape == (6, 64, 64)
    _check(WAVE_MIX, refs, out, "wave mix")


@pytest.mark.parametrize("B", [1, 5, 257])
def test_wave_batch_sizes(B):
    shapes = [("uniform", 3, 2), ("uniform", 7, 4), ("mixed", 6, 9), ("uniform", 12, 3)]
    members = [(*shapes[q % 4], q, shapes[q % 4][2]) for q in range(B)]
    refs, out = _run(members, 24, "wave")
    _check(members, refs, out, ("wave", B))


# ----------------------------------------------------------------------------------------------
# workgroup and global tiers
@pytest.mark.parametrize("name", list(WG_LAUNCHES))
def test_workgroup_shapes(name):
    """65 x 65 and 100 x 100 (two tiles, rows past every wave's first pass), 300 x 40 (75 rows a
    wave) and 40 x 300 (five tiles, past one workgroup's width)."""
    members, cap = WG_LAUNCHES[name]
    refs, out = _run(members, cap, "workgroup")
    _check(members, refs, out, name)
    if name == "100x100":
        basis = su.replay(refs[0][5], 100, 100)[0]
        exp = ru.of_case(refs[0], 100, 100)
        assert (int((basis < 100).sum()), ru.census(exp)) == ru.COUNTS[100, 100]


def test_global_141_by_141():
    members = [("uniform", 141, 141, 0, 141)]
    refs, out = _run(members, 64, "global")
    assert refs[0][4] > 0
    _check(members, refs, out, "global 141")


def test_mixed_dims_in_one_workgroup_launch():
    """dims differ from LP to LP inside one [4][101][101] launch: every LP's own n, m and tile
    count inside the padding."""
    members = [("uniform", 100, 100, 0, 100), ("uniform", 40, 7, 1, 7), ("uniform", 65, 65, 1, 65),
               ("mixed", 9, 33, 2, 33)]
    refs, out = _run(members, 256, "workgroup")
    assert out["rhs_lo"].shape == (4, 100) and out["cost_hi"].shape == (4, 100)
    _check(members, refs, out, "mixed dims")


@pytest.mark.parametrize("kernel", ["wave", "workgroup"])
def test_tables_false_returns_the_same_ranges_without_the_tables(kernel):
    members = WAVE_MIX if kernel == "wave" else WG_LAUNCHES["100x100"][0]
    cap = 64 if kernel == "wave" else 256
    refs, full = _run(members, cap, kernel)
    _, lean = _run(members, cap, kernel, tables=False)
    assert "final" in full and "final" not in lean
    assert set(full) - {"final"} == set(lean)
    for key in ru.FIELDS:
        assert su.same_floats(full[key], lean[key]), key
    _check(members, refs, lean, ("tables=False", kernel))


def test_defaults_return_todays_dict():
    refs = [case(kind, n, m, seed, 64, flen) for kind, n, m, seed, flen in WAVE_MIX[:2]]
    cases = [(r[0], n, m, flen) for r, (_, n, m, _, flen) in zip(refs, WAVE_MIX[:2])]
    assert list(_solve(cases, 64, kernel="wave")) == ["final", "rc", "xv", "status", "npivots"]
    sol = _solve(cases, 64, kernel="wave", solution=True)
    assert not set(ru.FIELDS) & set(sol)
    rng = _solve(cases, 64, kernel="wave", solution=True, ranging=True)
    assert list(rng) == list(sol) + list(ru.FIELDS)


@pytest.mark.parametrize("name", ["nan_first", "inf_b", "cols150"])
def test_special_value_tables(name):
    """NaN positions follow the table, every other element by its bits."""
    n, m, k = sv.WORKGROUP[0]
    assert (n, m) == (100, 100)
    T, Tref, st, done, log = sv.reference(name, n, m, sv.SEEDS[0], k)
    basis, nonbasis, _ = su.replay(log, n, m)
    exp = ru.expected(Tref, basis, nonbasis, n, m)
    flat = np.concatenate(exp)
    if name == "nan_first":
        assert np.isnan(flat).any() and not np.isnan(flat).all()
    elif name == "cols150":
        assert np.isfinite(flat).any() and (np.abs(flat[np.isfinite(flat)]) > 2.0 ** 100).any()
    out = _solve([(T, n, m, m)], k, kernel="workgroup", solution=True, ranging=True)
    assert int(out["npivots"][0]) == done == k
    ru.same_arrays(out, 0, n, m, exp, name, nan_aware=True)


# ----------------------------------------------------------------------------------------------
# the kernel alone, through the C ABI
def _launch(lps, Rmax, ldb):
    """lps: [(T, n, m, basis, nonbasis)], or None for an LP whose dims (Rmax, ldb) lie outside the
    block, over a table of ones -> the four raw outputs ([B][Rmax] / [B][ldb]) of one
    smx_batch_ranging launch.  Every output starts poisoned, so an element left unwritten shows;
    the labels past n / m are -1 as k_batch_solution leaves them."""
    import torch
    from simplex_mi355x import _lib
    B = len(lps)
    final = np.zeros((B, Rmax, ldb))
    dims = np.zeros((B, 3), dtype=np.int32)
    ba = np.full((B, Rmax), -1, dtype=np.int32)
    nb = np.full((B, ldb), -1, dtype=np.int32)
    for q, lp_ in enumerate(lps):
        if lp_ is None:
            final[q], dims[q], ba[q], nb[q] = 1.0, (Rmax, ldb, ldb), 0, 1
            continue
        T, n, m, basis, nonbasis = lp_
        final[q, :n + 1, :m + 1] = np.asarray(T)[:n + 1, :m + 1]
        dims[q] = (n, m, m)
        ba[q, :n] = basis
        nb[q, :m] = nonbasis
    dev = torch.device("cuda")
    d_in = [torch.from_numpy(a).to(dev) for a in (final, dims, ba, nb)]
    d_out = [torch.full((B, w), 7.0, dtype=torch.float64, device=dev)
             for w in (Rmax, Rmax, ldb, ldb)]
    _lib.check(_lib.load().smx_batch_ranging(
        d_in[0].data_ptr(), d_in[1].data_ptr(), B, Rmax, ldb, d_in[2].data_ptr(),
        d_in[3].data_ptr(), *(t.data_ptr() for t in d_out),
        torch.cuda.current_stream().cuda_stream), "smx_batch_ranging")
    return dict(zip(ru.FIELDS, (t.cpu().numpy() for t in d_out)))


EDGES = [(63, 63), (64, 64), (5, 255), (5, 256), (5, 257), (257, 3), (1, 1), (1, 8189), (8189, 1)]


@pytest.mark.parametrize("n,m", EDGES, ids=[f"{n}x{m}" for n, m in EDGES])
def test_tile_and_wave_edges(n, m):
    """A seeded table under a seeded permutation of the labels, no solve: the last tile full, one
    short of it and one past it, rows one past a wave's stride, the smallest LP and the two ends of
    the envelope's sum bound.  Every output slot is compared, the padding too."""
    from simplex_mi355x import lp
    T = lp.dense_tableau("uniform", 3, n, m)
    basis, nonbasis = ru.seeded_labels(n, m, 3)
    assert (basis < m).any() or n == 1 or m == 1
    exp = ru.expected(T, basis, nonbasis, n, m)
    out = _launch([(T, n, m, basis, nonbasis)], n + 1, m + 1)
    ru.same_arrays(out, 0, n, m, exp, (n, m))
    err, host = ru.host(T, n, m, basis, nonbasis)
    assert err == 0
    ru.same_ranges(host, exp, (n, m, "host"))


def test_handmade_tables_through_the_kernel():
    """The hand-made tables of the CPU test as LP 0, 1 and 4 of five-LP launches (the LPs between
    are a seeded table and an LP whose dims lie outside the block): the kernel against
    smx_host_ranging and ranging_util, by bit pattern."""
    from simplex_mi355x import lp
    cases = ru.handmade()
    fill = lp.dense_tableau("uniform", 1, 8, 6)
    fb, fn = ru.seeded_labels(8, 6, 1)
    Rmax, ldb = 11, 9
    assert all(c[2] < Rmax and c[3] < ldb for c in cases)
    while len(cases) % 3:
        cases.append(cases[0])
    for g in range(0, len(cases), 3):
        trio = cases[g:g + 3]
        lps = [trio[0][1:6], trio[1][1:6], (fill, 8, 6, fb, fn), None, trio[2][1:6]]
        out = _launch(lps, Rmax, ldb)
        for q, (name, T, n, m, basis, nonbasis, pins) in zip((0, 1, 4), trio):
            got = ru.Expected(*(out[f][q, :(n if f.startswith("rhs") else m)]
                                for f in ru.FIELDS))
            ru.check_handmade(name, got, T, n, m, basis, nonbasis, pins)
            err, host = ru.host(T, n, m, basis, nonbasis)
            assert err == 0
            ru.same_ranges(got, host, (name, "host"))
            ru.same_arrays(out, q, n, m, host, name)
        ru.same_arrays(out, 2, 8, 6, ru.expected(fill, fb, fn, 8, 6), "fill")
        for f in ru.FIELDS:                                  # outside the block: padding only
            assert not su.bits(out[f][3]).any(), (f, "outside")


# ----------------------------------------------------------------------------------------------
# the list-level call and SimplexMethod
def test_solve_batch_ranges_routes_and_keeps_order():
    """Wave, workgroup, int-entry and IndexError problems shuffled into one call: each Ranging
    equals SimplexMethod(...).ranging() of the same problem, the statuses those of
    solve_batch_solutions."""
    from simplex_mi355x import Ranging
    from simplex_mi355x.batch import route, solve_batch_ranges, solve_batch_solutions
    import simplex
    cap = 24
    rng = np.random.default_rng(7)
    probs = []
    for _ in range(6):
        A = rng.uniform(-50, 50, size=(3, 2))
        b = rng.uniform(-100, 400, size=3)
        probs.append(([list(map(float, A[i])) + [float(b[i])] for i in range(3)],
                      list(map(float, rng.uniform(-3, 3, size=2)))))
    for s in range(2):
        T = case("uniform", 65, 65, s, 1024, 65)[0]
        probs.append((T[:65].tolist(), T[65, :65].tolist()))
    probs.append(([[1, 2, -3], [2, 1, 4], [-1, 1, 2]], [-1, -2]))            # int entries
    probs.append(([[1.0, 2.0], [-2.0, 1.0]], [-1.0]))                          # IndexError
    random.Random(3).shuffle(probs)
    assert Counter(route(c, f) for c, f in probs) == {"wave": 6, "workgroup": 2, "single": 2}
    ranges, statuses = solve_batch_ranges(probs, max_pivots=cap)
    assert statuses == solve_batch_solutions(probs, max_pivots=cap)[1]
    raised = 0
    for k, ((cons, func), got) in enumerate(zip(probs, ranges)):
        try:
            sm = simplex.SimplexMethod([list(r) for r in cons], list(func))
            sm.solve(record_history=False, max_pivots=cap)
        except IndexError:
            assert isinstance(got, IndexError) and statuses[k] == "exception"
            raised += 1
            continue
        assert isinstance(got, Ranging) and sm.backend == "hip"
        assert got.rhs_lo.shape == (len(cons),) and got.cost_hi.shape == (len(cons[0]) - 1,)
        ru.same_ranges(got, sm.ranging(), k)
    assert raised == 1 and {"optimum", "cap"} <= set(statuses)


def test_simplexmethod_ranging_on_the_device_equals_the_batch():
    import simplex
    members = [("uniform", 100, 100, 0, 100)]
    refs, out = _run(members, 256, "workgroup")
    T = refs[0][0]
    sm = simplex.SimplexMethod(T[:100].tolist(), T[100, :100].tolist())
    assert sm.backend == "hip"
    sm.solve(record_history=False, max_pivots=256)
    got = sm.ranging()
    ru.same_ranges(got, ru.of_case(refs[0], 100, 100), "device")
    ru.same_arrays(out, 0, 100, 100, got, "batch")
