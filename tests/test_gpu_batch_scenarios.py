"""GPU: what-if scenarios on the device -- k_batch_scenario alone through the C ABI at its tile and
wave edges and on the hand-made tables, the whole chain of solve_batch_scenarios_arrays on all
three tiers, smx_batch_solution_from alone, solve_batch_scenarios and SimplexMethod.what_if on the
device backend -- against scenario_util's restatement on the C oracle's final tables and the
oracle's warm runs on the restated scenario tables, by bit pattern."""
from __future__ import annotations

import numpy as np
import pytest

import ranging_util as ru
import scenario_util as scu
import solution_util as su
import special_values as sv
from batch_util import case, solve as _solve

pytestmark = pytest.mark.gpu

FRAC, PROB = 0.05, 0.25
KEYS = ("x", "duals", "objective", "basis", "nonbasis", "npivots")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


# ----------------------------------------------------------------------------------------------
# the kernel alone, through the C ABI
GUARD = 64


def _guarded(torch, count, dtype, poison):
    """A device buffer of `count` elements between two poisoned guard bands -> (whole, view)."""
    whole = torch.full((count + 2 * GUARD,), poison, dtype=dtype, device="cuda")
    return whole, whole[GUARD:GUARD + count]


def _launch(lps, S, Rmax, ldb, deltas):
    """lps: [(T, n, m, basis, nonbasis, function)], or None for an LP whose dims (Rmax, ldb) lie
    outside the block; deltas[q][s] = (drhs [n], dcost [m]) -> (tabs_s [B*S][Rmax][ldb], func_s
    [B*S][ldb], dims_s [B*S][3], final, dims) of one smx_batch_scenario launch.  The padding of
    every base block holds a value that shows, every output starts poisoned and stands between
    poisoned guard bands that must come back untouched."""
    import torch
    from simplex_mi355x import _lib
    B = len(lps)
    final = np.full((B, Rmax, ldb), 3.25)
    dims = np.zeros((B, 3), dtype=np.int32)
    ba = np.full((B, Rmax), -1, dtype=np.int32)
    nb = np.full((B, ldb), -1, dtype=np.int32)
    func = np.full((B, ldb), 11.0)
    dr = np.full((B, S, Rmax), 5.0)                          # past n / m: never read
    dc = np.full((B, S, ldb), 5.0)
    for q, lp_ in enumerate(lps):
        if lp_ is None:
            dims[q], ba[q], nb[q] = (Rmax, ldb, ldb), 0, 1
            continue
        T, n, m, basis, nonbasis, function = lp_
        final[q, :n + 1, :m + 1] = np.asarray(T)[:n + 1, :m + 1]
        dims[q] = (n, m, m)
        ba[q, :n] = basis
        nb[q, :m] = nonbasis
        func[q, :m] = np.asarray(function)[:m]
        for s in range(S):
            dr[q, s, :n], dc[q, s, :m] = deltas[q][s]
    d_in = [torch.from_numpy(a).to("cuda") for a in (final, dims, ba, nb, func, dr, dc)]
    Q = B * S
    w_t, d_t = _guarded(torch, Q * Rmax * ldb, torch.float64, 7.0)
    w_f, d_f = _guarded(torch, Q * ldb, torch.float64, 7.0)
    w_d, d_d = _guarded(torch, Q * 3, torch.int32, 77)
    _lib.check(_lib.load().smx_batch_scenario(
        d_in[0].data_ptr(), d_in[1].data_ptr(), B, S, Rmax, ldb, d_in[2].data_ptr(),
        d_in[3].data_ptr(), d_in[4].data_ptr(), d_in[5].data_ptr(), d_in[6].data_ptr(),
        d_t.data_ptr(), d_f.data_ptr(), d_d.data_ptr(),
        torch.cuda.current_stream().cuda_stream), "smx_batch_scenario")
    for whole, poison in ((w_t, 7.0), (w_f, 7.0), (w_d, 77)):
        h = whole.cpu().numpy()
        assert (h[:GUARD] == poison).all() and (h[-GUARD:] == poison).all(), "guard band"
    return (d_t.cpu().numpy().reshape(Q, Rmax, ldb), d_f.cpu().numpy().reshape(Q, ldb),
            d_d.cpu().numpy().reshape(Q, 3), final, dims)


def _same_block(got, base, S_exp, n, m, what, nan_aware=False):
    """One whole Rmax x ldb output block: the base block's bits with rows 0..n, columns 0..m
    replaced by the expected scenario table."""
    exp = base.copy()
    exp[:n + 1, :m + 1] = S_exp
    if nan_aware:
        assert su.same_floats(got, exp, True), what
    else:
        scu.same_table(got, exp, what)


EDGES = [(63, 63, 3), (64, 64, 1), (65, 65, 3), (5, 255, 3), (5, 256, 1), (5, 257, 3), (257, 3, 3),
         (1, 1, 3), (1, 8189, 1), (8189, 1, 1)]


@pytest.mark.parametrize("n,m,S", EDGES, ids=[f"{n}x{m}-S{S}" for n, m, S in EDGES])
def test_tile_and_wave_edges(n, m, S):
    """Two seeded tables under seeded permutations of the labels, no solve, S scenarios each: a
    tile of 64 columns / a block of 64 rows full, one short of it and one past it, rows and
    columns one past a workgroup's stride of 256, the smallest LP and the two ends of the
    envelope's sum bound.  Every output element is compared, the padding too."""
    from simplex_mi355x import lp
    lps, deltas, exp = [], [], []
    for q in range(2):
        T = lp.dense_tableau("uniform", 3 + q, n, m)
        basis, nonbasis = ru.seeded_labels(n, m, 3 + q)
        lps.append((T, n, m, basis, nonbasis, T[n, :m]))
        deltas.append([scu.deltas(T, n, m, 3 + q, s, 0.5, 0.5) for s in range(S)])
        exp.append([scu.restate(T, n, m, basis, nonbasis, T[n, :m], *deltas[q][s])
                    for s in range(S)])
    assert any((d != 0).any() for ds in deltas for pair in ds for d in pair)
    wide = n + m + 5 <= 8192                                 # padding where the envelope has room
    tabs_s, func_s, dims_s, final, dims = _launch(lps, S, n + 1 + wide, m + 1 + 2 * wide, deltas)
    for q in range(2):
        for s in range(S):
            k = q * S + s
            _same_block(tabs_s[k], final[q], exp[q][s][0], n, m, (n, m, q, s))
            assert su.same_floats(func_s[k, :m], exp[q][s][1]), (n, m, q, s, "func_s")
            assert not su.bits(func_s[k, m:]).any(), (n, m, q, s, "func_s padding")
            assert dims_s[k].tolist() == dims[q].tolist()
            err, host, fhost = scu.host(lps[q][0], n, m, lps[q][3], lps[q][4], lps[q][5],
                                        *deltas[q][s])
            assert err == 0
            scu.same_table(host, exp[q][s][0], (n, m, q, s, "host"))


HANDMADE = scu.handmade()


@pytest.mark.parametrize("hm", HANDMADE, ids=[c[0] for c in HANDMADE])
def test_handmade_tables_on_the_device(hm):
    """Each hand-made table as LP 0, 1 and 4 of a five-LP launch (LP 2 has dims outside the
    block, LP 3 is a plain table without deltas), against smx_host_scenario."""
    name, T, n, m, basis, nonbasis, func, dr, dc, _ = hm
    err, S_host, f_host = scu.host(T, n, m, basis, nonbasis, func, dr, dc)
    assert err == 0
    scu.check_handmade(hm, S_host, f_host)
    mine = (T, n, m, basis, nonbasis, func)
    plain = (np.ones((n + 1, m + 1)), n, m, basis, nonbasis, func)
    lps = [mine, mine, None, plain, mine]
    deltas = [[(dr, dc)], [(dr, dc)], None, [(np.zeros(n), np.zeros(m))], [(dr, dc)]]
    tabs_s, func_s, dims_s, final, dims = _launch(lps, 1, n + 1, m + 1, deltas)
    for q in (0, 1, 4):
        assert su.same_floats(tabs_s[q], S_host, nan_aware=True), (name, q)
        assert su.same_floats(func_s[q, :m], f_host, nan_aware=True), (name, q)
    if name == "all zero":
        assert np.array_equal(su.bits(tabs_s[0]), su.bits(final[0]))
    assert np.array_equal(su.bits(tabs_s[2]), su.bits(final[2]))        # dims outside: a copy
    assert not su.bits(func_s[2]).any()
    assert np.array_equal(su.bits(tabs_s[3]), su.bits(final[3]))
    assert np.array_equal(dims_s, dims)


# ----------------------------------------------------------------------------------------------
# the whole chain
def _chain(members, cap, kernel, S, frac=FRAC, prob=PROB, warm=None, ranging=True, tables=None,
           delta_tables=None, nan_aware=False):
    """members: [(kind, n, m, seed, flen)] (or `tables`: [(T, Tref, st, done, log)] of
    special_values.reference for them) -> one solve_batch_scenarios_arrays launch, checked against
    the oracle: the base answers, and per scenario the oracle's warm run on the restated table."""
    from oracle import c_oracle
    from simplex_mi355x.batch import solve_batch_scenarios_arrays
    if tables is None:
        refs = [case(kind, n, m, seed, cap, flen) for kind, n, m, seed, flen in members]
    else:
        refs = [(T, flen, Tref, st, done, log)
                for (T, Tref, st, done, log), (_, _, _, _, flen) in zip(tables, members)]
    B = len(members)
    Rmax = max(n for _, n, _, _, _ in members) + 1
    ldb = max(m for _, _, m, _, _ in members) + 1
    tabs = np.zeros((B, Rmax, ldb))
    dims = np.zeros((B, 3), dtype=np.int32)
    drhs = np.zeros((B, S, Rmax - 1))
    dcost = np.zeros((B, S, ldb - 1))
    for q, ((_, n, m, seed, flen), ref) in enumerate(zip(members, refs)):
        tabs[q, :n + 1, :m + 1] = ref[0]
        dims[q] = (n, m, flen)
        src = ref[0] if delta_tables is None else delta_tables[q]
        for s in range(S):
            drhs[q, s, :n], dcost[q, s, :m] = scu.deltas(src, n, m, seed, s, frac, prob)
    capw = cap if warm is None else warm
    out = solve_batch_scenarios_arrays(tabs, dims, drhs, dcost, cap, warm, kernel=kernel,
                                       ranging=ranging)
    base = out["base"]
    stats = {"warm_pivots": 0, "status": []}
    for q, ((_, n, m, seed, flen), ref) in enumerate(zip(members, refs)):
        what = (kernel, q, n, m)
        assert int(base["status"][q]) == ref[3], what
        su.same_arrays(base, q, n, m, su.of_case(ref, n, m), what, nan_aware)
        if ranging:
            ru.same_arrays(base, q, n, m, ru.of_case(ref, n, m), what, nan_aware)
        basis, nonbasis, _ = su.replay(ref[5], n, m)
        for s in range(S):
            S_tab, func_s = scu.restate(ref[2], n, m, basis, nonbasis, ref[0][n, :m],
                                        drhs[q, s, :n], dcost[q, s, :m])
            Tw, wst, wdone, wlog = c_oracle.run(S_tab, n, m, flen, capw)
            wb, wn = scu.warm_labels(basis, nonbasis, wlog, n, m)
            assert int(out["status"][q, s]) == wst, (what, s, "status")
            view = {key: out[key][:, s] for key in KEYS}
            su.same_arrays(view, q, n, m,
                           scu.expected_solution(Tw, wb, wn, n, m, func_s, wdone), (what, s),
                           nan_aware)
            if ranging:
                ru.same_arrays({key: out[key][:, s] for key in ru.FIELDS}, q, n, m,
                               ru.expected(Tw, wb, wn, n, m), (what, s), nan_aware)
            stats["warm_pivots"] += wdone
            stats["status"].append(wst)
    return out, stats


WAVE_MIX = [("uniform", 3, 2, 0, 2), ("uniform", 40, 7, 1, 8), ("uniform", 63, 63, 0, 63),
            ("mixed", 20, 20, 0, 20)]


def test_wave_mixed_shapes_in_one_launch():
    out, stats = _chain(WAVE_MIX, 64, "wave", 3)
    assert out["status"].shape == (4, 3) and out["x"].shape == (4, 3, 63)
    assert out["duals"].shape == (4, 3, 63) and out["rhs_lo"].shape == (4, 3, 63)
    assert stats["warm_pivots"] > 0


def test_wave_larger_deltas_move_the_basis():
    """frac 0.5 on half the entries: most warm runs pivot, some end at an error status."""
    _, stats = _chain(WAVE_MIX, 64, "wave", 3, frac=0.5, prob=0.5)
    assert stats["warm_pivots"] > 0


@pytest.mark.parametrize("B,S", [(1, 1), (5, 3), (257, 1)])
def test_batch_sizes(B, S):
    shapes = [("uniform", 3, 2), ("uniform", 7, 4), ("mixed", 6, 9), ("uniform", 12, 3)]
    members = [(*shapes[q % 4], q, shapes[q % 4][2]) for q in range(B)]
    _chain(members, 24, "wave", S, frac=0.5, prob=0.5)


def test_workgroup_65_by_65():
    members = [("uniform", 65, 65, 0, 65), ("uniform", 65, 65, 1, 66)]
    out, stats = _chain(members, 1024, "workgroup", 3)
    assert int(out["base"]["npivots"][0]) == 502


def test_workgroup_100_by_100_from_a_capped_base_run():
    """The base run ends at the cap of 256: its table is still an equivalent form of its LP and
    the contract holds there."""
    members = [("uniform", 100, 100, 0, 100), ("uniform", 100, 100, 1, 100)]
    out, _ = _chain(members, 256, "workgroup", 3)
    assert (out["base"]["status"] == 0).all() and (out["base"]["npivots"] == 256).all()


def test_global_141_by_141():
    out, _ = _chain([("uniform", 141, 141, 0, 141)], 64, "global", 3)
    assert int(out["base"]["npivots"][0]) > 0


def test_a_separate_warm_cap():
    _, stats = _chain(WAVE_MIX, 64, "wave", 2, frac=0.5, prob=0.5, warm=3, ranging=False)
    assert 0 in stats["status"]                              # a warm run stopped by its own cap


@pytest.mark.parametrize("name", ["nan_first", "inf_b"])
def test_special_value_tables(name):
    """NaN positions follow the oracle, every other element by its bits; the deltas are sized on
    the clean table of the same seed (a NaN or inf mean would make every delta NaN)."""
    from simplex_mi355x import lp
    n, m, k = sv.WORKGROUP[0]
    ref = sv.reference(name, n, m, sv.SEEDS[0], k)
    clean = lp.dense_tableau("uniform", sv.SEEDS[0], n, m)
    _chain([("uniform", n, m, sv.SEEDS[0], m)], k, "workgroup", 2, tables=[ref],
           delta_tables=[clean], nan_aware=True)


def test_slices_of_scenarios_give_the_same_answer(monkeypatch):
    """A table budget that holds two scenarios of the launch at a time: three slices of S = 5."""
    from simplex_mi355x import batch
    whole, _ = _chain(WAVE_MIX, 64, "wave", 5, frac=0.5, prob=0.5)
    monkeypatch.setattr(batch, "GM_TABLE_BUDGET", 2 * 4 * 64 * 64 * 8)
    sliced, _ = _chain(WAVE_MIX, 64, "wave", 5, frac=0.5, prob=0.5)
    for key in whole:
        if key != "base":
            assert su.same_floats(whole[key], sliced[key]) if whole[key].dtype == np.float64 \
                else np.array_equal(whole[key], sliced[key]), key


# ----------------------------------------------------------------------------------------------
# smx_batch_solution_from alone
def _solution_from(out, dims, Rmax, ldb, cap, func, basis0, nonbasis0, group):
    import torch
    from simplex_mi355x import _lib
    B = len(dims)
    d = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
         for a in (out["final"], dims, out["rc"], out["npivots"], func, basis0, nonbasis0)]
    o = [torch.full((B, ldb), 7.0, dtype=torch.float64, device="cuda"),
         torch.full((B, Rmax), 7.0, dtype=torch.float64, device="cuda"),
         torch.full((B,), 7.0, dtype=torch.float64, device="cuda"),
         torch.full((B, Rmax), 77, dtype=torch.int32, device="cuda"),
         torch.full((B, ldb), 77, dtype=torch.int32, device="cuda")]
    _lib.check(_lib.load().smx_batch_solution_from(
        d[0].data_ptr(), d[1].data_ptr(), B, Rmax, ldb, cap, d[2].data_ptr(), d[3].data_ptr(),
        d[4].data_ptr(), d[5].data_ptr(), d[6].data_ptr(), group, *(t.data_ptr() for t in o),
        torch.cuda.current_stream().cuda_stream), "smx_batch_solution_from")
    x, du, obj, ba, nb = (t.cpu().numpy() for t in o)
    return {"x": x[:, :ldb - 1], "duals": du[:, :Rmax - 1], "objective": obj,
            "basis": ba[:, :Rmax - 1], "nonbasis": nb[:, :ldb - 1]}, (x, du, ba, nb)


def test_solution_from_identity_labels_is_smx_batch_solution():
    """Identity start labels reproduce smx_batch_solution bit for bit: per LP (group = 1, mixed
    dims) and one start row shared by a whole launch of equal dims (group = B)."""
    members = WAVE_MIX
    refs = [case(kind, n, m, seed, 64, flen) for kind, n, m, seed, flen in members]
    out = _solve([(r[0], n, m, flen) for r, (_, n, m, _, flen) in zip(refs, members)], 64,
                 kernel="wave", solution=True)
    dims = np.array([(n, m, flen) for _, n, m, _, flen in members], dtype=np.int32)
    func = np.zeros((4, 64))
    b0 = np.full((4, 64), -1, dtype=np.int32)
    n0 = np.full((4, 64), -1, dtype=np.int32)
    for q, ((_, n, m, _, _), ref) in enumerate(zip(members, refs)):
        func[q, :m + 1] = ref[0][n]
        b0[q, :n] = np.arange(m, m + n)
        n0[q, :m] = np.arange(m)
    got, _ = _solution_from(out, dims, 64, 64, 64, func, b0, n0, 1)
    for key in got:
        assert np.array_equal(got[key].view(np.int64) if got[key].dtype == np.float64
                              else got[key], out[key].view(np.int64)
                              if out[key].dtype == np.float64 else out[key]), key
    same = [("mixed", 20, 20, s, 20) for s in range(4)]
    refs = [case(kind, n, m, seed, 64, flen) for kind, n, m, seed, flen in same]
    out = _solve([(r[0], 20, 20, 20) for r in refs], 64, kernel="wave", solution=True)
    dims = np.array([(20, 20, 20)] * 4, dtype=np.int32)
    func = np.stack([r[0][20] for r in refs])
    b0 = np.arange(20, 41, dtype=np.int32)[None, :].copy()
    n0 = np.arange(21, dtype=np.int32)[None, :].copy()
    got, _ = _solution_from(out, dims, 21, 21, 64, func, b0, n0, 4)
    for q, ref in enumerate(refs):
        su.same_arrays({**got, "npivots": out["npivots"]}, q, 20, 20, su.of_case(ref, 20, 20), q)


def test_solution_from_a_start_code_out_of_range_gives_padding_only():
    same = [("mixed", 20, 20, s, 20) for s in range(5)]
    refs = [case(kind, n, m, seed, 64, flen) for kind, n, m, seed, flen in same]
    out = _solve([(r[0], 20, 20, 20) for r in refs], 64, kernel="wave", solution=True)
    dims = np.array([(20, 20, 20)] * 5, dtype=np.int32)
    func = np.stack([r[0][20] for r in refs])
    b0 = np.tile(np.arange(20, 41, dtype=np.int32), (5, 1))
    n0 = np.tile(np.arange(21, dtype=np.int32), (5, 1))
    b0[1, 19] = 40                                           # n + m
    n0[3, 0] = -1
    b0[4, 20] = 9999                                         # past n: never read
    got, raw = _solution_from(out, dims, 21, 21, 64, func, b0, n0, 1)
    for q in (1, 3):
        assert not su.bits(raw[0][q]).any() and not su.bits(raw[1][q]).any(), q
        assert (raw[2][q] == -1).all() and (raw[3][q] == -1).all(), q
        assert su.bits(got["objective"][q]) == 0, q
    for q in (0, 2, 4):
        su.same_arrays({**got, "npivots": out["npivots"]}, q, 20, 20,
                       su.of_case(refs[q], 20, 20), q)


# ----------------------------------------------------------------------------------------------
# the object level
def _lists(T, n, m):
    return T[:n].tolist(), T[n, :m].tolist()


def _oracle_scenario(cons, func, n, m, dr, dc, cap, capw):
    """(status name, Expected) of the warm run the oracle makes of one scenario."""
    from oracle import c_oracle
    T0 = np.zeros((n + 1, m + 1))
    T0[:n], T0[n, :m] = cons, func
    Tf, _, _, log = c_oracle.run(T0, n, m, m, cap)
    basis, nonbasis, _ = su.replay(log, n, m)
    dr = np.zeros(n) if dr is None else np.asarray(dr, dtype=np.float64)
    dc = np.zeros(m) if dc is None else np.asarray(dc, dtype=np.float64)
    S_tab, func_s = scu.restate(Tf, n, m, basis, nonbasis, func, dr, dc)
    Tw, wst, wdone, wlog = c_oracle.run(S_tab, n, m, m, capw)
    wb, wn = scu.warm_labels(basis, nonbasis, wlog, n, m)
    name = {0: "cap", 1: "optimum", 2: "error", 3: "error"}[wst]
    return name, scu.expected_solution(Tw, wb, wn, n, m, func_s, wdone)


def test_solve_batch_scenarios_over_a_mixed_bag():
    """Wave, workgroup and single problems in one call, uneven scenario counts (0, 1, 3, 2), a
    None on either side: the order is kept and every answer is the oracle's."""
    import simplex
    from simplex_mi355x import lp
    from simplex_mi355x.batch import route, solve_batch_scenarios, solve_batch_solutions
    shapes = [(65, 65, 0), (3, 2, 0), (20, 20, 1), (40, 7, 1)]
    problems, scen = [], []
    for k, (n, m, seed) in enumerate(shapes):
        T = lp.dense_tableau("uniform", seed, n, m)
        problems.append(_lists(T, n, m))
        ds = [scu.deltas(T, n, m, seed, s, 0.5, 0.5) for s in range(3)]
        scen.append([[], [(ds[0][0], None)], ds, [(None, ds[1][1]), (None, None)]][k])
    ints = ([[1, 1, -2.0], [-1, 1, 1.5], [1, -2, 4.0]], [-1, -1.0])        # int entries: single
    problems.append(ints)
    scen.append([([-1.0, 0.0, 0.0], [2.0, 0.0])])
    assert [route(*p) for p in problems] == ["workgroup", "wave", "wave", "wave", "single"]
    got = solve_batch_scenarios(problems, scen, max_pivots=1024, cold_fallback=False)
    base, _ = solve_batch_solutions(problems, max_pivots=1024)
    assert len(got) == 5
    for k, (n, m, _) in enumerate(shapes):
        sol, answers = got[k]
        su.same_solution(sol, su.Expected(*base[k]), (k, "base"))
        assert len(answers) == len(scen[k])
        for s, (dr, dc) in enumerate(scen[k]):
            name, exp = _oracle_scenario(*problems[k], n, m, dr, dc, 1024, 1024)
            assert answers[s].warm is True and answers[s].status == name, (k, s)
            su.same_solution(answers[s].solution, exp, (k, s))
    sm = simplex.SimplexMethod(*ints)
    sm.solve(record_history=False, max_pivots=1024)
    wi = sm.what_if(*scen[4][0])
    wi.solve(record_history=False, max_pivots=1024)
    su.same_solution(got[4][0], su.Expected(*sm.solution()), "single base")
    su.same_solution(got[4][1][0].solution, su.Expected(*wi.solution()), "single scenario")
    assert got[4][1][0].status == wi.status and wi.pivots > 0


def test_cold_fallback_on_the_case_whose_warm_run_does_not_terminate():
    """Uniform 60 x 12, seed 5, scenario 1 at frac 0.2, prob 0.5 with warm_pivots=64: the warm run
    is stopped by its cap, the answer is the cold solve of the perturbed problem."""
    from simplex_mi355x import lp
    from simplex_mi355x.batch import _perturbed, solve_batch_scenarios, solve_batch_solutions
    n, m, seed = 60, 12, 5
    T = lp.dense_tableau("uniform", seed, n, m)
    prob = _lists(T, n, m)
    ds = [scu.deltas(T, n, m, seed, s, 0.2, 0.5) for s in range(2)]
    got = solve_batch_scenarios([prob], [ds], max_pivots=256, warm_pivots=64)
    assert got[0][0].pivots == 12
    hard = got[0][1][1]
    assert hard.warm is False and hard.status == "optimum" and hard.solution.pivots == 22
    cold, st = solve_batch_solutions([_perturbed(*prob, *ds[1])], max_pivots=256)
    assert st == ["optimum"]
    su.same_solution(hard.solution, su.Expected(*cold[0]), "cold")
    kept = solve_batch_scenarios([prob], [ds], max_pivots=256, warm_pivots=64,
                                 cold_fallback=False)
    assert kept[0][1][1].warm is True and kept[0][1][1].status == "cap"
    assert kept[0][1][1].solution.pivots == 64
    name, exp = _oracle_scenario(*prob, n, m, *ds[1], 256, 64)
    assert name == "cap"
    su.same_solution(kept[0][1][1].solution, exp, "capped warm run")


def test_what_if_on_the_device_backend_equals_the_batch():
    import simplex
    from simplex_mi355x import lp
    from simplex_mi355x.batch import solve_batch_scenarios
    n, m, seed = 20, 20, 0
    T = lp.dense_tableau("mixed", seed, n, m)
    prob = _lists(T, n, m)
    dr, dc = scu.deltas(T, n, m, seed, 0, 0.5, 0.5)
    got = solve_batch_scenarios([prob], [[(dr, dc)]], max_pivots=64, cold_fallback=False)
    sm = simplex.SimplexMethod(*prob)
    assert sm.backend == "hip"
    sm.solve(record_history=False, max_pivots=64)
    wi = sm.what_if(dr, dc)
    assert wi.backend == "hip" and wi.pivots == 0
    wi.solve(record_history=False, max_pivots=64)
    su.same_solution(wi.solution(), su.Expected(*got[0][1][0].solution), "what_if")
    assert wi.status == got[0][1][0].status
    name, exp = _oracle_scenario(*prob, n, m, dr, dc, 64, 64)
    su.same_solution(wi.solution(), exp, "what_if against the oracle")
    assert wi.status == name


# ----------------------------------------------------------------------------------------------
# nothing else moved
def test_existing_calls_return_todays_keys():
    refs = [case(kind, n, m, seed, 64, flen) for kind, n, m, seed, flen in WAVE_MIX[:2]]
    cases = [(r[0], n, m, flen) for r, (_, n, m, _, flen) in zip(refs, WAVE_MIX[:2])]
    assert list(_solve(cases, 64, kernel="wave")) == ["final", "rc", "xv", "status", "npivots"]
    sol = _solve(cases, 64, kernel="wave", solution=True, tables=False)
    assert list(sol) == ["rc", "xv", "status", "npivots", "x", "duals", "objective", "basis",
                         "nonbasis"]
    rng = _solve(cases, 64, kernel="wave", solution=True, tables=False, ranging=True)
    assert list(rng) == list(sol) + list(ru.FIELDS)
    out, _ = _chain(WAVE_MIX[:2], 64, "wave", 1)
    assert list(out["base"]) == list(rng)
    for key in rng:
        a, b = out["base"][key], rng[key]
        assert a.dtype == b.dtype and a.shape == b.shape, key
        assert np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a,
                              b.view(np.int64) if b.dtype == np.float64 else b), key
