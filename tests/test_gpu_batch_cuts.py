"""GPU: new constraints on solved LPs on the device -- k_batch_cuts alone through the C ABI at its
tile and wave edges and on the hand-made tables, the whole chain of solve_batch_cuts_arrays on all
three tiers and across them, solve_batch_cuts and SimplexMethod.add_constraints on the device
backend -- against cuts_util's restatement on the C oracle's final tables and the oracle's warm
runs on the restated extended tables, by bit pattern."""
from __future__ import annotations

import numpy as np
import pytest

import cuts_util as cu
import ranging_util as ru
import solution_util as su
import special_values as sv
from batch_util import case

pytestmark = pytest.mark.gpu

KEYS = ("x", "duals", "objective", "basis", "nonbasis", "npivots")
PASS = 4                                                     # kCutPass: cuts per walk over T


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


def _launch(lps, S, K, Rmax, ldb, Rout, sets, ncuts=None):
    """lps: [(T, n, m, basis, nonbasis)], or None for an LP whose dims (Rmax, ldb) lie outside the
    block; sets[q][s] = G [K'][m + 1]; `ncuts` [B][S] overrides the counts -> one smx_batch_cuts
    launch, every output block compared whole with what the contract says.  The padding of every
    base block and of every cut holds a value that shows, every output starts poisoned and stands
    between poisoned guard bands that must come back untouched.  Returns tabs_c."""
    import torch
    from simplex_mi355x import _lib
    B = len(lps)
    final = np.full((B, Rmax, ldb), 3.25)
    dims = np.zeros((B, 3), dtype=np.int32)
    ba = np.full((B, Rmax), 7, dtype=np.int32)
    nb = np.full((B, ldb), 7, dtype=np.int32)
    g = np.full((B, S, K, ldb), 5.0)                         # past m and past K': never read
    nc = np.zeros((B, S), dtype=np.int32)
    for q, lp_ in enumerate(lps):
        if lp_ is None:
            dims[q] = (Rmax, ldb, ldb)
            continue
        T, n, m, basis, nonbasis = lp_
        final[q, :n + 1, :m + 1] = np.asarray(T)[:n + 1, :m + 1]
        dims[q] = (n, m, m)
        ba[q, :n], nb[q, :m] = basis, nonbasis
        for s in range(S):
            G = np.asarray(sets[q][s], dtype=np.float64).reshape(-1, m + 1)
            nc[q, s] = len(G)
            g[q, s, :len(G), :m + 1] = G
    if ncuts is not None:
        nc[:] = ncuts
    d_in = [torch.from_numpy(a).to("cuda") for a in (final, dims, ba, nb, g, nc)]
    Q = B * S
    w_t, d_t = _guarded(torch, Q * Rout * ldb, torch.float64, 7.0)
    w_d, d_d = _guarded(torch, Q * 3, torch.int32, 77)
    w_b, d_b = _guarded(torch, Q * Rout, torch.int32, 77)
    _lib.check(_lib.load().smx_batch_cuts(
        d_in[0].data_ptr(), d_in[1].data_ptr(), B, S, Rmax, ldb, d_in[2].data_ptr(),
        d_in[3].data_ptr(), d_in[4].data_ptr(), d_in[5].data_ptr(), K, Rout, d_t.data_ptr(),
        d_d.data_ptr(), d_b.data_ptr(), torch.cuda.current_stream().cuda_stream),
        "smx_batch_cuts")
    for whole, poison in ((w_t, 7.0), (w_d, 77), (w_b, 77)):
        h = whole.cpu().numpy()
        assert (h[:GUARD] == poison).all() and (h[-GUARD:] == poison).all(), "guard band"
    tabs_c = d_t.cpu().numpy().reshape(Q, Rout, ldb)
    dims_c = d_d.cpu().numpy().reshape(Q, 3)
    basis_c = d_b.cpu().numpy().reshape(Q, Rout)
    for q, lp_ in enumerate(lps):
        for s in range(S):
            k, what = q * S + s, (q, s, Rout)
            exp = np.zeros((Rout, ldb))
            bexp = np.full(Rout, -1, dtype=np.int32)
            if lp_ is None:                                  # n = Rmax - 1, no cuts, dims kept
                exp[:Rmax] = final[q]
                bexp[:Rmax - 1] = ba[q, :Rmax - 1]
                assert dims_c[k].tolist() == dims[q].tolist(), what
            else:
                T, n, m, basis, nonbasis = lp_
                kc = int(nc[q, s])
                taken = 0 <= kc <= K and n + kc < Rout
                G = np.asarray(sets[q][s], dtype=np.float64).reshape(-1, m + 1)[:kc] if taken \
                    else np.zeros((0, m + 1))
                kc = len(G)
                E, blab = cu.restate(T, n, m, basis, nonbasis, G)
                exp[:n] = final[q, :n]
                exp[n:n + kc, :m + 1] = E[n:n + kc]
                exp[n + kc] = final[q, n]
                bexp[:n + kc] = blab
                assert dims_c[k].tolist() == [n + kc, m, m], what
            assert su.same_floats(tabs_c[k], exp, nan_aware=True), what
            assert np.array_equal(basis_c[k], bexp), what
    return tabs_c


EDGES = [(63, 63, 2), (64, 64, 1), (65, 65, PASS + 1), (5, 255, PASS + 1), (5, 256, 1),
         (5, 257, 2), (257, 3, PASS + 1), (1, 1, PASS + 1), (1, 8000, 2), (8000, 1, 1)]


@pytest.mark.parametrize("n,m,K", EDGES, ids=[f"{n}x{m}-K{K}" for n, m, K in EDGES])
def test_tile_and_wave_edges(n, m, K):
    """Two seeded tables under seeded permutations of the labels, no solve, three cut sets each
    with K, 0 and about K / 2 cuts in a different order per LP: a tile of 64 columns / a chunk of 64
    rows full, one short of it and one past it, columns one past a workgroup's stride of 256, one
    cut more than a pass holds, the smallest LP and the two ends of the envelope's sum bound; with
    Rmax_out = max n + K + 1 and above it.  Every output element is compared, the padding too."""
    from simplex_mi355x import lp
    lps, sets = [], []
    for q in range(2):
        T = lp.dense_tableau("uniform", 3 + q, n, m)
        basis, nonbasis = ru.seeded_labels(n, m, 3 + q)
        lps.append((T, n, m, basis, nonbasis))
        counts = [K, 0, (K + 1) // 2][q:] + [K, 0, (K + 1) // 2][:q]
        sets.append([cu.cut_set(T, n, m, 3 + q, s, counts[s], 0.05, np.ones(m))
                     for s in range(3)])
    assert sum(int((G[:, basis[basis < m]] != 0).sum()) for _, _, _, basis, _ in lps[:1]
               for G in sets[0]) > 0
    wide = n + m + K + 8 <= 8192                             # padding where the envelope has room
    _launch(lps, 3, K, n + 1 + wide, m + 1 + 2 * wide, n + K + 1 + wide, sets)
    if wide:
        _launch(lps, 3, K, n + 1, m + 1, n + K + 4, sets)
    for q in range(2):                                       # the host twin on the same inputs
        T, _, _, basis, nonbasis = lps[q]
        err, host, _ = cu.host(T, n, m, basis, nonbasis, sets[q][q])
        assert err == 0
        cu.same_table(host, cu.restate(T, n, m, basis, nonbasis, sets[q][q])[0], (n, m, q, "host"))


HANDMADE = cu.handmade()


@pytest.mark.parametrize("hm", HANDMADE, ids=[c[0] for c in HANDMADE])
def test_handmade_tables_on_the_device(hm):
    """Each hand-made table as LP 0, 1 and 4 of a five-LP launch (LP 2 has dims outside the
    block, LP 3 is a plain table whose counts are invalid: -1 and K + 1), against smx_host_cuts."""
    name, T, n, m, basis, nonbasis, G, _ = hm
    K = 3
    err, E_host, b_host = cu.host(T, n, m, basis, nonbasis, G)
    assert err == 0
    cu.check_handmade(hm, E_host, b_host)
    mine = (T, n, m, basis, nonbasis)
    plain = (np.ones((n + 1, m + 1)), n, m, basis, nonbasis)
    one = np.ones((1, m + 1))
    lps = [mine, mine, None, plain, mine]
    sets = [[G, []], [G, one], None, [one, one], [[], G]]
    counts = np.array([[len(G), 0], [len(G), 1], [1, 1], [-1, K + 1], [0, len(G)]], dtype=np.int32)
    for Rout in (n + K + 1, n + K + 3):
        tabs_c = _launch(lps, 2, K, n + 1, m + 1, Rout, sets, ncuts=counts)
        for k in (0, 2, 9):                                  # (LP 0, set 0), (1, 0), (4, 1)
            assert su.same_floats(tabs_c[k, :n + len(G) + 1], E_host, nan_aware=True), (name, k)
        # NaN payloads of T travel as bits
        assert np.array_equal(su.bits(tabs_c[1, :n + 1]), su.bits(np.asarray(T)))


def test_a_set_that_does_not_fit_the_output_block_is_a_relayout():
    """n + ncuts >= Rmax_out: Rmax_out = n + 2 takes one cut and refuses two."""
    from simplex_mi355x import lp
    n, m = 5, 4
    T = lp.dense_tableau("uniform", 1, n, m)
    basis, nonbasis = ru.seeded_labels(n, m, 1)
    two = cu.cut_set(T, n, m, 1, 0, 2, 0.05, np.ones(m))
    _launch([(T, n, m, basis, nonbasis)], 3, 2, n + 1, m + 1, n + 2, [[two[:1], two, []]])


def test_every_refusal():
    """smx_batch_cuts with real device pointers: each bad argument alone is refused with
    hipErrorInvalidValue and nothing is written; smx_batch_cuts_fits at the envelope's edge."""
    import torch
    from simplex_mi355x import _lib
    L = _lib.load()
    B, S, K, Rmax, ldb, Rout = 2, 2, 1, 4, 3, 5
    t = {"final": torch.zeros(B * Rmax * ldb, dtype=torch.float64, device="cuda"),
         "dims": torch.tensor([[3, 2, 2]] * B, dtype=torch.int32, device="cuda"),
         "basis": torch.zeros(B * Rmax, dtype=torch.int32, device="cuda"),
         "nonbasis": torch.zeros(B * ldb, dtype=torch.int32, device="cuda"),
         "cuts": torch.zeros(B * S * K * ldb, dtype=torch.float64, device="cuda"),
         "ncuts": torch.zeros(B * S, dtype=torch.int32, device="cuda"),
         "tabs_c": torch.full((B * S * Rout * ldb,), 7.0, dtype=torch.float64, device="cuda"),
         "dims_c": torch.full((B * S * 3,), 77, dtype=torch.int32, device="cuda"),
         "basis_c": torch.full((B * S * Rout,), 77, dtype=torch.int32, device="cuda")}
    stream = torch.cuda.current_stream().cuda_stream

    def call(null=None, **kw):
        a = dict(B=B, S=S, K=K, Rmax=Rmax, ldb=ldb, Rout=Rout)
        a.update(kw)
        p = {k: (None if k == null else v.data_ptr()) for k, v in t.items()}
        return L.smx_batch_cuts(p["final"], p["dims"], a["B"], a["S"], a["Rmax"], a["ldb"],
                                p["basis"], p["nonbasis"], p["cuts"], p["ncuts"], a["K"],
                                a["Rout"], p["tabs_c"], p["dims_c"], p["basis_c"], stream)
    for kw in (dict(B=-1), dict(S=-1), dict(K=-1), dict(Rout=Rmax - 1), dict(Rmax=1, Rout=1),
               dict(ldb=1), dict(ldb=8190), dict(Rout=8190), dict(B=1 << 20, S=1 << 12)):
        assert call(**kw) == 1, kw
    for name in t:
        assert call(null=name) == 1, name
    assert call(B=0) == 0 and call(S=0) == 0
    torch.cuda.synchronize()
    assert (t["tabs_c"] == 7.0).all() and (t["dims_c"] == 77).all() and (t["basis_c"] == 77).all()
    assert call(null="cuts", K=0) == 0                       # no cut rows: the pointer is not read
    assert call() == 0
    torch.cuda.synchronize()
    assert (t["dims_c"].cpu().numpy().reshape(-1, 3) == [3, 2, 2]).all()
    for Rmax_out, ldb_, fits in ((2, 2, 1), (8190, 2, 1), (2, 8190, 1), (1, 3, 0), (8191, 2, 0),
                                 (-1, 4, 0)):
        assert L.smx_batch_cuts_fits(Rmax_out, ldb_) == fits, (Rmax_out, ldb_)


# ----------------------------------------------------------------------------------------------
# the whole chain
def _chain(members, cap, kernel, S, K, viol=0.05, warm=None, ranging=True, tables=None,
           clean=None, nan_aware=False):
    """members: [(kind, n, m, seed, flen)] (or `tables`: [(T, Tref, st, done, log)] of
    special_values.reference for them, with `clean` tables to size the cuts on) -> one
    solve_batch_cuts_arrays launch, checked against the oracle: the base answers, and per cut set
    the oracle's warm run on the restated extended table.  Set s of LP q holds (q + s) % (K + 1)
    cuts."""
    from oracle import c_oracle
    from simplex_mi355x.batch import solve_batch_cuts_arrays
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
    g = np.zeros((B, S, K, ldb))
    nc = np.zeros((B, S), dtype=np.int32)
    for q, ((_, n, m, seed, flen), ref) in enumerate(zip(members, refs)):
        tabs[q, :n + 1, :m + 1] = ref[0]
        dims[q] = (n, m, flen)
        src = ref[0] if clean is None else clean[q]
        x = cu.base_of_case(ref, n, m)[2] if clean is None else np.ones(m)
        for s in range(S):
            nc[q, s] = (q + s) % (K + 1)
            g[q, s, :nc[q, s], :m + 1] = cu.cut_set(src, n, m, seed, s, nc[q, s], viol, x)
    capw = cap if warm is None else warm
    out = solve_batch_cuts_arrays(tabs, dims, g, nc, cap, warm, kernel=kernel, ranging=ranging,
                                  log=True)
    base = out["base"]
    stats = {"warm_pivots": 0, "status": [], "logs": []}
    for q, ((_, n, m, seed, flen), ref) in enumerate(zip(members, refs)):
        what = (kernel, q, n, m)
        assert int(base["status"][q]) == ref[3], what
        su.same_arrays(base, q, n, m, su.of_case(ref, n, m), what, nan_aware)
        if ranging:
            ru.same_arrays(base, q, n, m, ru.of_case(ref, n, m), what, nan_aware)
        basis, nonbasis, _ = su.replay(ref[5], n, m)
        for s in range(S):
            kc = int(nc[q, s])
            E, basis_c = cu.restate(ref[2], n, m, basis, nonbasis, g[q, s, :kc, :m + 1])
            Tw, wst, wdone, wlog = c_oracle.run(E, n + kc, m, flen, capw)
            wb, wn = cu.warm_labels(basis_c, nonbasis, wlog, n + kc, m)
            assert int(out["status"][q, s]) == wst, (what, s, "status")
            assert np.array_equal(out["rc"][q, s, :wdone], wlog), (what, s, "log")
            view = {key: out[key][:, s] for key in KEYS}
            su.same_arrays(view, q, n + kc, m,
                           cu.expected_solution(Tw, wb, wn, n + kc, m, ref[0][n, :m], wdone),
                           (what, s), nan_aware)
            if ranging:
                ru.same_arrays({key: out[key][:, s] for key in ru.FIELDS}, q, n + kc, m,
                               ru.expected(Tw, wb, wn, n + kc, m), (what, s), nan_aware)
            stats["warm_pivots"] += wdone
            stats["status"].append(wst)
            stats["logs"].append((Tw, wst, wdone, wlog, wb, wn))
    return out, stats


WAVE_MIX = [("uniform", 3, 2, 0, 2), ("uniform", 40, 7, 1, 8), ("uniform", 60, 63, 0, 63),
            ("mixed", 20, 20, 0, 20)]


def test_wave_mixed_shapes_in_one_launch():
    out, stats = _chain(WAVE_MIX, 64, "wave", 4, 3)
    assert out["status"].shape == (4, 4) and out["x"].shape == (4, 4, 63)
    assert out["duals"].shape == (4, 4, 63) and out["rhs_lo"].shape == (4, 4, 63)
    assert out["basis"].shape == (4, 4, 63) and out["rc"].shape == (4, 4, 64, 2)
    assert stats["warm_pivots"] > 0


@pytest.mark.parametrize("B,S", [(1, 1), (5, 3), (257, 1)])
def test_batch_sizes(B, S):
    shapes = [("uniform", 3, 2), ("uniform", 7, 4), ("mixed", 6, 9), ("uniform", 12, 3)]
    members = [(*shapes[q % 4], q, shapes[q % 4][2]) for q in range(B)]
    _chain(members, 24, "wave", S, 2, viol=0.2)


def test_workgroup_100_by_100_from_a_capped_base_run():
    """The base run ends at the cap of 256: its table is still an equivalent form of its LP and
    the contract holds there."""
    members = [("uniform", 100, 100, 0, 100), ("uniform", 100, 100, 1, 100)]
    out, _ = _chain(members, 256, "workgroup", 3, 2)
    assert (out["base"]["status"] == 0).all() and (out["base"]["npivots"] == 256).all()


def test_global_141_by_141():
    out, _ = _chain([("uniform", 141, 141, 0, 141)], 64, "global", 3, 2)
    assert int(out["base"]["npivots"][0]) > 0


def test_a_separate_warm_cap():
    _, stats = _chain(WAVE_MIX, 64, "wave", 4, 3, viol=0.2, warm=1, ranging=False)
    assert 0 in stats["status"]                              # a warm run stopped by its own cap


@pytest.mark.parametrize("name", ["nan_first", "inf_b"])
def test_special_value_tables(name):
    """NaN positions follow the oracle, every other element by its bits; the cuts are sized on
    the clean table of the same seed (a NaN or inf mean would make every constant NaN)."""
    from simplex_mi355x import lp
    n, m, k = sv.WORKGROUP[0]
    ref = sv.reference(name, n, m, sv.SEEDS[0], k)
    clean = lp.dense_tableau("uniform", sv.SEEDS[0], n, m)
    _chain([("uniform", n, m, sv.SEEDS[0], m)], k, "workgroup", 3, 2, tables=[ref], clean=[clean],
           nan_aware=True)


def test_slices_of_cut_sets_give_the_same_answer(monkeypatch):
    """A table budget that holds two cut sets of the launch at a time: three slices of S = 5."""
    from simplex_mi355x import batch
    whole, _ = _chain(WAVE_MIX, 64, "wave", 5, 2, viol=0.2)
    monkeypatch.setattr(batch, "GM_TABLE_BUDGET", 2 * 4 * 66 * 64 * 8)
    seen = []
    real = batch._lib.load().smx_batch_cuts
    monkeypatch.setattr(batch._lib.load(), "smx_batch_cuts",
                        lambda *a: (seen.append(a[3]), real(*a))[1])
    sliced, _ = _chain(WAVE_MIX, 64, "wave", 5, 2, viol=0.2)
    assert seen == [2, 2, 1]
    for key in whole:
        if key != "base":
            assert su.same_floats(whole[key], sliced[key]) if whole[key].dtype == np.float64 \
                else np.array_equal(whole[key], sliced[key]), key


def test_slices_with_ranges_and_the_warm_log_equal_the_whole_call(monkeypatch):
    """The same budget with ``ranging`` and ``log`` named: the ranges, the warm pivot logs and
    the base answers of the sliced call are the unsliced call's, key by key and bit by bit."""
    from simplex_mi355x import batch
    whole, _ = _chain(WAVE_MIX, 64, "wave", 5, 2, viol=0.2, ranging=True)
    monkeypatch.setattr(batch, "GM_TABLE_BUDGET", 2 * 4 * 66 * 64 * 8)
    sliced, _ = _chain(WAVE_MIX, 64, "wave", 5, 2, viol=0.2, ranging=True)
    assert list(whole) == list(sliced) and list(whole["base"]) == list(sliced["base"])
    assert {"rc", "rhs_lo", "rhs_hi", "cost_lo", "cost_hi"} <= set(whole)
    assert whole["rc"].shape == (4, 5, 64, 2) and whole["rhs_lo"].shape == (4, 5, 62)
    for a, b in ((whole, sliced), (whole["base"], sliced["base"])):
        for key in a:
            if key != "base":
                assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape, key
                assert a[key].tobytes() == b[key].tobytes(), key


# ----------------------------------------------------------------------------------------------
# tier crossings
def _tiers_of(monkeypatch):
    from simplex_mi355x import batch
    seen = []
    real = batch.warm_kernel

    def spy(base, Rout, ldb):
        seen.append((base, real(base, Rout, ldb)))
        return seen[-1][1]
    monkeypatch.setattr(batch, "warm_kernel", spy)
    return seen


def test_63_rows_plus_one_cut_leave_the_wavefront_tier(monkeypatch):
    seen = _tiers_of(monkeypatch)
    _, stats = _chain([("uniform", 63, 63, 0, 63), ("uniform", 63, 40, 1, 40)], 64, "wave", 2, 1,
                      viol=0.2)
    assert seen == [("wave", "workgroup")] and stats["warm_pivots"] > 0


def test_a_table_at_the_lds_edge_plus_cuts_goes_to_the_global_memory_tier(monkeypatch):
    """141 columns: the last Rmax the workgroup kernel's LDS holds, plus two cut rows."""
    from simplex_mi355x.batch import gm_fits, wg_lds_bytes
    ldb = 141
    Rmax = max(R for R in range(100, 400) if wg_lds_bytes(R, ldb) >= 0)
    assert wg_lds_bytes(Rmax + 1, ldb) < 0 and gm_fits(Rmax + 2, ldb)
    seen = _tiers_of(monkeypatch)
    _, stats = _chain([("uniform", Rmax - 1, ldb - 1, 0, ldb - 1)], 16, "auto", 2, 2, viol=0.2,
                      warm=16)
    assert seen == [("workgroup", "global")]


def test_a_shape_pushed_out_of_every_envelope_raises():
    from simplex_mi355x.batch import ENVELOPE_ERROR, gm_fits, solve_batch_cuts_arrays
    assert gm_fits(724, 724) and not gm_fits(725, 724)
    tabs = np.zeros((1, 724, 724))
    dims = np.array([[723, 723, 723]], dtype=np.int32)
    with pytest.raises(ValueError, match=ENVELOPE_ERROR):
        solve_batch_cuts_arrays(tabs, dims, np.zeros((1, 1, 1, 724)),
                                np.ones((1, 1), dtype=np.int32), 4, kernel="global")
    with pytest.raises(ValueError, match=ENVELOPE_ERROR):
        # 2 x 6783 is the workgroup kernel's thinnest block; 78 rows of it are past every tier
        solve_batch_cuts_arrays(np.zeros((1, 2, 6783)), np.array([[1, 6782, 6782]], np.int32),
                                np.zeros((1, 1, 76, 6783)), np.ones((1, 1), dtype=np.int32), 4)


def test_a_base_run_of_zero_pivots_is_the_cold_solve_of_the_enlarged_problem():
    """max_pivots=0: identity labels, so E is the enlarged original and the chain is the oracle's
    cold run on it bit for bit -- log, final labels, x, duals, objective."""
    from oracle import c_oracle
    from simplex_mi355x.batch import solve_batch_cuts_arrays
    members = WAVE_MIX[:2] + [("mixed", 20, 20, 0, 20)]
    refs = [case(kind, n, m, seed, 64, flen) for kind, n, m, seed, flen in members]
    B, K, S = len(members), 2, 2
    tabs, dims = np.zeros((B, 41, 21)), np.zeros((B, 3), dtype=np.int32)
    g, nc = np.zeros((B, S, K, 21)), np.zeros((B, S), dtype=np.int32)
    for q, ((_, n, m, seed, flen), ref) in enumerate(zip(members, refs)):
        tabs[q, :n + 1, :m + 1], dims[q] = ref[0], (n, m, flen)
        for s in range(S):
            nc[q, s] = 1 + (q + s) % 2
            g[q, s, :nc[q, s], :m + 1] = cu.cut_set(ref[0], n, m, seed, s, nc[q, s], 0.2,
                                                    cu.base_of_case(ref, n, m)[2])
    out = solve_batch_cuts_arrays(tabs, dims, g, nc, 0, 64, kernel="wave", ranging=False,
                                  log=True)
    assert (out["base"]["npivots"] == 0).all()
    quiet = solve_batch_cuts_arrays(tabs, dims, g, nc, 0, 64, kernel="wave", ranging=False)
    assert "rc" not in quiet and [k for k in out if k != "rc"] == list(quiet)
    pivots = 0
    for q, ((_, n, m, seed, flen), ref) in enumerate(zip(members, refs)):
        for s in range(S):
            kc = int(nc[q, s])
            T1 = cu.enlarged(ref[0], n, m, g[q, s, :kc, :m + 1])
            Tc, cst, cdone, clog = c_oracle.run(T1, n + kc, m, flen, 64)
            assert int(out["status"][q, s]) == cst and int(out["npivots"][q, s]) == cdone
            assert np.array_equal(out["rc"][q, s, :cdone], clog), (q, s)
            su.same_arrays({key: out[key][:, s] for key in KEYS}, q, n + kc, m,
                           su.expected(Tc, clog, n + kc, m, ref[0][n]), (q, s))
            pivots += cdone
    assert pivots > 0


# ----------------------------------------------------------------------------------------------
# the object level
def _lists(T, n, m):
    return T[:n].tolist(), T[n, :m].tolist()


def _oracle_cuts(cons, func, n, m, rows, cap, capw):
    """(status name, Expected) of the warm run the oracle makes of one cut set."""
    from oracle import c_oracle
    T0 = np.zeros((n + 1, m + 1))
    T0[:n], T0[n, :m] = cons, func
    Tf, _, _, log = c_oracle.run(T0, n, m, m, cap)
    basis, nonbasis, _ = su.replay(log, n, m)
    K = len(rows)
    E, basis_c = cu.restate(Tf, n, m, basis, nonbasis, rows)
    Tw, wst, wdone, wlog = c_oracle.run(E, n + K, m, m, capw)
    wb, wn = cu.warm_labels(basis_c, nonbasis, wlog, n + K, m)
    name = {0: "cap", 1: "optimum", 2: "error", 3: "error"}[wst]
    return name, cu.expected_solution(Tw, wb, wn, n + K, m, func, wdone)


def _sets_for(T, n, m, seed, counts, cap):
    from oracle import c_oracle
    Tf, _, _, log = c_oracle.run(T, n, m, m, cap)
    x = su.expected(Tf, log, n, m, T[n]).x
    return [cu.cut_set(T, n, m, seed, s, K, 0.2, x).tolist() for s, K in enumerate(counts)]


def test_solve_batch_cuts_over_a_mixed_bag():
    """Wave, workgroup, global and single problems in one call, uneven set counts and sizes (an
    empty list of sets, an empty set): the order is kept and every answer is the oracle's."""
    import simplex
    from simplex_mi355x import lp
    from simplex_mi355x.batch import route, solve_batch_cuts, solve_batch_solutions
    shapes = [(65, 65, 0), (3, 2, 0), (20, 20, 1), (40, 7, 1), (141, 141, 0)]
    counts = [[1, 2], [], [2, 0, 3], [1], [2]]
    problems, sets = [], []
    for (n, m, seed), cs in zip(shapes, counts):
        T = lp.dense_tableau("uniform", seed, n, m)
        problems.append(_lists(T, n, m))
        sets.append(_sets_for(T, n, m, seed, cs, 128))
    ints = ([[1, 1, -2.0], [-1, 1, 1.5], [1, -2, 4.0]], [-1, -1.0])        # int entries: single
    problems.append(ints)
    sets.append([[[-1.0, -0.5, 9.25]], []])
    assert [route(*p) for p in problems] == ["workgroup", "wave", "wave", "wave", "global",
                                             "single"]
    got = solve_batch_cuts(problems, sets, max_pivots=128, cold_fallback=False)
    base, _ = solve_batch_solutions(problems, max_pivots=128)
    assert len(got) == 6
    for k, (n, m, _) in enumerate(shapes):
        sol, answers = got[k]
        su.same_solution(sol, su.Expected(*base[k]), (k, "base"))
        assert len(answers) == len(sets[k])
        for s, rows in enumerate(sets[k]):
            name, exp = _oracle_cuts(*problems[k], n, m, rows, 128, 128)
            assert answers[s].warm is True and answers[s].status == name, (k, s)
            su.same_solution(answers[s].solution, exp, (k, s))
            assert len(answers[s].solution.duals) == n + len(rows)
    sm = simplex.SimplexMethod(*ints)
    sm.solve(record_history=False, max_pivots=128)
    ext = sm.add_constraints(sets[5][0])
    ext.solve(record_history=False, max_pivots=128)
    su.same_solution(got[5][0], su.Expected(*sm.solution()), "single base")
    su.same_solution(got[5][1][0].solution, su.Expected(*ext.solution()), "single cut set")
    assert got[5][1][0].status == ext.status and ext.pivots > 0
    assert got[5][1][1].solution.pivots == 0


def test_cold_fallback_on_the_case_whose_warm_run_ends_elsewhere():
    """Seed 183 (6 x 5), cut set 2 of two cuts at 20 % (test_cuts.py pins it on the oracle): the
    warm run ends at "does not converge" after 4 pivots; with cold_fallback the answer is the cold
    solve of the enlarged problem, `optimum` after 8."""
    from simplex_mi355x import lp
    from simplex_mi355x.batch import _enlarged, solve_batch_cuts, solve_batch_solutions
    n, m, seed = 6, 5, 183
    T = lp.dense_tableau("uniform", seed, n, m)
    prob = _lists(T, n, m)
    sets = _sets_for(T, n, m, seed, [2, 2, 2], 512)
    got = solve_batch_cuts([prob], [sets], max_pivots=512)
    hard = got[0][1][2]
    assert hard.warm is False and hard.status == "optimum" and hard.solution.pivots == 8
    cold, st = solve_batch_solutions([_enlarged(*prob, sets[2])], max_pivots=512)
    assert st == ["optimum"]
    su.same_solution(hard.solution, su.Expected(*cold[0]), "cold")
    kept = solve_batch_cuts([prob], [sets], max_pivots=512, cold_fallback=False)
    assert kept[0][1][2].warm is True and kept[0][1][2].status == "error"
    assert kept[0][1][2].solution.pivots == 4
    name, exp = _oracle_cuts(*prob, n, m, sets[2], 512, 512)
    assert name == "error"
    su.same_solution(kept[0][1][2].solution, exp, "warm run")
    for s in (0, 1):                                         # the others agree: warm answers kept
        assert got[0][1][s].warm is (kept[0][1][s].status == "optimum")


def test_add_constraints_on_the_device_backend_equals_the_batch():
    import simplex
    from simplex_mi355x import lp
    from simplex_mi355x.batch import solve_batch_cuts
    n, m, seed = 20, 20, 0
    T = lp.dense_tableau("mixed", seed, n, m)
    prob = _lists(T, n, m)
    rows = _sets_for(T, n, m, seed, [2], 64)[0]
    got = solve_batch_cuts([prob], [[rows]], max_pivots=64, cold_fallback=False)
    sm = simplex.SimplexMethod(*prob)
    assert sm.backend == "hip"
    sm.solve(record_history=False, max_pivots=64)
    ext = sm.add_constraints(rows)
    assert ext.backend == "hip" and ext.pivots == 0 and ext.n == n + 2
    assert ext.column[n:] == [f"y{n + 1}", f"y{n + 2}", "f"]
    ext.solve(record_history=False, max_pivots=64)
    su.same_solution(ext.solution(), su.Expected(*got[0][1][0].solution), "add_constraints")
    assert ext.status == got[0][1][0].status
    name, exp = _oracle_cuts(*prob, n, m, rows, 64, 64)
    su.same_solution(ext.solution(), exp, "add_constraints against the oracle")
    assert ext.status == name
