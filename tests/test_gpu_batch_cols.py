"""GPU: new variables on solved LPs on the device -- k_batch_cols alone through the C ABI at its
row-block, column-chunk and pass edges and on the hand-made tables, the whole chain of
solve_batch_columns_arrays on all three tiers and across them, solve_batch_columns and
SimplexMethod.add_variables on the device backend -- against cols_util's restatement on the C
oracle's final tables and the oracle's warm runs on the restated widened tables, by bit pattern."""
from __future__ import annotations

import numpy as np
import pytest

import cols_util as co
import ranging_util as ru
import solution_util as su
import special_values as sv
from batch_util import case

pytestmark = pytest.mark.gpu

KEYS = ("x", "duals", "objective", "basis", "nonbasis", "npivots")
PASS = 4                                                     # kColPass: columns per walk over T
F8, I4 = np.dtype(np.float64), np.dtype(np.int32)


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


def _launch(lps, S, K, Rmax, ldb, ldb_out, sets, ncols=None, memo=None):
    """lps: [(T, n, m, basis, nonbasis, flen)], or None for an LP whose dims (Rmax, ldb) lie
    outside the block; sets[q][s] = A [K'][n + 1]; `ncols` [B][S] overrides the counts -> one
    smx_batch_cols launch, every output block compared whole with what the contract says.  The
    padding of every base block, of `func` and of every column holds a value that shows, every
    output starts poisoned and stands between poisoned guard bands that must come back untouched.
    `memo` keeps the restatements between two launches of the same inputs.  Returns tabs_v."""
    import torch
    from simplex_mi355x import _lib
    B = len(lps)
    final = np.full((B, Rmax, ldb), 3.25)
    dims = np.zeros((B, 3), dtype=np.int32)
    ba = np.full((B, Rmax), 7, dtype=np.int32)
    nb = np.full((B, ldb), 7, dtype=np.int32)
    func = np.full((B, ldb), 9.5)
    a = np.full((B, S, K, Rmax), 5.0)                        # past n and past K': never read
    nc = np.zeros((B, S), dtype=np.int32)
    for q, lp_ in enumerate(lps):
        if lp_ is None:
            dims[q] = (Rmax, ldb, ldb)
            continue
        T, n, m, basis, nonbasis, flen = lp_
        final[q, :n + 1, :m + 1] = np.asarray(T)[:n + 1, :m + 1]
        func[q, :m] = np.arange(1.0, m + 1.0)
        dims[q] = (n, m, flen)
        ba[q, :n], nb[q, :m] = basis, nonbasis
        for s in range(S):
            A = np.asarray(sets[q][s], dtype=np.float64).reshape(-1, n + 1)
            nc[q, s] = len(A)
            a[q, s, :len(A), :n + 1] = A
    if ncols is not None:
        nc[:] = ncols
    d_in = [torch.from_numpy(x).to("cuda") for x in (final, dims, ba, nb, func, a, nc)]
    Q = B * S
    w_t, d_t = _guarded(torch, Q * Rmax * ldb_out, torch.float64, 7.0)
    w_f, d_f = _guarded(torch, Q * ldb_out, torch.float64, 7.0)
    w_d, d_d = _guarded(torch, Q * 3, torch.int32, 77)
    w_b, d_b = _guarded(torch, Q * Rmax, torch.int32, 77)
    w_n, d_n = _guarded(torch, Q * ldb_out, torch.int32, 77)
    _lib.check(_lib.load().smx_batch_cols(
        d_in[0].data_ptr(), d_in[1].data_ptr(), B, S, Rmax, ldb, d_in[2].data_ptr(),
        d_in[3].data_ptr(), d_in[4].data_ptr(), d_in[5].data_ptr(), d_in[6].data_ptr(), K, ldb_out,
        d_t.data_ptr(), d_f.data_ptr(), d_d.data_ptr(), d_b.data_ptr(), d_n.data_ptr(),
        torch.cuda.current_stream().cuda_stream), "smx_batch_cols")
    for whole, poison in ((w_t, 7.0), (w_f, 7.0), (w_d, 77), (w_b, 77), (w_n, 77)):
        h = whole.cpu().numpy()
        assert (h[:GUARD] == poison).all() and (h[-GUARD:] == poison).all(), "guard band"
    tabs_v = d_t.cpu().numpy().reshape(Q, Rmax, ldb_out)
    func_v = d_f.cpu().numpy().reshape(Q, ldb_out)
    dims_v = d_d.cpu().numpy().reshape(Q, 3)
    basis_v = d_b.cpu().numpy().reshape(Q, Rmax)
    nonbasis_v = d_n.cpu().numpy().reshape(Q, ldb_out)
    memo = {} if memo is None else memo
    for q, lp_ in enumerate(lps):
        for s in range(S):
            k, what = q * S + s, (q, s, ldb_out)
            exp = np.zeros((Rmax, ldb_out))
            fexp = np.zeros(ldb_out)
            bexp = np.full(Rmax, -1, dtype=np.int32)
            nexp = np.full(ldb_out, -1, dtype=np.int32)
            if lp_ is None:                                  # m = ldb - 1, no columns, dims kept
                exp[:, :ldb] = final[q]
                assert dims_v[k].tolist() == dims[q].tolist(), what
            else:
                T, n, m, basis, nonbasis, flen = lp_
                kc = int(nc[q, s])
                taken = 0 <= kc <= K and m + kc < ldb_out and flen >= m
                A = np.asarray(sets[q][s], dtype=np.float64).reshape(-1, n + 1)[:kc] if taken \
                    else np.zeros((0, n + 1))
                kc = len(A)
                if (q, s, kc) not in memo:
                    memo[q, s, kc] = co.restate(T, n, m, basis, nonbasis, A)
                W, blab, nlab = memo[q, s, kc]
                exp[:, :m] = final[q, :, :m]                 # the rows past n too
                exp[:, m + kc] = final[q, :, m]
                exp[:n + 1, m:m + kc] = W[:, m:m + kc]
                fexp[:m], fexp[m:m + kc] = func[q, :m], A[:, n]
                bexp[:n], nexp[:m + kc] = blab, nlab
                assert dims_v[k].tolist() == [n, m + kc, flen + kc], what
            assert su.same_floats(tabs_v[k], exp, nan_aware=True), what
            assert np.array_equal(su.bits(func_v[k]), su.bits(fexp)), what
            assert np.array_equal(basis_v[k], bexp) and np.array_equal(nonbasis_v[k], nexp), what
    return tabs_v


EDGES = [(63, 63, 2), (64, 64, 1), (65, 65, PASS + 1), (255, 5, PASS + 1), (256, 5, 1),
         (257, 5, 2), (3, 257, PASS + 1), (1, 1, PASS + 1), (8000, 1, 2), (1, 8000, 1)]


@pytest.mark.parametrize("n,m,K", EDGES, ids=[f"{n}x{m}-K{K}" for n, m, K in EDGES])
def test_block_chunk_and_pass_edges(n, m, K):
    """Two seeded tables under seeded permutations of the labels, no solve, three column sets each
    with K, 0 and about K / 2 columns in a different order per LP: a block of 64 rows (rows 0..n)
    / a chunk of 64 columns full, one short of it and one past it, rows one past a workgroup's
    stride of 256, one column more than a pass holds, the smallest LP and the two ends of the
    envelope's sum bound; with ldb_out = ldb + K and above it.  Every output element is compared,
    the padding too."""
    from simplex_mi355x import lp
    lps, sets = [], []
    for q in range(2):
        T = lp.dense_tableau("uniform", 3 + q, n, m)
        basis, nonbasis = ru.seeded_labels(n, m, 3 + q)
        lps.append((T, n, m, basis, nonbasis, m + q))
        counts = [K, 0, (K + 1) // 2][q:] + [K, 0, (K + 1) // 2][:q]
        sets.append([co.plain_cols(n, 3 + q, s, counts[s]) for s in range(3)])
    applied = sum(int((A[:, lp_[4][lp_[4] >= m] - m] != 0).sum())
                  for lp_, group in zip(lps, sets) for A in group)
    assert applied > 0 or n + m == 2                         # terms to sum, past the 1 x 1 LP
    wide = n + m + K + 8 <= 8192                             # padding where the envelope has room
    memo = {}
    _launch(lps, 3, K, n + 1 + wide, m + 1 + 2 * wide, m + 1 + 2 * wide + K, sets, memo=memo)
    if wide:
        _launch(lps, 3, K, n + 1, m + 1, m + K + 4, sets, memo=memo)
    for q in range(2):                                       # the host twin on the same inputs
        T, _, _, basis, nonbasis, _ = lps[q]
        err, host, bv, nv = co.host(T, n, m, basis, nonbasis, sets[q][q])
        assert err == 0
        W, bexp, nexp = memo[q, q, len(sets[q][q])]
        co.same_table(host, W, (n, m, q, "host"))
        assert np.array_equal(bv, bexp) and np.array_equal(nv, nexp)


HANDMADE = co.handmade()


@pytest.mark.parametrize("hm", HANDMADE, ids=[c[0] for c in HANDMADE])
def test_handmade_tables_on_the_device(hm):
    """Each hand-made table as LP 0, 1 and 4 of a six-LP launch (LP 2 has dims outside the
    block, LP 3 is a plain table whose counts are invalid, -1 and K + 1, and whose second twin, LP
    5, has a function shorter than m), against smx_host_cols."""
    name, T, n, m, basis, nonbasis, A, _ = hm
    K = 3
    err, W_host, b_host, n_host = co.host(T, n, m, basis, nonbasis, A)
    assert err == 0
    co.check_handmade(hm, W_host, b_host, n_host)
    mine = (T, n, m, basis, nonbasis, m)
    ident = (np.arange(m, m + n, dtype=np.int32), np.arange(m, dtype=np.int32))
    plain = (np.ones((n + 1, m + 1)), n, m, *ident, m)
    short = (np.ones((n + 1, m + 1)), n, m, *ident, m - 1)
    one = np.ones((1, n + 1))
    lps = [mine, mine, None, plain, mine, short]
    sets = [[A, []], [A, one], None, [one, one], [[], A], [one, []]]
    counts = np.array([[len(A), 0], [len(A), 1], [1, 1], [-1, K + 1], [0, len(A)], [1, 0]],
                      dtype=np.int32)
    for ldb_out in (m + 1 + K, m + 1 + K + 2):
        tabs_v = _launch(lps, 2, K, n + 1, m + 1, ldb_out, sets, ncols=counts)
        for k in (0, 2, 9):                                  # (LP 0, set 0), (1, 0), (4, 1)
            assert su.same_floats(tabs_v[k, :, :m + len(A) + 1], W_host, nan_aware=True), (name, k)
        # NaN payloads of T travel as bits: a set of no columns is T, "-b" in place
        assert np.array_equal(su.bits(tabs_v[1, :, :m + 1]), su.bits(np.asarray(T)))


def test_a_set_that_does_not_fit_the_output_block_is_a_relayout():
    """m + ncols >= ldb_out: ldb_out = m + 2 takes one column and refuses two."""
    from simplex_mi355x import lp
    n, m = 5, 4
    T = lp.dense_tableau("uniform", 1, n, m)
    basis, nonbasis = ru.seeded_labels(n, m, 1)
    two = co.plain_cols(n, 1, 0, 2)
    _launch([(T, n, m, basis, nonbasis, m)], 3, 2, n + 1, m + 1, m + 2, [[two[:1], two, []]])


def test_every_refusal():
    """smx_batch_cols with real device pointers: each bad argument alone is refused with
    hipErrorInvalidValue and nothing is written; smx_batch_cols_fits at the envelope's edge."""
    import torch
    from simplex_mi355x import _lib
    L = _lib.load()
    B, S, K, Rmax, ldb, ldo = 2, 2, 1, 4, 3, 4
    t = {"final": torch.zeros(B * Rmax * ldb, dtype=torch.float64, device="cuda"),
         "dims": torch.tensor([[3, 2, 2]] * B, dtype=torch.int32, device="cuda"),
         "basis": torch.zeros(B * Rmax, dtype=torch.int32, device="cuda"),
         "nonbasis": torch.zeros(B * ldb, dtype=torch.int32, device="cuda"),
         "func": torch.zeros(B * ldb, dtype=torch.float64, device="cuda"),
         "cols": torch.zeros(B * S * K * Rmax, dtype=torch.float64, device="cuda"),
         "ncols": torch.zeros(B * S, dtype=torch.int32, device="cuda"),
         "tabs_v": torch.full((B * S * Rmax * ldo,), 7.0, dtype=torch.float64, device="cuda"),
         "func_v": torch.full((B * S * ldo,), 7.0, dtype=torch.float64, device="cuda"),
         "dims_v": torch.full((B * S * 3,), 77, dtype=torch.int32, device="cuda"),
         "basis_v": torch.full((B * S * Rmax,), 77, dtype=torch.int32, device="cuda"),
         "nonbasis_v": torch.full((B * S * ldo,), 77, dtype=torch.int32, device="cuda")}
    outs = ("tabs_v", "func_v", "dims_v", "basis_v", "nonbasis_v")
    stream = torch.cuda.current_stream().cuda_stream

    def call(null=None, **kw):
        a = dict(B=B, S=S, K=K, Rmax=Rmax, ldb=ldb, ldo=ldo)
        a.update(kw)
        p = {k: (None if k == null else v.data_ptr()) for k, v in t.items()}
        return L.smx_batch_cols(p["final"], p["dims"], a["B"], a["S"], a["Rmax"], a["ldb"],
                                p["basis"], p["nonbasis"], p["func"], p["cols"], p["ncols"],
                                a["K"], a["ldo"], *(p[k] for k in outs), stream)
    for kw in (dict(B=-1), dict(S=-1), dict(K=-1), dict(ldo=ldb - 1), dict(ldb=1, ldo=1),
               dict(Rmax=1), dict(Rmax=8190), dict(ldo=8189), dict(B=1 << 20, S=1 << 12)):
        assert call(**kw) == 1, kw
    for name in t:
        assert call(null=name) == 1, name
    assert call(B=0) == 0 and call(S=0) == 0
    torch.cuda.synchronize()
    for k in outs:
        assert (t[k] == (7.0 if t[k].dtype == torch.float64 else 77)).all(), k
    assert call(null="cols", K=0) == 0                       # no columns: the pointer is not read
    assert call() == 0
    torch.cuda.synchronize()
    assert (t["dims_v"].cpu().numpy().reshape(-1, 3) == [3, 2, 2]).all()
    for Rmax_, ldo_, fits in ((2, 2, 1), (8190, 2, 1), (2, 8190, 1), (1, 3, 0), (8191, 2, 0),
                              (4, -1, 0)):
        assert L.smx_batch_cols_fits(Rmax_, ldo_) == fits, (Rmax_, ldo_)


# ----------------------------------------------------------------------------------------------
# the whole chain
def _chain(members, cap, kernel, S, K, viol=0.05, warm=None, ranging=True, tables=None,
           nan_aware=False):
    """members: [(kind, n, m, seed, flen)] (or `tables`: [(T, Tref, st, done, log)] of
    special_values.reference for them; their columns then look at no table) -> one
    solve_batch_columns_arrays launch, checked against the oracle: the base answers, and per
    column set the oracle's warm run on the restated widened table.  Set s of LP q holds
    (q + s) % (K + 1) columns."""
    from oracle import c_oracle
    from simplex_mi355x.batch import solve_batch_columns_arrays
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
    a = np.zeros((B, S, K, Rmax))
    nc = np.zeros((B, S), dtype=np.int32)
    labels = []
    for q, ((_, n, m, seed, flen), ref) in enumerate(zip(members, refs)):
        tabs[q, :n + 1, :m + 1] = ref[0]
        dims[q] = (n, m, flen)
        labels.append(co.base_of_case(ref, n, m))
        for s in range(S):
            nc[q, s] = (q + s) % (K + 1)
            a[q, s, :nc[q, s], :n + 1] = (
                co.plain_cols(n, seed, s, nc[q, s]) if tables is not None else
                co.col_set(ref[0], n, m, seed, s, nc[q, s], viol, ref[2], *labels[q]))
    capw = cap if warm is None else warm
    out = solve_batch_columns_arrays(tabs, dims, a, nc, cap, warm, kernel=kernel, ranging=ranging,
                                     log=True)
    base = out["base"]
    assert out["x"].shape == (B, S, ldb + K - 1) and out["duals"].shape == (B, S, Rmax - 1)
    assert out["nonbasis"].shape == (B, S, ldb + K - 1) and out["basis"].shape == (B, S, Rmax - 1)
    stats = {"warm_pivots": 0, "status": []}
    for q, ((_, n, m, seed, flen), ref) in enumerate(zip(members, refs)):
        what = (kernel, q, n, m)
        assert int(base["status"][q]) == ref[3], what
        su.same_arrays(base, q, n, m, su.of_case(ref, n, m), what, nan_aware)
        if ranging:
            ru.same_arrays(base, q, n, m, ru.of_case(ref, n, m), what, nan_aware)
        basis, nonbasis = labels[q]
        for s in range(S):
            kc = int(nc[q, s])
            A = a[q, s, :kc, :n + 1]
            W, basis_v, nonbasis_v = co.restate(ref[2], n, m, basis, nonbasis, A)
            Tw, wst, wdone, wlog = c_oracle.run(W, n, m + kc, flen + kc, capw)
            wb, wn = co.warm_labels(basis_v, nonbasis_v, wlog, n, m + kc)
            assert int(out["status"][q, s]) == wst, (what, s, "status")
            assert np.array_equal(out["rc"][q, s, :wdone], wlog), (what, s, "log")
            view = {key: out[key][:, s] for key in KEYS}
            wfunc = list(ref[0][n, :m]) + list(A[:, n])
            su.same_arrays(view, q, n, m + kc,
                           co.expected_solution(Tw, wb, wn, n, m + kc, wfunc, wdone),
                           (what, s), nan_aware)
            if ranging:
                ru.same_arrays({key: out[key][:, s] for key in ru.FIELDS}, q, n, m + kc,
                               ru.expected(Tw, wb, wn, n, m + kc), (what, s), nan_aware)
            stats["warm_pivots"] += wdone
            stats["status"].append(wst)
    return out, stats


WAVE_MIX = [("uniform", 3, 2, 0, 2), ("uniform", 40, 7, 1, 8), ("uniform", 60, 59, 0, 59),
            ("mixed", 20, 20, 0, 20)]


def test_wave_mixed_shapes_in_one_launch():
    out, stats = _chain(WAVE_MIX, 64, "wave", 4, 3)
    assert out["status"].shape == (4, 4) and out["x"].shape == (4, 4, 62)
    assert out["duals"].shape == (4, 4, 60) and out["cost_lo"].shape == (4, 4, 62)
    assert out["rc"].shape == (4, 4, 64, 2)
    assert stats["warm_pivots"] > 0


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
    """NaN positions follow the oracle, every other element by its bits; the columns look at no
    table (a cost found on a NaN table would be NaN)."""
    n, m, k = sv.WORKGROUP[0]
    ref = sv.reference(name, n, m, sv.SEEDS[0], k)
    _chain([("uniform", n, m, sv.SEEDS[0], m)], k, "workgroup", 3, 2, tables=[ref],
           nan_aware=True)


def test_slices_of_column_sets_give_the_same_answer(monkeypatch):
    """A table budget that holds two column sets of the launch at a time, counted in the WIDENED
    tables' columns: three slices of S = 5, and the whole call's answer key by key, bit by bit."""
    from simplex_mi355x import batch
    whole, _ = _chain(WAVE_MIX, 64, "wave", 5, 2, viol=0.2)
    monkeypatch.setattr(batch, "GM_TABLE_BUDGET", 2 * 4 * 61 * 62 * 8)
    seen = []
    real = batch._lib.load().smx_batch_cols
    monkeypatch.setattr(batch._lib.load(), "smx_batch_cols",
                        lambda *a: (seen.append(a[3]), real(*a))[1])
    sliced, _ = _chain(WAVE_MIX, 64, "wave", 5, 2, viol=0.2)
    assert seen == [2, 2, 1]
    assert list(whole) == list(sliced) and list(whole["base"]) == list(sliced["base"])
    assert {"rc", "rhs_lo", "rhs_hi", "cost_lo", "cost_hi"} <= set(whole)
    for x, y in ((whole, sliced), (whole["base"], sliced["base"])):
        for key in x:
            if key != "base":
                assert x[key].dtype == y[key].dtype and x[key].shape == y[key].shape, key
                assert x[key].tobytes() == y[key].tobytes(), key


# ----------------------------------------------------------------------------------------------
# tier crossings
def _tiers_of(monkeypatch):
    from simplex_mi355x import batch
    seen = []
    real = batch.warm_kernel

    def spy(base, Rmax, ldb_out):
        seen.append((base, real(base, Rmax, ldb_out)))
        return seen[-1][1]
    monkeypatch.setattr(batch, "warm_kernel", spy)
    return seen


def test_64_columns_plus_one_leave_the_wavefront_tier(monkeypatch):
    seen = _tiers_of(monkeypatch)
    _, stats = _chain([("uniform", 63, 63, 0, 63), ("uniform", 40, 63, 1, 63)], 64, "wave", 2, 1,
                      viol=0.2)
    assert seen == [("wave", "workgroup")] and stats["warm_pivots"] > 0


def test_a_table_at_the_lds_edge_plus_columns_goes_to_the_global_memory_tier(monkeypatch):
    """141 rows: the last ldb the workgroup kernel's LDS holds, plus two new columns."""
    from simplex_mi355x.batch import gm_fits, wg_lds_bytes
    Rmax = 141
    ldb = max(c for c in range(100, 400) if wg_lds_bytes(Rmax, c) >= 0)
    assert wg_lds_bytes(Rmax, ldb + 1) < 0 and gm_fits(Rmax, ldb + 2)
    seen = _tiers_of(monkeypatch)
    _chain([("uniform", Rmax - 1, ldb - 1, 0, ldb - 1)], 16, "auto", 2, 2, viol=0.2, warm=16)
    assert seen == [("workgroup", "global")]


def test_a_shape_pushed_out_of_every_envelope_raises_before_anything_is_enqueued(monkeypatch):
    import torch
    from simplex_mi355x.batch import ENVELOPE_ERROR, gm_fits, solve_batch_columns_arrays
    assert gm_fits(724, 724) and not gm_fits(724, 725)

    def boom(*a, **k):
        raise AssertionError("something was sent to the device")
    monkeypatch.setattr(torch, "from_numpy", boom)
    tabs = np.zeros((1, 724, 724))
    dims = np.array([[723, 723, 723]], dtype=np.int32)
    with pytest.raises(ValueError, match=ENVELOPE_ERROR):
        solve_batch_columns_arrays(tabs, dims, np.zeros((1, 1, 1, 724)),
                                   np.ones((1, 1), dtype=np.int32), 4, kernel="global")
    with pytest.raises(ValueError, match=ENVELOPE_ERROR):
        # a wave block whose widened form is past the envelope's sum bound (Rmax + ldb <= 8192)
        solve_batch_columns_arrays(np.zeros((1, 3, 3)), np.array([[2, 2, 2]], np.int32),
                                   np.zeros((1, 1, 8187, 3)), np.ones((1, 1), dtype=np.int32), 4)


def test_a_base_run_of_zero_pivots_is_the_cold_solve_of_the_widened_problem():
    """max_pivots=0: identity labels, so W is the widened original and the chain is the oracle's
    cold run on it bit for bit -- log, final labels, x, duals, objective."""
    from oracle import c_oracle
    from simplex_mi355x.batch import solve_batch_columns_arrays
    members = WAVE_MIX[:2] + [("mixed", 20, 20, 0, 20)]
    refs = [case(kind, n, m, seed, 64, flen) for kind, n, m, seed, flen in members]
    B, K, S = len(members), 2, 2
    tabs, dims = np.zeros((B, 41, 21)), np.zeros((B, 3), dtype=np.int32)
    a, nc = np.zeros((B, S, K, 41)), np.zeros((B, S), dtype=np.int32)
    for q, ((_, n, m, seed, flen), ref) in enumerate(zip(members, refs)):
        tabs[q, :n + 1, :m + 1], dims[q] = ref[0], (n, m, flen)
        for s in range(S):
            nc[q, s] = 1 + (q + s) % 2
            a[q, s, :nc[q, s], :n + 1] = co.col_set(ref[0], n, m, seed, s, nc[q, s], 0.2, ref[2],
                                                    *co.base_of_case(ref, n, m))
    out = solve_batch_columns_arrays(tabs, dims, a, nc, 0, 64, kernel="wave", ranging=False,
                                     log=True)
    assert (out["base"]["npivots"] == 0).all()
    quiet = solve_batch_columns_arrays(tabs, dims, a, nc, 0, 64, kernel="wave", ranging=False)
    assert "rc" not in quiet and [k for k in out if k != "rc"] == list(quiet)
    pivots = 0
    for q, ((_, n, m, seed, flen), ref) in enumerate(zip(members, refs)):
        for s in range(S):
            kc = int(nc[q, s])
            T1 = co.widened(ref[0], n, m, a[q, s, :kc, :n + 1])
            Tc, cst, cdone, clog = c_oracle.run(T1, n, m + kc, flen + kc, 64)
            assert int(out["status"][q, s]) == cst and int(out["npivots"][q, s]) == cdone
            assert np.array_equal(out["rc"][q, s, :cdone], clog), (q, s)
            su.same_arrays({key: out[key][:, s] for key in KEYS}, q, n, m + kc,
                           su.expected(Tc, clog, n, m + kc, T1[n]), (q, s))
            pivots += cdone
    assert pivots > 0


@pytest.mark.parametrize("B,S", [(2, 0), (0, 0), (0, 2)])
def test_keys_order_shapes_and_dtypes_without_sets_or_problems(B, S):
    """S == 0 and B == 0 (2 x 2 LPs, room for K = 2 columns): the keys of any other call in its
    order, the column-shaped arrays ldb + K - 1 wide."""
    from simplex_mi355x.batch import solve_batch_arrays, solve_batch_columns_arrays
    tabs = np.zeros((B, 3, 3))
    for q in range(B):
        tabs[q] = [[1.0, 1.0, 2.0 + q], [1.0, -1.0, 1.0], [-1.0, -1.0, 0.0]]
    dims = np.full((B, 3), 2, dtype=np.int32)
    K, cap = 2, 4

    def call(S_, ranging, log):
        return solve_batch_columns_arrays(tabs, dims, np.zeros((B, S_, K, 3)),
                                          np.zeros((B, S_), dtype=np.int32), cap, ranging=ranging,
                                          log=log)
    for ranging in (False, True):
        for log in (False, True):
            out = call(S, ranging, log)
            form = {"base": None, "status": ((B, S), I4), "npivots": ((B, S), I4)}
            if log:
                form["rc"] = ((B, S, cap, 2), I4)
            form.update({"x": ((B, S, 2 + K), F8), "duals": ((B, S, 2), F8),
                         "objective": ((B, S), F8), "basis": ((B, S, 2), I4),
                         "nonbasis": ((B, S, 2 + K), I4)})
            if ranging:
                form.update({"rhs_lo": ((B, S, 2), F8), "rhs_hi": ((B, S, 2), F8),
                             "cost_lo": ((B, S, 2 + K), F8), "cost_hi": ((B, S, 2 + K), F8)})
            assert list(out) == list(form), (ranging, log)
            for key, spec in form.items():
                if spec is not None:
                    assert out[key].shape == spec[0] and out[key].dtype == spec[1], (key, ranging)
            ref = solve_batch_arrays(tabs, dims, cap, solution=True, tables=False, ranging=ranging)
            assert list(out["base"]) == list(ref)
            for key in ref:
                assert out["base"][key].tobytes() == ref[key].tobytes(), key
            if B:
                assert list(call(1, ranging, log)) == list(out)


# ----------------------------------------------------------------------------------------------
# the object level
def _lists(T, n, m):
    return T[:n].tolist(), T[n, :m].tolist()


def _oracle_cols(cons, func, n, m, cols, cap, capw):
    """(status name, Expected) of the warm run the oracle makes of one column set."""
    from oracle import c_oracle
    T0 = np.zeros((n + 1, m + 1))
    T0[:n], T0[n, :m] = cons, func
    Tf, _, _, log = c_oracle.run(T0, n, m, m, cap)
    basis, nonbasis, _ = su.replay(log, n, m)
    K = len(cols)
    W, basis_v, nonbasis_v = co.restate(Tf, n, m, basis, nonbasis, cols)
    Tw, wst, wdone, wlog = c_oracle.run(W, n, m + K, m + K, capw)
    wb, wn = co.warm_labels(basis_v, nonbasis_v, wlog, n, m + K)
    name = {0: "cap", 1: "optimum", 2: "error", 3: "error"}[wst]
    wfunc = list(func) + [float(c[n]) for c in cols]
    return name, co.expected_solution(Tw, wb, wn, n, m + K, wfunc, wdone)


def _sets_for(T, n, m, seed, counts, cap):
    from oracle import c_oracle
    Tf, _, _, log = c_oracle.run(T, n, m, m, cap)
    basis, nonbasis, _ = su.replay(log, n, m)
    return [co.col_set(T, n, m, seed, s, K, 0.2, Tf, basis, nonbasis).tolist()
            for s, K in enumerate(counts)]


def test_solve_batch_columns_over_a_mixed_bag():
    """Wave, workgroup and single problems in one call, uneven set counts and sizes (an empty
    list of sets, an empty set): the order is kept and every answer is the oracle's."""
    import simplex
    from simplex_mi355x import lp
    from simplex_mi355x.batch import route, solve_batch_columns, solve_batch_solutions
    shapes = [(65, 65, 0), (3, 2, 0), (20, 20, 1), (40, 7, 1)]
    counts = [[1, 2], [], [2, 0, 3], [1]]
    problems, sets = [], []
    for (n, m, seed), cs in zip(shapes, counts):
        T = lp.dense_tableau("uniform", seed, n, m)
        problems.append(_lists(T, n, m))
        sets.append(_sets_for(T, n, m, seed, cs, 128))
    ints = ([[1, 1, -2.0], [-1, 1, 1.5], [1, -2, 4.0]], [-1, -1.0])        # int entries: single
    problems.append(ints)
    sets.append([[[1.0, -1.0, 0.5, -2.5]], []])
    assert [route(*p) for p in problems] == ["workgroup", "wave", "wave", "wave", "single"]
    got = solve_batch_columns(problems, sets, max_pivots=128, cold_fallback=False)
    base, _ = solve_batch_solutions(problems, max_pivots=128)
    assert len(got) == 5
    for k, (n, m, _) in enumerate(shapes):
        sol, answers = got[k]
        su.same_solution(sol, su.Expected(*base[k]), (k, "base"))
        assert len(answers) == len(sets[k])
        for s, cols in enumerate(sets[k]):
            name, exp = _oracle_cols(*problems[k], n, m, cols, 128, 128)
            assert answers[s].warm is True and answers[s].status == name, (k, s)
            su.same_solution(answers[s].solution, exp, (k, s))
            assert len(answers[s].solution.x) == m + len(cols)
            assert len(answers[s].solution.duals) == n
    sm = simplex.SimplexMethod(*ints)
    sm.solve(record_history=False, max_pivots=128)
    ext = sm.add_variables(sets[4][0])
    ext.solve(record_history=False, max_pivots=128)
    su.same_solution(got[4][0], su.Expected(*sm.solution()), "single base")
    su.same_solution(got[4][1][0].solution, su.Expected(*ext.solution()), "single column set")
    assert got[4][1][0].status == ext.status and ext.pivots > 0
    assert got[4][1][1].solution.pivots == 0
    # with the cold fallback every set that did not end at an optimum warm is solved cold
    cold = solve_batch_columns(problems[1:3], sets[1:3], max_pivots=128)
    for k in (1, 2):
        for s, sc in enumerate(cold[k - 1][1]):
            assert sc.warm is (got[k][1][s].status == "optimum"), (k, s)


def test_add_variables_on_the_device_backend_equals_the_batch():
    import simplex
    from simplex_mi355x import lp
    from simplex_mi355x.batch import solve_batch_columns
    n, m, seed = 20, 20, 0
    T = lp.dense_tableau("mixed", seed, n, m)
    prob = _lists(T, n, m)
    cols = _sets_for(T, n, m, seed, [2], 64)[0]
    got = solve_batch_columns([prob], [[cols]], max_pivots=64, cold_fallback=False)
    sm = simplex.SimplexMethod(*prob)
    assert sm.backend == "hip"
    sm.solve(record_history=False, max_pivots=64)
    ext = sm.add_variables(cols)
    assert ext.backend == "hip" and ext.pivots == 0 and (ext.n, ext.m) == (n, m + 2)
    assert ext.row[m:] == [f"x{m + 1}", f"x{m + 2}", "-b"]
    ext.solve(record_history=False, max_pivots=64)
    su.same_solution(ext.solution(), su.Expected(*got[0][1][0].solution), "add_variables")
    assert ext.status == got[0][1][0].status
    name, exp = _oracle_cols(*prob, n, m, cols, 64, 64)
    su.same_solution(ext.solution(), exp, "add_variables against the oracle")
    assert ext.status == name
