"""New variables from a batch: 2048 uniform LPs of 100 x 100 and of 65 x 65 (k_batch_wg,
max_pivots = 256) and 200 000 UI-shaped LPs (m = 2, n = 3..20, k_batch, 64), each with S = 8 column
sets of one new variable (normal coefficients on three quarters of the constraints, the cost placed
so that the variable's reduced cost at the base answer is -+5 % of the mean |cost|, the sign
alternating with the set).  Per workload one JSON line:

  kernel_ms          k_batch_cols alone on resident buffers by HIP events (10 launches after a
                     warm-up launch) with the bytes per second of the copy it contains (one read of
                     a base table and one write of a widened table per set) and smx_copy_probe's
                     rate on as many bytes
  new                wall time of solve_batch_columns_arrays (base solve included)
  yardstick          what a caller does without it: the B * S widened originals through
                     solve_batch_arrays(solution=True, tables=False)
  not_optimum        column sets whose warm run did not end at `optimum`, beside the cold runs'
  pivots             warm against cold, summed over the sets

new and yardstick alternate in one process after a warm-up of each, five times, in two rounds;
every wall figure is (median, min, max) in seconds.  Before anything is timed the two answers are
compared: statuses, and the objectives where both runs end at `optimum` (they are two different
pivot sequences, so the last bits differ: the largest relative difference is reported).

    python tools/bench_batch_cols.py WORKLOAD [B [CAP]]     WORKLOAD: 100x100, 65x65 or ui
CAP replaces the workload's max_pivots: the 65 x 65 LPs need about 500 pivots, so at the series'
256 every base run ends at its cap and the warm runs merely carry on; at 1024 they start from optima.
Run the workloads as separate processes, one after another, one process at a time on one box;
`--out FILE` appends the line to FILE as well."""
import sys

from batch_bench_util import emit, pop_out, timed
from bench_batch_scenarios import events_ms
from bench_batch_solution import REPS, spread, workloads
import numpy as np
import torch

S, K, VIOL, PROB = 8, 1, 0.05, 0.75


def col_sets(tabs, dims, duals, seed=0):
    """cols [B][S][K][Rmax], ncols [B][S]: one new variable per set, the cost at entry n.  The
    reduced cost of a variable with coefficients a and cost c under the base answer is
    c - a . duals (the duals are the f-row entries over the non-basic slacks)."""
    B, Rmax, ldb = tabs.shape
    g = np.random.default_rng(seed)
    n, m = dims[:, 0].astype(np.int64), dims[:, 1].astype(np.int64)
    q = np.arange(B)
    rows = np.arange(Rmax)[None, :] < n[:, None]
    cols = np.arange(ldb)[None, :] < m[:, None]
    mean = (np.abs(tabs[q, n, :]) * cols).sum(1) / m
    a = g.normal(size=(B, S, Rmax)) * (g.random((B, S, Rmax)) < PROB) * rows[:, None, :]
    a[:, :, 0] = np.where(a.any(axis=2), a[:, :, 0], 1.0)
    du = np.zeros((B, Rmax))
    du[:, :duals.shape[1]] = np.nan_to_num(duals)
    d = VIOL * mean[:, None] * np.where(np.arange(S) % 2 == 0, 1.0, -1.0)[None, :]
    cost = (a * du[:, None, :]).sum(2) - d
    a[q[:, None], np.arange(S)[None, :], n[:, None]] = cost
    return a[:, :, None, :].copy(), np.full((B, S), K, dtype=np.int32)


def widened(tabs, dims, cols):
    """The B * S widened originals, set q = b * S + s: the variable as column m, "-b" right of
    it."""
    B, Rmax, ldb = tabs.shape
    out = np.zeros((B * S, Rmax, ldb + K))
    d = np.repeat(dims, S, axis=0)
    q = np.arange(B * S)
    m = d[:, 1].astype(np.int64)
    base = np.repeat(tabs, S, axis=0)
    out[:, :, :ldb] = base
    out[q, :, m + K] = base[q, :, m]
    out[q, :, m] = cols.reshape(B * S, Rmax)
    d[:, 1] += K
    d[:, 2] += K
    return out, d


def kernel_ms(entry, tabs, dims, cols, ncols, cap, reps):
    """k_batch_cols on the resident outputs of the base solve and k_batch_solution, by HIP events,
    beside smx_copy_probe on as many bytes."""
    from simplex_mi355x import _lib
    L = _lib.load()
    B, Rmax, ldb = tabs.shape
    Q, ldo, dev = B * S, ldb + K, "cuda"
    stream = torch.cuda.current_stream().cuda_stream
    dt, dd = torch.from_numpy(tabs).to(dev), torch.from_numpy(dims).to(dev)
    o = torch.empty_like(dt)
    rc = torch.zeros((B, cap, 2), dtype=torch.int32, device=dev)
    xv = torch.zeros((B, cap, 2), dtype=torch.float64, device=dev)
    st = torch.zeros(B, dtype=torch.int32, device=dev)
    npv = torch.zeros(B, dtype=torch.int32, device=dev)
    _lib.check(getattr(L, entry)(dt.data_ptr(), dd.data_ptr(), B, Rmax, ldb, cap, o.data_ptr(),
                                 rc.data_ptr(), xv.data_ptr(), None, st.data_ptr(),
                                 npv.data_ptr(), stream), entry)
    func = dt[torch.arange(B, device=dev), dd[:, 0].long()].contiguous()
    x = torch.empty((B, ldb), dtype=torch.float64, device=dev)
    du = torch.empty((B, Rmax), dtype=torch.float64, device=dev)
    obj = torch.empty(B, dtype=torch.float64, device=dev)
    ba = torch.empty((B, Rmax), dtype=torch.int32, device=dev)
    nb = torch.empty((B, ldb), dtype=torch.int32, device=dev)
    _lib.check(L.smx_batch_solution(o.data_ptr(), dd.data_ptr(), B, Rmax, ldb, cap, rc.data_ptr(),
                                    npv.data_ptr(), func.data_ptr(), x.data_ptr(), du.data_ptr(),
                                    obj.data_ptr(), ba.data_ptr(), nb.data_ptr(), stream),
               "smx_batch_solution")
    d_a, d_nc = torch.from_numpy(cols).to(dev), torch.from_numpy(ncols).to(dev)
    tv = torch.empty((Q, Rmax, ldo), dtype=torch.float64, device=dev)
    fv = torch.empty((Q, ldo), dtype=torch.float64, device=dev)
    dv = torch.empty((Q, 3), dtype=torch.int32, device=dev)
    bv = torch.empty((Q, Rmax), dtype=torch.int32, device=dev)
    nv = torch.empty((Q, ldo), dtype=torch.int32, device=dev)

    def run():
        _lib.check(L.smx_batch_cols(
            o.data_ptr(), dd.data_ptr(), B, S, Rmax, ldb, ba.data_ptr(), nb.data_ptr(),
            func.data_ptr(), d_a.data_ptr(), d_nc.data_ptr(), K, ldo, tv.data_ptr(), fv.data_ptr(),
            dv.data_ptr(), bv.data_ptr(), nv.data_ptr(), stream), "smx_batch_cols")
    ms = {"cols": events_ms(run, reps)}
    ms["cols_copy_GBps"] = 2 * tv.numel() * 8 / (ms["cols"] * 1e-3) / 1e9
    wo = torch.empty_like(tv)
    nd = (tv.numel() // 2) * 2
    ms["copy_probe_GBps"] = max(
        2 * nd * 8 / (events_ms(lambda v=v: _lib.check(L.smx_copy_probe(
            tv.data_ptr(), wo.data_ptr(), nd, v, stream), "smx_copy_probe"), reps) * 1e-3) / 1e9
        for v in (0, 1))
    return ms


def main():
    args = sys.argv[1:]
    out = pop_out(args)
    if not args or args[0] not in ("100x100", "65x65", "ui"):
        sys.exit(__doc__)
    B = int(args[1]) if len(args) > 1 else 2048
    from simplex_mi355x.batch import solve_batch_arrays, solve_batch_columns_arrays
    name, entry, cap, tabs, dims = next(w for w in workloads(B) if w[0] == args[0])
    cap = int(args[2]) if len(args) > 2 else cap
    base = solve_batch_arrays(tabs, dims, cap, solution=True, tables=False)
    cols, ncols = col_sets(tabs, dims, base["duals"])
    cold_tabs, cold_dims = widened(tabs, dims, cols)
    rec = {"what": "batch_cols", "workload": name, "lps": len(tabs), "sets": S, "cols_per_set": K,
           "shape": list(tabs.shape[1:]), "max_pivots": cap, "reps": REPS}

    def new():
        return solve_batch_columns_arrays(tabs, dims, cols, ncols, cap)

    def yardstick():
        return solve_batch_arrays(cold_tabs, cold_dims, cap, solution=True, tables=False)

    got, cold = new(), yardstick()                                             # warm, and compare
    wst, cst = got["status"].reshape(-1), cold["status"]
    both = (wst == 1) & (cst == 1)
    wobj, cobj = got["objective"].reshape(-1)[both], cold["objective"][both]
    rec["sets_total"] = int(wst.size)
    rec["base_not_optimum"] = int((got["base"]["status"] != 1).sum())
    rec["not_optimum"] = {"warm": int((wst != 1).sum()), "cold": int((cst != 1).sum()),
                          "warm_only": int(((wst != 1) & (cst == 1)).sum())}
    rec["same_status"] = int((wst == cst).sum())
    rec["no_warm_pivot"] = int((got["npivots"] == 0).sum())
    rel = np.abs(wobj - cobj) / np.maximum(np.abs(cobj), 1e-300)
    rec["objective_max_rel_diff"] = float(rel.max(initial=0.0))
    rec["objective_differs"] = {"both_optimum": int(both.sum()), "rel_above_1e-9": int((rel > 1e-9).sum())}
    rec["pivots"] = {"warm": int(got["npivots"].sum()), "cold": int(cold["npivots"].sum()),
                     "base": int(got["base"]["npivots"].sum())}
    rec["new"], rec["yardstick"] = [], []
    for _ in range(2):
        w_new, w_old = [], []
        for _ in range(REPS):
            w_new.append(timed(new, 1)[0])
            w_old.append(timed(yardstick, 1)[0])
        rec["new"].append(spread(w_new))
        rec["yardstick"].append(spread(w_old))
    rec["kernel_ms"] = kernel_ms(entry, tabs, dims, cols, ncols, cap, 10)
    rec["widened_bytes"] = int(cold_tabs.nbytes)
    emit(rec, out)


if __name__ == "__main__":
    main()
