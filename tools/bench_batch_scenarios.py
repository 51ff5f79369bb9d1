"""What-if scenarios from a batch: 2048 uniform LPs of 100 x 100 and of 65 x 65 (k_batch_wg,
max_pivots = 256) and 200 000 UI-shaped LPs (m = 2, n = 3..20, k_batch, 64), each with S = 8
scenarios (normal deltas of 5 % of the mean constant / cost on a quarter of the entries).  Per
workload one JSON line:

  kernel_ms          k_batch_scenario alone on resident buffers by HIP events (10 launches after a
                     warm-up launch) with the bytes per second of the copy it contains (one read
                     and one write of every scenario table) and smx_copy_probe's rate on as many
                     bytes, beside the warm solve kernel on the
                     scenario tables and the cold solve kernel on the perturbed originals
  new                wall time of solve_batch_scenarios_arrays (base solve included)
  yardstick          what a caller does without it: the B * S perturbed originals through
                     solve_batch_arrays(solution=True, tables=False)
  not_optimum        scenarios whose warm run did not end at `optimum`, beside the cold runs'
  pivots             warm against cold, summed over the scenarios

new and yardstick alternate in one process after a warm-up of each, five times, in two rounds;
every wall figure is (median, min, max) in seconds.  Before anything is timed the two answers are
compared: statuses, and the objectives where both runs end at `optimum` (they are two different
pivot sequences, so the last bits differ: the largest relative difference is reported).

    python tools/bench_batch_scenarios.py WORKLOAD [B [CAP]]     WORKLOAD: 100x100, 65x65 or ui
CAP replaces the workload's max_pivots: the 65 x 65 LPs need about 500 pivots, so at the series'
256 every base run ends at its cap and the warm runs merely carry on; at 1024 they start from optima.
Run the three workloads as three processes, one after another, one process at a time on one box;
`--out FILE` appends the line to FILE as well."""
import sys

from batch_bench_util import emit, pop_out, timed
from bench_batch_solution import REPS, spread, workloads
import numpy as np
import torch

S, FRAC, PROB = 8, 0.05, 0.25


def deltas(tabs, dims, seed=0):
    """drhs [B][S][Rmax - 1], dcost [B][S][ldb - 1]: per LP scaled by the mean magnitude of its
    constants / costs, exact zeros on three quarters of the entries and past n / m."""
    B, Rmax, ldb = tabs.shape
    g = np.random.default_rng(seed)
    n, m = dims[:, 0].astype(np.int64), dims[:, 1].astype(np.int64)
    rows = np.arange(Rmax - 1)[None, :] < n[:, None]
    cols = np.arange(ldb - 1)[None, :] < m[:, None]
    q = np.arange(B)
    sr = (np.abs(tabs[q, :Rmax - 1, m]) * rows).sum(1) / n
    sc = (np.abs(tabs[q, n, :ldb - 1]) * cols).sum(1) / m
    drhs = g.normal(size=(B, S, Rmax - 1)) * (g.random((B, S, Rmax - 1)) < PROB)
    dcost = g.normal(size=(B, S, ldb - 1)) * (g.random((B, S, ldb - 1)) < PROB)
    return (drhs * (FRAC * sr)[:, None, None] * rows[:, None, :],
            dcost * (FRAC * sc)[:, None, None] * cols[:, None, :])


def perturbed(tabs, dims, drhs, dcost):
    """The B * S perturbed originals, scenario q = b * S + s."""
    B, Rmax, ldb = tabs.shape
    out = np.repeat(tabs, S, axis=0)
    d = np.repeat(dims, S, axis=0)
    q = np.arange(B * S)
    n, m = d[:, 0].astype(np.int64), d[:, 1].astype(np.int64)
    for i in range(Rmax - 1):
        out[q, i, m] += drhs.reshape(B * S, -1)[:, i]
    for k in range(ldb - 1):
        out[q, n, k] += dcost.reshape(B * S, -1)[:, k]
    return out, d


def events_ms(call, reps):
    call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def kernels_ms(entry, tabs, dims, drhs, dcost, cold_tabs, cold_dims, cap, reps):
    """k_batch_scenario on the resident outputs of the base solve and k_batch_solution, the warm
    solve on its tables and the cold solve on the perturbed originals, each by HIP events."""
    from simplex_mi355x import _lib
    L = _lib.load()
    B, Rmax, ldb = tabs.shape
    Q = B * S
    dev = "cuda"
    stream = torch.cuda.current_stream().cuda_stream

    def solver(count):
        rc = torch.zeros((count, cap, 2), dtype=torch.int32, device=dev)
        xv = torch.zeros((count, cap, 2), dtype=torch.float64, device=dev)
        st = torch.zeros(count, dtype=torch.int32, device=dev)
        npv = torch.zeros(count, dtype=torch.int32, device=dev)

        def run(d_in, d_dims, d_out):
            _lib.check(getattr(L, entry)(d_in.data_ptr(), d_dims.data_ptr(), count, Rmax, ldb,
                                         cap, d_out.data_ptr(), rc.data_ptr(), xv.data_ptr(),
                                         None, st.data_ptr(), npv.data_ptr(), stream), entry)
        return run, rc, npv

    dt, dd = torch.from_numpy(tabs).to(dev), torch.from_numpy(dims).to(dev)
    o = torch.empty_like(dt)
    run, rc, npv = solver(B)
    run(dt, dd, o)
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
    h_dr = np.zeros((B, S, Rmax))
    h_dr[:, :, :Rmax - 1] = drhs
    h_dc = np.zeros((B, S, ldb))
    h_dc[:, :, :ldb - 1] = dcost
    d_dr, d_dc = torch.from_numpy(h_dr).to(dev), torch.from_numpy(h_dc).to(dev)
    ts = torch.empty((Q, Rmax, ldb), dtype=torch.float64, device=dev)
    fs = torch.empty((Q, ldb), dtype=torch.float64, device=dev)
    ds = torch.empty((Q, 3), dtype=torch.int32, device=dev)

    def scenario():
        _lib.check(L.smx_batch_scenario(
            o.data_ptr(), dd.data_ptr(), B, S, Rmax, ldb, ba.data_ptr(), nb.data_ptr(),
            func.data_ptr(), d_dr.data_ptr(), d_dc.data_ptr(), ts.data_ptr(), fs.data_ptr(),
            ds.data_ptr(), stream), "smx_batch_scenario")
    ms = {"scenario": events_ms(scenario, reps)}
    ms["scenario_copy_GBps"] = 2 * ts.numel() * 8 / (ms["scenario"] * 1e-3) / 1e9
    wo = torch.empty_like(ts)
    # the box's plain streaming copy of as many bytes (it reads all of them from HBM, the kernel
    # reads each base table once per S scenarios)
    nd = (ts.numel() // 2) * 2
    ms["copy_probe_GBps"] = max(
        2 * nd * 8 / (events_ms(lambda v=v: _lib.check(L.smx_copy_probe(
            ts.data_ptr(), wo.data_ptr(), nd, v, stream), "smx_copy_probe"), reps) * 1e-3) / 1e9
        for v in (0, 1))
    wrun, _, _ = solver(Q)
    ms["warm_solve"] = events_ms(lambda: wrun(ts, ds, wo), reps)
    ct, cd = torch.from_numpy(cold_tabs).to(dev), torch.from_numpy(cold_dims).to(dev)
    ms["cold_solve"] = events_ms(lambda: wrun(ct, cd, wo), reps)
    return ms


def main():
    args = sys.argv[1:]
    out = pop_out(args)
    if not args or args[0] not in ("100x100", "65x65", "ui"):
        sys.exit(__doc__)
    B = int(args[1]) if len(args) > 1 else 2048
    from simplex_mi355x.batch import solve_batch_arrays, solve_batch_scenarios_arrays
    name, entry, cap, tabs, dims = next(w for w in workloads(B) if w[0] == args[0])
    cap = int(args[2]) if len(args) > 2 else cap
    drhs, dcost = deltas(tabs, dims)
    cold_tabs, cold_dims = perturbed(tabs, dims, drhs, dcost)
    rec = {"what": "batch_scenarios", "workload": name, "lps": len(tabs), "scenarios": S,
           "shape": list(tabs.shape[1:]), "max_pivots": cap, "reps": REPS}

    def new():
        return solve_batch_scenarios_arrays(tabs, dims, drhs, dcost, cap)

    def yardstick():
        return solve_batch_arrays(cold_tabs, cold_dims, cap, solution=True, tables=False)

    got, cold = new(), yardstick()                                             # warm, and compare
    wst, cst = got["status"].reshape(-1), cold["status"]
    both = (wst == 1) & (cst == 1)
    wobj, cobj = got["objective"].reshape(-1)[both], cold["objective"][both]
    rec["scenarios_total"] = int(wst.size)
    rec["base_not_optimum"] = int((got["base"]["status"] != 1).sum())
    rec["not_optimum"] = {"warm": int((wst != 1).sum()), "cold": int((cst != 1).sum()),
                          "warm_only": int(((wst != 1) & (cst == 1)).sum())}
    rec["same_status"] = int((wst == cst).sum())
    rec["objective_max_rel_diff"] = float(
        (np.abs(wobj - cobj) / np.maximum(np.abs(cobj), 1e-300)).max(initial=0.0))
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
    rec["kernel_ms"] = kernels_ms(entry, tabs, dims, drhs, dcost, cold_tabs, cold_dims, cap, 10)
    rec["scenario_bytes"] = int(cold_tabs.nbytes)
    emit(rec, out)


if __name__ == "__main__":
    main()
