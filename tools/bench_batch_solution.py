"""Whole solutions from a batch without the tables: 2048 uniform LPs of 100 x 100 and of 65 x 65
(k_batch_wg, max_pivots = 256) and 200 000 UI-shaped LPs (m = 2, n = 3..20, k_batch, 64).  Per
workload one JSON line:

  kernel_ms          the solve kernel and k_batch_solution on resident buffers by HIP events
                     (10 launches each after a warm-up launch)
  new                wall time of solve_batch_arrays(solution=True, tables=False)
  yardstick          what a caller does without it: the default solve_batch_arrays call, which
                     copies every final table back, plus a numpy replay of rc to the same x and
                     objective (replay_on_host below, vectorised over the batch)
  default_call       the untouched default call alone

new and yardstick alternate in one process after a warm-up of each, five times; every wall figure
is (median, min, max) in seconds.  The two answers are compared bit for bit before anything is
reported.

    python tools/bench_batch_solution.py [B]           the lines above
    python tools/bench_batch_solution.py --default     only default_call (runs on a commit without
                                                       k_batch_solution too: the before / after)
Run one process at a time on one box; `--out FILE` appends the lines to FILE as well."""
import sys

from batch_bench_util import CAP, emit, pop_out, tables, timed
import numpy as np
import torch

REPS = 5


def ui_tables(B, seed=0):
    """The UI's shape (main.py:309-313): m = 2, n = 3..20, as tools/bench_batch.py draws them."""
    rng = np.random.default_rng(seed)
    n = rng.integers(3, 21, size=B)
    tabs = np.zeros((B, 21, 3))
    tabs[:, :20, :2] = rng.uniform(-50, 50, size=(B, 20, 2))
    tabs[:, :20, 2] = rng.uniform(-100, 400, size=(B, 20))
    tabs[np.arange(21)[None, :] >= n[:, None]] = 0.0
    tabs[np.arange(B), n, :2] = rng.uniform(-3, 3, size=(B, 2))
    dims = np.stack([n, np.full(B, 2), np.full(B, 2)], axis=1).astype(np.int32)
    return tabs, dims


def replay_on_host(tabs, dims, out):
    """x [B][ldb - 1] and objective [B] from the default call's final tables and pivot log: the
    labels replayed step by step for the whole batch at once, x gathered from the "-b" column,
    the objective summed left to right (the same roundings as the device)."""
    B, Rmax, ldb = tabs.shape
    n, m = dims[:, 0].astype(np.int64), dims[:, 1].astype(np.int64)
    rows = np.arange(B)
    basis = m[:, None] + np.arange(Rmax)[None, :]
    nonbasis = np.tile(np.arange(ldb), (B, 1))
    rc, npiv = out["rc"], out["npivots"]
    for s in range(int(npiv.max(initial=0))):
        act = rows[npiv > s]
        r, c = rc[act, s, 0], rc[act, s, 1]
        basis[act, r], nonbasis[act, c] = nonbasis[act, c], basis[act, r]
    x = np.zeros((B, ldb))
    i = np.arange(Rmax)[None, :]
    basic = (i < n[:, None]) & (basis < m[:, None])
    bq, bi = np.nonzero(basic)
    x[bq, basis[bq, bi]] = out["final"][bq, bi, m[bq]]
    p = tabs[rows, n] * x
    obj = p[:, 0].copy()
    for k in range(1, int(m.max())):
        obj = np.where(k < m, obj + p[:, k], obj)
    return x[:, :ldb - 1], obj


def spread(walls):
    return [float(np.median(walls)), float(min(walls)), float(max(walls))]


def kernels_ms(entry, tabs, dims, cap, reps):
    """The solve kernel `entry` and then k_batch_solution on its resident outputs, each by HIP
    events: one warm-up launch, then `reps` back to back.  Returns (solve ms, solution ms, pivots
    of one launch)."""
    from simplex_mi355x import _lib
    L = _lib.load()
    B, Rmax, ldb = tabs.shape
    dt, dd = torch.from_numpy(tabs).cuda(), torch.from_numpy(dims).cuda()
    o = torch.empty_like(dt)
    rc = torch.zeros((B, cap, 2), dtype=torch.int32, device="cuda")
    xv = torch.zeros((B, cap, 2), dtype=torch.float64, device="cuda")
    st = torch.zeros(B, dtype=torch.int32, device="cuda")
    npv = torch.zeros(B, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    func = dt[torch.arange(B, device="cuda"), dd[:, 0].long()].contiguous()
    x = torch.empty((B, ldb), dtype=torch.float64, device="cuda")
    du = torch.empty((B, Rmax), dtype=torch.float64, device="cuda")
    obj = torch.empty(B, dtype=torch.float64, device="cuda")
    ba = torch.empty((B, Rmax), dtype=torch.int32, device="cuda")
    nb = torch.empty((B, ldb), dtype=torch.int32, device="cuda")
    calls = ((getattr(L, entry), entry,
              (dt.data_ptr(), dd.data_ptr(), B, Rmax, ldb, cap, o.data_ptr(), rc.data_ptr(),
               xv.data_ptr(), None, st.data_ptr(), npv.data_ptr(), stream)),
             (L.smx_batch_solution, "smx_batch_solution",
              (o.data_ptr(), dd.data_ptr(), B, Rmax, ldb, cap, rc.data_ptr(), npv.data_ptr(),
               func.data_ptr(), x.data_ptr(), du.data_ptr(), obj.data_ptr(), ba.data_ptr(),
               nb.data_ptr(), stream)))
    ms = []
    for fn, what, a in calls:
        _lib.check(fn(*a), what)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn(*a)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    return ms[0], ms[1], int(npv.sum().item())


def workloads(B):
    return (("100x100", "smx_batch_solve_wg", CAP) + tables(B, 100, 100),
            ("65x65", "smx_batch_solve_wg", CAP) + tables(B, 65, 65),
            ("ui", "smx_batch_solve", 64) + ui_tables(200000 if B == 2048 else 100 * B))


def main():
    args = sys.argv[1:]
    out = pop_out(args)
    default_only = "--default" in args
    args = [a for a in args if a != "--default"]
    B = int(args[0]) if args else 2048
    from simplex_mi355x.batch import solve_batch_arrays
    for name, entry, cap, tabs, dims in workloads(B):
        rec = {"what": "batch_solution", "workload": name, "lps": len(tabs),
               "shape": list(tabs.shape[1:]), "max_pivots": cap, "reps": REPS}
        solve_batch_arrays(tabs, dims, cap)                                    # warm
        walls = [timed(lambda: solve_batch_arrays(tabs, dims, cap), 1)[0] for _ in range(REPS)]
        rec["default_call"] = spread(walls)
        if default_only:
            rec["what"] = "batch_default_call"
            emit(rec, out)
            continue

        def new():
            return solve_batch_arrays(tabs, dims, cap, solution=True, tables=False)

        def yardstick():
            res = solve_batch_arrays(tabs, dims, cap)
            return res, replay_on_host(tabs, dims, res)

        got = new()                                                            # warm, and compare
        res, (x, obj) = yardstick()
        assert "final" not in got and np.array_equal(got["rc"], res["rc"])

        def same(a, b):
            return np.array_equal(np.ascontiguousarray(a).view(np.int64),
                                  np.ascontiguousarray(b).view(np.int64))
        assert same(got["x"], x) and same(got["objective"], obj), "the two answers differ"
        w_new, w_old = [], []
        for _ in range(REPS):
            w_new.append(timed(new, 1)[0])
            w_old.append(timed(yardstick, 1)[0])
        rec["new"], rec["yardstick"] = spread(w_new), spread(w_old)
        kms, sms, pivots = kernels_ms(entry, tabs, dims, cap, 10)
        rec["kernel_ms"] = {"solve": kms, "solution": sms}
        rec["pivots"] = pivots
        rec["final_bytes"] = int(tabs.nbytes)
        emit(rec, out)


if __name__ == "__main__":
    main()
