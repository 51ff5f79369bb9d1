"""Sensitivity ranges from a batch without the tables: 2048 uniform LPs of 100 x 100 and of 65 x 65
(k_batch_wg, max_pivots = 256) and 200 000 UI-shaped LPs (m = 2, n = 3..20, k_batch, 64).  Per
workload one JSON line:

  kernel_ms          k_batch_ranging alone on resident buffers by HIP events (10 launches after a
                     warm-up launch), beside the solve kernel and k_batch_solution
  new                wall time of solve_batch_arrays(solution=True, ranging=True, tables=False)
  yardstick          what a caller does without it: the default solve_batch_arrays call, which
                     copies every final table back, plus a numpy replay of rc to the labels, plus
                     the rules of include/smx.h on `final` (ranges_on_host below, vectorised over
                     the batch)

new and yardstick alternate in one process after a warm-up of each, five times; every wall figure
is (median, min, max) in seconds.  The two answers are compared bit for bit before anything is
reported.

    python tools/bench_batch_ranging.py WORKLOAD [B]     WORKLOAD: 100x100, 65x65 or ui
Run the three workloads as three processes, one after another, one process at a time on one box;
`--out FILE` appends the line to FILE as well."""
import sys

from batch_bench_util import emit, pop_out, timed
from bench_batch_solution import REPS, kernels_ms, spread, workloads
import numpy as np
import torch

MASK63 = np.int64(0x7FFFFFFFFFFFFFFF)
INF = np.float64(np.inf)


def key(q):
    """float64 -> int64 in the contract's total order (-0.0 below +0.0); its own inverse."""
    b = np.ascontiguousarray(q).view(np.int64)
    return b ^ ((b >> 63) & MASK63)


def fold(q, mask, axis, smallest):
    """The ordered minimum / maximum of q where mask, along axis: +inf / -inf without a candidate,
    NaN with a NaN candidate."""
    none = key(np.array(INF if smallest else -INF))
    k = np.where(mask, key(q), none)
    k = k.min(axis) if smallest else k.max(axis)
    out = (k ^ ((k >> 63) & MASK63)).view(np.float64)
    out[(np.isnan(q) & mask).any(axis)] = np.nan
    return out


def labels_on_host(dims, out, Rmax, ldb):
    """basis [B][Rmax], nonbasis [B][ldb] from the pivot log, the whole batch at once."""
    B = len(dims)
    m = dims[:, 1].astype(np.int64)
    rows = np.arange(B)
    basis = m[:, None] + np.arange(Rmax)[None, :]
    nonbasis = np.tile(np.arange(ldb), (B, 1))
    rc, npiv = out["rc"], out["npivots"]
    for s in range(int(npiv.max(initial=0))):
        act = rows[npiv > s]
        r, c = rc[act, s, 0], rc[act, s, 1]
        basis[act, r], nonbasis[act, c] = nonbasis[act, c], basis[act, r]
    return basis, nonbasis


def ranges_on_host(dims, final, basis, nonbasis):
    """The four arrays ([B][Rmax - 1] / [B][ldb - 1]) by the rules of include/smx.h."""
    B, Rmax, ldb = final.shape
    n, m = dims[:, 0].astype(np.int64), dims[:, 1].astype(np.int64)
    q_ = np.arange(B)
    rowm = np.arange(Rmax)[None, :] < n[:, None]
    colm = np.arange(ldb)[None, :] < m[:, None]
    bcol = final[q_, :, m]                                   # [B][Rmax]: the "-b" column
    frow = final[q_, n, :]                                   # [B][ldb]: the f-row
    inside = rowm[:, :, None] & colm[:, None, :]
    pos, neg = (final > 0) & inside, (final < 0) & inside
    with np.errstate(all="ignore"):
        q = bcol[:, :, None] / final
        col_hi, col_lo = fold(q, pos, 1, True), fold(q, neg, 1, False)
        q = (-frow)[:, None, :] / final
        row_lo, row_hi = fold(q, pos, 2, False), fold(q, neg, 2, True)
    rhs_lo, rhs_hi = np.zeros((B, Rmax)), np.zeros((B, Rmax))
    cost_lo, cost_hi = np.zeros((B, ldb)), np.zeros((B, ldb))
    slack = colm & (nonbasis >= m[:, None])
    b, j = np.nonzero(slack)
    rhs_lo[b, nonbasis[b, j] - m[b]], rhs_hi[b, nonbasis[b, j] - m[b]] = col_lo[b, j], col_hi[b, j]
    b, j = np.nonzero(colm & ~slack)
    cost_lo[b, nonbasis[b, j]], cost_hi[b, nonbasis[b, j]] = -frow[b, j], INF
    slack = rowm & (basis >= m[:, None])
    b, p = np.nonzero(slack)
    rhs_lo[b, basis[b, p] - m[b]], rhs_hi[b, basis[b, p] - m[b]] = -bcol[b, p], INF
    b, p = np.nonzero(rowm & ~slack)
    cost_lo[b, basis[b, p]], cost_hi[b, basis[b, p]] = row_lo[b, p], row_hi[b, p]
    return {"rhs_lo": rhs_lo[:, :Rmax - 1], "rhs_hi": rhs_hi[:, :Rmax - 1],
            "cost_lo": cost_lo[:, :ldb - 1], "cost_hi": cost_hi[:, :ldb - 1]}


def ranging_ms(entry, tabs, dims, cap, reps):
    """k_batch_ranging on the resident outputs of `entry` and k_batch_solution, by HIP events: one
    warm-up launch, then `reps` back to back."""
    from simplex_mi355x import _lib
    L = _lib.load()
    B, Rmax, ldb = tabs.shape
    dev = "cuda"
    dt, dd = torch.from_numpy(tabs).to(dev), torch.from_numpy(dims).to(dev)
    o = torch.empty_like(dt)
    rc = torch.zeros((B, cap, 2), dtype=torch.int32, device=dev)
    xv = torch.zeros((B, cap, 2), dtype=torch.float64, device=dev)
    st = torch.zeros(B, dtype=torch.int32, device=dev)
    npv = torch.zeros(B, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    func = dt[torch.arange(B, device=dev), dd[:, 0].long()].contiguous()
    x = torch.empty((B, ldb), dtype=torch.float64, device=dev)
    du = torch.empty((B, Rmax), dtype=torch.float64, device=dev)
    obj = torch.empty(B, dtype=torch.float64, device=dev)
    ba = torch.empty((B, Rmax), dtype=torch.int32, device=dev)
    nb = torch.empty((B, ldb), dtype=torch.int32, device=dev)
    rl, rh = (torch.empty((B, Rmax), dtype=torch.float64, device=dev) for _ in "lh")
    cl, ch = (torch.empty((B, ldb), dtype=torch.float64, device=dev) for _ in "lh")
    _lib.check(getattr(L, entry)(dt.data_ptr(), dd.data_ptr(), B, Rmax, ldb, cap, o.data_ptr(),
                                 rc.data_ptr(), xv.data_ptr(), None, st.data_ptr(),
                                 npv.data_ptr(), stream), entry)
    _lib.check(L.smx_batch_solution(o.data_ptr(), dd.data_ptr(), B, Rmax, ldb, cap, rc.data_ptr(),
                                    npv.data_ptr(), func.data_ptr(), x.data_ptr(), du.data_ptr(),
                                    obj.data_ptr(), ba.data_ptr(), nb.data_ptr(), stream),
               "smx_batch_solution")
    a = (o.data_ptr(), dd.data_ptr(), B, Rmax, ldb, ba.data_ptr(), nb.data_ptr(), rl.data_ptr(),
         rh.data_ptr(), cl.data_ptr(), ch.data_ptr(), stream)
    _lib.check(L.smx_batch_ranging(*a), "smx_batch_ranging")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        L.smx_batch_ranging(*a)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64),
                          np.ascontiguousarray(b).view(np.int64))


def main():
    args = sys.argv[1:]
    out = pop_out(args)
    if not args or args[0] not in ("100x100", "65x65", "ui"):
        sys.exit(__doc__)
    B = int(args[1]) if len(args) > 1 else 2048
    from simplex_mi355x.batch import solve_batch_arrays
    name, entry, cap, tabs, dims = next(w for w in workloads(B) if w[0] == args[0])
    rec = {"what": "batch_ranging", "workload": name, "lps": len(tabs),
           "shape": list(tabs.shape[1:]), "max_pivots": cap, "reps": REPS}

    def new():
        return solve_batch_arrays(tabs, dims, cap, solution=True, ranging=True, tables=False)

    def yardstick():
        res = solve_batch_arrays(tabs, dims, cap)
        basis, nonbasis = labels_on_host(dims, res, *tabs.shape[1:])
        return res, ranges_on_host(dims, res["final"], basis, nonbasis)

    got = new()                                                                # warm, and compare
    res, host = yardstick()
    assert "final" not in got and np.array_equal(got["rc"], res["rc"])
    nans = 0
    for f, h in host.items():
        nans += int(np.isnan(h).sum())
        assert same(got[f], h), f"the two answers differ in {f}"
    rec["nan_bounds"] = nans
    rec["finite_two_ended"] = int(
        (np.isfinite(host["rhs_lo"]) & np.isfinite(host["rhs_hi"])).sum()
        + (np.isfinite(host["cost_lo"]) & np.isfinite(host["cost_hi"])).sum())
    w_new, w_old = [], []
    for _ in range(REPS):
        w_new.append(timed(new, 1)[0])
        w_old.append(timed(yardstick, 1)[0])
    rec["new"], rec["yardstick"] = spread(w_new), spread(w_old)
    kms, sms, pivots = kernels_ms(entry, tabs, dims, cap, 10)
    rec["kernel_ms"] = {"solve": kms, "solution": sms,
                        "ranging": ranging_ms(entry, tabs, dims, cap, 10)}
    rec["pivots"] = pivots
    rec["final_bytes"] = int(tabs.nbytes)
    emit(rec, out)


if __name__ == "__main__":
    main()
