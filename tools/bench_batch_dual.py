"""The dual-simplex warm rule against the reference rule on the workloads of DESIGN 9.6 and 9.7:
2048 uniform LPs of 65 x 65 (k_batch_wg; max_pivots 1024, where the base runs reach their optima,
and 256, where they end at the cap), 2048 of 100 x 100 (256) and 200 000 UI-shaped LPs (m = 2,
n = 3..20, k_batch, 64), each with S = 8 rhs-only scenarios at 5 % (bench_batch_scenarios' deltas
with the cost deltas zeroed, so that a table made from an optimum is dual feasible) or S = 8 cut
sets of one cut at 5 % (bench_batch_cuts').  Per workload and warm feature one JSON line:

  not_optimum   warm runs that did not end at `optimum`, per rule, beside the base runs that did not
  pivots        warm pivots summed over the sets, per rule
  kernel_ms     the warm solve kernel alone on resident warm tables by HIP events (10 launches
                after a warm-up launch), per rule
  wall          wall time of the whole call (solve_batch_scenarios_arrays / solve_batch_cuts_arrays,
                base solve included) per rule: (median, min, max) seconds of five calls, the two
                rules alternating, in two rounds
  agree         sets where both rules end at `optimum`, and the largest relative difference of
                their objectives (two different pivot sequences: the last bits differ)

    python tools/bench_batch_dual.py FEATURE WORKLOAD [B [CAP]]
        FEATURE: scenarios or cuts; WORKLOAD: 100x100, 65x65 or ui

In a tree without the rule (the parent commit, the yardstick of DESIGN 9.3's rule) the same
command times the same call without `warm_rule` and reports it as "reference" alone; run the two
trees alternating, one process at a time on one box; `--reference-only` makes this tree's process
the same sequence of calls as the parent's (the default path against the yardstick).  `--out FILE`
appends the line to FILE."""
import inspect
import sys

from batch_bench_util import emit, pop_out, timed
from bench_batch_cuts import cut_sets
from bench_batch_scenarios import deltas, events_ms
from bench_batch_solution import REPS, spread, workloads
import numpy as np
import torch

S = 8


def warm_tables(feature, L, tier_entry, tabs, dims, sets, cap):
    """The B * S warm tables of `feature` on the device, made once from the base run: (tables,
    their dims) as device tensors."""
    from simplex_mi355x import _lib
    B, Rmax, ldb = tabs.shape
    dev = "cuda"
    stream = torch.cuda.current_stream().cuda_stream
    dt, dd = torch.from_numpy(tabs).to(dev), torch.from_numpy(dims).to(dev)
    o = torch.empty_like(dt)
    rc = torch.zeros((B, cap, 2), dtype=torch.int32, device=dev)
    xv = torch.zeros((B, cap, 2), dtype=torch.float64, device=dev)
    st = torch.zeros(B, dtype=torch.int32, device=dev)
    npv = torch.zeros(B, dtype=torch.int32, device=dev)
    _lib.check(getattr(L, tier_entry)(dt.data_ptr(), dd.data_ptr(), B, Rmax, ldb, cap,
                                      o.data_ptr(), rc.data_ptr(), xv.data_ptr(), None,
                                      st.data_ptr(), npv.data_ptr(), stream), tier_entry)
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
    Q = B * S
    if feature == "scenarios":
        drhs, dcost = sets
        h_dr = np.zeros((B, S, Rmax))
        h_dr[:, :, :Rmax - 1] = drhs
        h_dc = np.zeros((B, S, ldb))
        h_dc[:, :, :ldb - 1] = dcost
        d_dr, d_dc = torch.from_numpy(h_dr).to(dev), torch.from_numpy(h_dc).to(dev)
        ts = torch.empty((Q, Rmax, ldb), dtype=torch.float64, device=dev)
        fs = torch.empty((Q, ldb), dtype=torch.float64, device=dev)
        ds = torch.empty((Q, 3), dtype=torch.int32, device=dev)
        _lib.check(L.smx_batch_scenario(
            o.data_ptr(), dd.data_ptr(), B, S, Rmax, ldb, ba.data_ptr(), nb.data_ptr(),
            func.data_ptr(), d_dr.data_ptr(), d_dc.data_ptr(), ts.data_ptr(), fs.data_ptr(),
            ds.data_ptr(), stream), "smx_batch_scenario")
    else:
        cuts, ncuts = sets
        K = cuts.shape[2]
        d_g, d_nc = torch.from_numpy(cuts).to(dev), torch.from_numpy(ncuts).to(dev)
        ts = torch.empty((Q, Rmax + K, ldb), dtype=torch.float64, device=dev)
        ds = torch.empty((Q, 3), dtype=torch.int32, device=dev)
        bc = torch.empty((Q, Rmax + K), dtype=torch.int32, device=dev)
        _lib.check(L.smx_batch_cuts(
            o.data_ptr(), dd.data_ptr(), B, S, Rmax, ldb, ba.data_ptr(), nb.data_ptr(),
            d_g.data_ptr(), d_nc.data_ptr(), K, Rmax + K, ts.data_ptr(), ds.data_ptr(),
            bc.data_ptr(), stream), "smx_batch_cuts")
    torch.cuda.synchronize()
    return ts, ds


def warm_kernel_ms(L, entry, rule, ts, ds, cap, reps):
    """The warm solve kernel of `entry` on the resident warm tables, by HIP events; rule None is
    the entry without a rule (the only one a tree without the rule has)."""
    from simplex_mi355x import _lib
    Q, rows, ldb = ts.shape
    dev = "cuda"
    stream = torch.cuda.current_stream().cuda_stream
    wo = torch.empty_like(ts)
    rc = torch.zeros((Q, cap, 2), dtype=torch.int32, device=dev)
    xv = torch.zeros((Q, cap, 2), dtype=torch.float64, device=dev)
    st = torch.zeros(Q, dtype=torch.int32, device=dev)
    npv = torch.zeros(Q, dtype=torch.int32, device=dev)
    args = (ts.data_ptr(), ds.data_ptr(), Q, rows, ldb, cap, wo.data_ptr(), rc.data_ptr(),
            xv.data_ptr(), None, st.data_ptr(), npv.data_ptr())
    if rule is None:
        return events_ms(lambda: _lib.check(getattr(L, entry)(*args, stream), entry), reps)
    name = entry + "_rule"
    return events_ms(lambda: _lib.check(getattr(L, name)(*args, rule, stream), name), reps)


def main():
    args = sys.argv[1:]
    out = pop_out(args)
    reference_only = "--reference-only" in args
    args = [a for a in args if a != "--reference-only"]
    if len(args) < 2 or args[0] not in ("scenarios", "cuts") or \
            args[1] not in ("100x100", "65x65", "ui"):
        sys.exit(__doc__)
    feature = args[0]
    B = int(args[2]) if len(args) > 2 else 2048
    from simplex_mi355x import _lib, batch
    name, entry, cap, tabs, dims = next(w for w in workloads(B) if w[0] == args[1])
    cap = int(args[3]) if len(args) > 3 else cap
    call = (batch.solve_batch_scenarios_arrays if feature == "scenarios"
            else batch.solve_batch_cuts_arrays)
    has_rule = "warm_rule" in inspect.signature(call).parameters and not reference_only
    rules = ("reference", "dual") if has_rule else ("reference",)
    base = batch.solve_batch_arrays(tabs, dims, cap, solution=True, tables=False)
    if feature == "scenarios":
        drhs, dcost = deltas(tabs, dims)
        sets = (drhs, np.zeros_like(dcost))                  # rhs-only
    else:
        sets = cut_sets(tabs, dims, base["x"])

    def run(rule):
        kw = {"warm_rule": rule} if has_rule else {}
        return call(tabs, dims, *sets, cap, **kw)

    rec = {"what": "batch_dual", "feature": feature, "workload": name, "lps": len(tabs), "sets": S,
           "shape": list(tabs.shape[1:]), "max_pivots": cap, "reps": REPS, "rules": list(rules),
           "base_not_optimum": int((base["status"] != 1).sum())}
    got = {rule: run(rule) for rule in rules}                # warm-up of each, and the census
    rec["sets_total"] = int(got["reference"]["status"].size)
    rec["not_optimum"] = {r: int((got[r]["status"] != 1).sum()) for r in rules}
    rec["at_cap"] = {r: int((got[r]["status"] == 0).sum()) for r in rules}
    rec["pivots"] = {r: int(got[r]["npivots"].sum()) for r in rules}
    if has_rule:
        a, b = got["reference"], got["dual"]
        both = (a["status"] == 1) & (b["status"] == 1)
        rel = np.abs(a["objective"][both] - b["objective"][both]) / \
            np.maximum(np.abs(a["objective"][both]), 1e-300)
        rec["agree"] = {"both_optimum": int(both.sum()),
                        "dual_only": int(((a["status"] != 1) & (b["status"] == 1)).sum()),
                        "reference_only": int(((a["status"] == 1) & (b["status"] != 1)).sum()),
                        "objective_max_rel_diff": float(rel.max(initial=0.0)),
                        "rel_above_1e-9": int((rel > 1e-9).sum())}
    rec["wall"] = {r: [] for r in rules}
    for _ in range(2):
        walls = {r: [] for r in rules}
        for _ in range(REPS):
            for r in rules:
                walls[r].append(timed(lambda r=r: run(r), 1)[0])
        for r in rules:
            rec["wall"][r].append(spread(walls[r]))
    L = _lib.load()
    ts, ds = warm_tables(feature, L, entry, tabs, dims, sets, cap)
    warm_entry = entry
    if feature == "cuts" and ts.shape[1] > 64 and entry == "smx_batch_solve":
        warm_entry = "smx_batch_solve_wg"
    rec["kernel_ms"] = {"reference": warm_kernel_ms(L, warm_entry, None, ts, ds, cap, 10)}
    if has_rule:
        rec["kernel_ms"]["reference_rule_entry"] = warm_kernel_ms(L, warm_entry, 0, ts, ds, cap, 10)
        rec["kernel_ms"]["dual"] = warm_kernel_ms(L, warm_entry, 1, ts, ds, cap, 10)
    emit(rec, out)


if __name__ == "__main__":
    main()
