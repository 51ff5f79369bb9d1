"""Integer programs from a batch: 2048 uniform LPs of 65 x 65 (k_batch_wg, max_pivots = 1024, so
that the trees start from optima) and 200 000 UI-shaped LPs (m = 2, n = 3..20, k_batch, 64), every
variable held to a whole number, max_depth = DEPTH.  Per workload one JSON line:

  kernel_ms          k_batch_branch_pick and k_batch_branch alone on the resident outputs of the
                     root solve by HIP events (10 launches after a warm-up launch; every root is
                     expanded on its picked row), the branch kernel's bytes per second (one read
                     of a parent's block, two writes of a child's) beside smx_copy_probe's rate on
                     as many bytes
  new                wall time of solve_batch_integer_arrays (root solve included)
  yardstick          the same tree driven from the host with the calls that exist without it:
                     every level's children as enlarged ORIGINAL problems (their bound rows
                     appended), solved cold through solve_batch_arrays(rule="dual", solution=True,
                     tables=False); the pick is read off x on the host, a child at SMX_INCORRECT
                     counts as empty
  statuses, nodes    of both, and the pivots: warm (all but the roots) against cold

new and yardstick alternate in one process after a warm-up of each, five times, in two rounds;
every wall figure is (median, min, max) in seconds.  The two walk different pivot sequences and
the yardstick cannot see how far a constant stands below zero, so their trees need not be equal:
the objectives are compared where both end "optimal".

    python tools/bench_batch_branch.py WORKLOAD [B [CAP [DEPTH]]]     WORKLOAD: 65x65 or ui
Run the workloads as separate processes, one after another, one process at a time on one box;
`--out FILE` appends the line to FILE as well."""
import sys

from batch_bench_util import emit, pop_out, timed
from bench_batch_scenarios import events_ms
from bench_batch_solution import REPS, spread, workloads
import numpy as np
import torch

TOL = 1e-6


def host_pick(x, m):
    """(bvar [Q]) read off x [Q][ldb-1]: the variable furthest from a whole number, ties to the
    lowest code; -1 where none is further than TOL."""
    lo = np.floor(x)
    d = np.minimum(x - lo, (lo + 1.0) - x)
    d = np.where((np.arange(x.shape[1])[None, :] < m[:, None]) & (d > TOL), d, -1.0)
    k = d.argmax(axis=1)
    return np.where(d[np.arange(len(x)), k] > 0, k, -1)


def yardstick_tree(tabs, dims, cap, depth, max_nodes):
    """The tree of branch.Tree on cold solves of enlarged originals; returns (answers, cold
    pivots)."""
    from simplex_mi355x import _lib, branch
    from simplex_mi355x.batch import solve_batch_arrays
    B, Rmax, ldb = tabs.shape
    tree = branch.Tree(B, depth, max_nodes, TOL)
    out = solve_batch_arrays(tabs, dims, cap, solution=True, tables=False)
    names = ["optimum" if s == _lib.OPTIMUM else "cap" if s == _lib.PIVOT else "error"
             for s in out["status"]]
    live = tree.start(names)
    frontier = [(k, k, float(out["objective"][k])) for k in live]
    cur_t = np.zeros((B, Rmax + depth, ldb))
    cur_t[:, :Rmax] = tabs
    cur_d, lp, x = dims.copy(), np.arange(B), out["x"]
    cold, level = 0, 0
    while frontier:
        bvar = host_pick(x, cur_d[:, 1])
        parents = tree.close(level, frontier, bvar, lambda qs: x[qs])
        if not parents:
            break
        level += 1
        src = np.array([q for q, _, _ in parents])
        kid_t = np.repeat(cur_t[src], 2, axis=0)
        kid_d = np.repeat(cur_d[src], 2, axis=0)
        q2 = np.arange(len(kid_t))
        n, m = kid_d[:, 0].astype(np.int64), kid_d[:, 1].astype(np.int64)
        k = np.repeat(bvar[src], 2)
        v = np.repeat(x[src, bvar[src]], 2)
        up = q2 % 2 == 1
        kid_t[q2, n + 1] = kid_t[q2, n]                      # the f-row moves down
        kid_t[q2, n] = 0.0
        kid_t[q2, n, k] = np.where(up, 1.0, -1.0)
        kid_t[q2, n, m] = np.where(up, -np.ceil(v), np.floor(v))
        kid_d[:, 0] += 1
        out = solve_batch_arrays(kid_t, kid_d, cap, rule="dual", solution=True, tables=False)
        cold += int(out["npivots"].sum())
        gone = np.full(len(kid_t), -np.inf)                  # SMX_INCORRECT counts as empty
        frontier = tree.children(level, parents, out["status"], out["npivots"], out["objective"],
                                 gone, gone)
        cur_t, cur_d, lp, x = kid_t, kid_d, np.repeat(lp[src], 2), out["x"]
    ints = np.ones(ldb, dtype=np.int32)
    return [tree.answer(b, tabs[b, dims[b, 0], :dims[b, 1]], ints[:dims[b, 1]])
            for b in range(B)], cold


def kernel_ms(entry, tabs, dims, cap, depth, reps):
    """Both kernels on the resident outputs of the root solve and k_batch_solution."""
    from simplex_mi355x import _lib, batch
    L = _lib.load()
    B, Rmax, ldb = tabs.shape
    dev = torch.device("cuda")
    stream = torch.cuda.current_stream(dev)
    tier = {"smx_batch_solve": "wave", "smx_batch_solve_wg": "workgroup",
            "smx_batch_solve_gm": "global"}[entry]
    d_dims = torch.from_numpy(dims).to(dev)
    run, d_func, sol, _ = batch._enqueue_base(L, stream, tier, torch.from_numpy(tabs).to(dev),
                                              d_dims, cap)
    node = (run[0], d_dims, sol[3], sol[4], d_func)
    d_ints = torch.ones((B, ldb), dtype=torch.int32, device=dev)
    d_lp = torch.arange(B, dtype=torch.int32, device=dev)
    picks = batch._device_pick(L, stream, node, d_ints, d_lp, TOL)
    ms = {"pick": events_ms(lambda: batch._device_pick(L, stream, node, d_ints, d_lp, TOL), reps)}
    d_src = torch.arange(B, dtype=torch.int32, device=dev)
    Rout = Rmax + depth
    kids = batch._device_branch(L, stream, node, d_src, picks[1], Rout, TOL)
    tc, dc, bc, nc, fc = kids

    def run_branch():
        _lib.check(L.smx_batch_branch(
            node[0].data_ptr(), node[1].data_ptr(), B, Rmax, ldb, node[2].data_ptr(),
            node[3].data_ptr(), node[4].data_ptr(), d_src.data_ptr(), picks[1].data_ptr(), B, Rout,
            TOL, tc.data_ptr(), dc.data_ptr(), bc.data_ptr(), nc.data_ptr(), fc.data_ptr(),
            stream.cuda_stream), "smx_batch_branch")
    ms["branch"] = events_ms(run_branch, reps)
    moved = (node[0].numel() + tc.numel()) * 8               # one read, two writes
    ms["branch_GBps"] = moved / (ms["branch"] * 1e-3) / 1e9
    wo = torch.empty_like(tc)
    nd = (moved // 16 // 2) * 2                              # a copy of nd doubles moves 16 nd bytes
    nd = min(nd, (tc.numel() // 2) * 2)
    ms["copy_probe_GBps"] = max(
        2 * nd * 8 / (events_ms(lambda v=v: _lib.check(L.smx_copy_probe(
            tc.data_ptr(), wo.data_ptr(), nd, v, stream.cuda_stream), "smx_copy_probe"), reps)
            * 1e-3) / 1e9 for v in (0, 1))
    ms["expanded"] = int((picks[0] >= 0).sum())
    return ms


def counts(answers):
    names = [a.status for a in answers]
    return {s: names.count(s) for s in sorted(set(names))}


def main():
    args = sys.argv[1:]
    out = pop_out(args)
    if not args or args[0] not in ("65x65", "ui"):
        sys.exit(__doc__)
    B = int(args[1]) if len(args) > 1 else 2048            # "ui" then holds 200 000 LPs
    from simplex_mi355x import branch
    from simplex_mi355x.batch import GM_TABLE_BUDGET, solve_batch_integer_arrays
    name, entry, cap, tabs, dims = next(w for w in workloads(B) if w[0] == args[0])
    cap = int(args[2]) if len(args) > 2 else (1024 if name == "65x65" else cap)
    depth = int(args[3]) if len(args) > 3 else 4
    max_nodes = branch.default_max_nodes(tabs.shape[1] + depth, tabs.shape[2], GM_TABLE_BUDGET)
    rec = {"what": "batch_branch", "workload": name, "lps": len(tabs),
           "shape": list(tabs.shape[1:]), "max_pivots": cap, "max_depth": depth,
           "max_nodes": max_nodes, "reps": REPS}

    def new():
        return solve_batch_integer_arrays(tabs, dims, None, cap, None, depth)

    def yardstick():
        return yardstick_tree(tabs, dims, cap, depth, max_nodes)

    got, (cold, cold_pivots) = new(), yardstick()            # warm, and compare
    rec["status"] = {"new": {s: got["status"].count(s) for s in sorted(set(got["status"]))},
                     "yardstick": counts(cold)}
    rec["nodes"] = {"new": int(got["nodes"].sum()), "yardstick": sum(a.nodes for a in cold)}
    rec["pivots"] = {"warm": int(got["warm_pivots"].sum()), "cold": cold_pivots}
    rec["depth"] = {"new": int(got["depth"].max(initial=0)),
                    "yardstick": max((a.depth for a in cold), default=0)}
    both = [b for b, a in enumerate(cold) if a.status == "optimal" and got["status"][b] == "optimal"]
    rel = [abs(got["objective"][b] - cold[b].objective) / max(abs(cold[b].objective), 1e-300)
           for b in both]
    rec["objective"] = {"both_optimal": len(both), "max_rel_diff": float(max(rel, default=0.0)),
                        "rel_above_1e-9": int(sum(r > 1e-9 for r in rel))}
    rec["new"], rec["yardstick"] = [], []
    for _ in range(2):
        w_new, w_old = [], []
        for _ in range(REPS):
            w_new.append(timed(new, 1)[0])
            w_old.append(timed(yardstick, 1)[0])
        rec["new"].append(spread(w_new))
        rec["yardstick"].append(spread(w_old))
    rec["kernel_ms"] = kernel_ms(entry, tabs, dims, cap, depth, 10)
    emit(rec, out)


if __name__ == "__main__":
    main()
