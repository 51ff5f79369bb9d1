"""Batched mid-sized LP throughput: B uniform LPs of 100 x 100 and of 65 x 65, one workgroup each
(k_batch_wg), max_pivots = 256.  Per shape one JSON line: kernel ms by HIP events (10 repeats after
a warm-up launch), pivots/s and LPs/s on the device, and end to end through solve_batch_arrays and
through solve_batch(history=False).

    python tools/bench_batch_wg.py [B]            the lines above
    python tools/bench_batch_wg.py --serial K     the yardstick: the same solve_batch(history=False)
                                                  call on K LPs per shape, timed per LP -- on a
                                                  commit without the workgroup kernel that call
                                                  runs them one by one through SimplexMethod
Run one process at a time on one box; `--out FILE` appends the lines to FILE as well."""
import sys
import time

from batch_bench_util import CAP, emit, kernel_ms, pop_out, problems, tables
import numpy as np
import torch

SHAPES = ((100, 100), (65, 65))


def serial(K, out):
    from simplex_mi355x import batch
    for n, m in SHAPES:
        tabs, _ = tables(K, n, m)
        probs = problems(tabs, n, m)
        batch.solve_batch(probs[:2], max_pivots=CAP, history=False)          # warm
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res, st = batch.solve_batch(probs, max_pivots=CAP, history=False)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        emit({"what": "batch_wg_yardstick", "shape": [n, m], "lps": K, "max_pivots": CAP,
              "routes": sorted({batch.route(c, f) if hasattr(batch, "route") else "single"
                                for c, f in probs[:4]}),
              "wall_s": wall, "ms_per_lp": 1e3 * wall / K, "lps_per_s": K / wall,
              "statuses": {s: st.count(s) for s in sorted(set(st))}}, out)


def main():
    args = sys.argv[1:]
    out = pop_out(args)
    if args and args[0] == "--serial":
        return serial(int(args[1]) if len(args) > 1 else 64, out)
    from simplex_mi355x.batch import solve_batch, solve_batch_arrays, wg_lds_bytes
    B = int(args[0]) if args else 2048
    for n, m in SHAPES:
        tabs, dims = tables(B, n, m)
        solve_batch_arrays(tabs[:64], dims[:64], CAP)                         # warm
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = solve_batch_arrays(tabs, dims, CAP)                             # H2D + kernel + D2H
        torch.cuda.synchronize()
        wall_arrays = time.perf_counter() - t0
        probs = problems(tabs, n, m)
        solve_batch(probs[:64], max_pivots=CAP, history=False)                # warm
        t0 = time.perf_counter()
        solve_batch(probs, max_pivots=CAP, history=False)                     # Info-object API
        wall_infos = time.perf_counter() - t0
        kms, npiv = kernel_ms("smx_batch_solve_wg", tabs, dims, n, m, 10)    # device only
        pivots = int(npiv.sum())
        assert np.array_equal(npiv, res["npivots"])
        codes = {0: "cap", 1: "optimum", 2: "incorrect system", 3: "does not converge"}
        emit({"what": "batch_wg", "shape": [n, m], "lps": B, "max_pivots": CAP,
              "lds_bytes": wg_lds_bytes(n + 1, m + 1), "pivots": pivots, "kernel_ms": kms,
              "lps_per_s_device": B / (kms * 1e-3),
              "pivots_per_s_device": pivots / (kms * 1e-3),
              "arrays_end_to_end_s": wall_arrays, "lps_per_s_arrays_end_to_end": B / wall_arrays,
              "solve_batch_s": wall_infos, "ms_per_lp_solve_batch": 1e3 * wall_infos / B,
              "lps_per_s_solve_batch": B / wall_infos,
              "statuses": {codes.get(int(k), str(k)): int((res["status"] == k).sum())
                           for k in np.unique(res["status"])}}, out)


if __name__ == "__main__":
    main()
