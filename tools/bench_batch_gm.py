"""Batched LPs past one CU's LDS: B uniform LPs with tables of 142 x 142, 256 x 256, 512 x 512 and
724 x 724 (shapes the library's envelope leaves out are skipped), one workgroup each with the table in global memory (k_batch_gm), max_pivots = 256.  Per shape and
batch size one JSON line: kernel ms by HIP events (back-to-back launches after a warm-up launch),
us per pivot step, and the wall time of solve_batch(history=False) on the kernel path
(GM_MIN_BATCH set to 1), per LP: the median and the least of REPS timed calls after a warm-up call.

    python tools/bench_batch_gm.py                the lines above, B in 1, 4, 16, 256, 1024
    python tools/bench_batch_gm.py --ab           workgroup size (256 / 512 / 1024) x LDS mirrors
                                                  (on / off) x loads ahead (8 / 4 / 1) at 141 x 141 and
                                                  512 x 512, B = 256 and B = 1, kernel only
    python tools/bench_batch_gm.py --serial K     the yardstick: K LPs per shape one by one through
                                                  SimplexMethod (solve_batch(history=False,
                                                  kernel="workgroup"), which leaves a table past
                                                  the LDS edge to that path on this commit and on
                                                  its parent alike), timed per LP, REPS times
Batch sizes are bounded by the launch's table budget (batch.GM_TABLE_BUDGET); the solve_batch
timing, which holds every table as Python lists, stops at 2^24 table elements per call.  The LPs
of a batch are seeds 0..15 repeated.  Run one process at a time on one box; `--out FILE` appends
the lines to FILE as well."""
import sys

import batch_bench_util as util
from batch_bench_util import CAP, emit, problems

SHAPES = ((141, 141), (255, 255), (511, 511), (723, 723))   # tables of 142^2, 256^2, 512^2, 724^2
BATCHES = (1, 4, 16, 256, 1024)
DISTINCT = 16
LIST_ELEMS = 1 << 24
REPS = 5


def timed(call, reps=REPS):
    return util.timed(call, reps)


def tables(B, n, m):
    return util.tables(B, n, m, DISTINCT)


def kernel_ms(tabs, dims, n, m, reps):
    """(ms per launch, pivots of one launch, most pivots of one LP)."""
    kms, npiv = util.kernel_ms("smx_batch_solve_gm", tabs, dims, n, m, reps)
    return kms, int(npiv.sum()), int(npiv.max())


def serial(K, out):
    from simplex_mi355x import batch
    for n, m in SHAPES:
        if not batch.gm_fits(n + 1, m + 1):
            continue
        tabs, _ = tables(K, n, m)
        probs = problems(tabs, n, m)
        batch.solve_batch(probs[:2], max_pivots=CAP, history=False, kernel="workgroup")   # warm
        wall, least, (res, st) = timed(lambda: batch.solve_batch(
            probs, max_pivots=CAP, history=False, kernel="workgroup"))
        emit({"what": "batch_gm_yardstick", "shape": [n, m], "lps": K, "max_pivots": CAP,
              "path": "SimplexMethod one by one", "reps": REPS, "wall_s": wall,
              "ms_per_lp": 1e3 * wall / K, "ms_per_lp_least": 1e3 * least / K,
              "statuses": {s: st.count(s) for s in sorted(set(st))}}, out)


def ab(out):
    from simplex_mi355x import _lib
    L = _lib.load()
    prev = L.smx_tune_batch_gm(-1, -1, -1)
    try:
        for n, m in (SHAPES[0], SHAPES[2]):
            for B in (256, 1):
                tabs, dims = tables(B, n, m)
                for unroll in (8, 4, 1):
                    for mirrors in (1, 0):
                        for threads in (256, 512, 1024):
                            L.smx_tune_batch_gm(threads, mirrors, unroll)
                            kms, pivots, deepest = kernel_ms(tabs, dims, n, m, 5)
                            emit({"what": "batch_gm_ab", "threads": threads, "mirrors": mirrors,
                                  "unroll": unroll, "shape": [n, m], "lps": B, "max_pivots": CAP,
                                  "kernel_ms": kms, "pivots": pivots,
                                  "us_per_step": 1e3 * kms / max(deepest, 1)}, out)
    finally:
        L.smx_tune_batch_gm(prev & 0xffff, (prev >> 16) & 0xf, prev >> 20)


def main():
    args = sys.argv[1:]
    out = util.pop_out(args)
    if args and args[0] == "--serial":
        return serial(int(args[1]) if len(args) > 1 else 8, out)
    if args and args[0] == "--ab":
        return ab(out)
    from simplex_mi355x import _lib, batch
    L = _lib.load()
    batch.GM_MIN_BATCH = 1                                   # time the kernel path at every B
    cfg = L.smx_tune_batch_gm(-1, -1, -1)
    cfg = {"threads": cfg & 0xffff, "mirrors": (cfg >> 16) & 0xf, "unroll": cfg >> 20}
    for n, m in SHAPES:
        if not batch.gm_fits(n + 1, m + 1):
            continue
        elems = (n + 1) * (m + 1)
        for B in BATCHES:
            if B * elems * 8 > batch.GM_TABLE_BUDGET:
                continue
            tabs, dims = tables(B, n, m)
            kms, pivots, deepest = kernel_ms(tabs, dims, n, m, 5 if B <= 256 else 2)
            rec = {"what": "batch_gm", "shape": [n, m], "lps": B, "max_pivots": CAP,
                   **cfg, "pivots": pivots, "kernel_ms": kms, "kernel_ms_per_lp": kms / B,
                   "us_per_step": 1e3 * kms / max(deepest, 1),
                   "pivots_per_s_device": pivots / (kms * 1e-3)}
            if B * elems <= LIST_ELEMS:
                probs = problems(tabs, n, m)
                assert {batch.route(c, f) for c, f in probs[:2]} == {"global"}
                batch.solve_batch(probs[:2], max_pivots=CAP, history=False)      # warm
                wall, least, (res, st) = timed(lambda: batch.solve_batch(
                    probs, max_pivots=CAP, history=False), REPS if B <= 16 else 2)
                rec.update({"solve_batch_s": wall, "ms_per_lp_solve_batch": 1e3 * wall / B,
                            "ms_per_lp_solve_batch_least": 1e3 * least / B,
                            "statuses": {s: st.count(s) for s in sorted(set(st))}})
            emit(rec, out)


if __name__ == "__main__":
    main()
