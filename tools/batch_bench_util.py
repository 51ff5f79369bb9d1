"""What tools/bench_batch_wg.py and tools/bench_batch_gm.py share: seeded batches, wall and HIP-event
timing, and the JSON lines."""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "simplex-method-solver_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

CAP = 256


def timed(call, reps):
    """Wall seconds of `call` (synchronised), `reps` times: (median, least, the last result)."""
    walls = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ret = call()
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    return float(np.median(walls)), min(walls), ret


def tables(B, n, m, distinct=None):
    """B uniform n x m LPs: seeds 0..B-1, or seeds 0..distinct-1 repeated."""
    from simplex_mi355x import lp
    base = np.stack([lp.dense_tableau("uniform", s, n, m) for s in range(min(B, distinct or B))])
    tabs = np.ascontiguousarray(np.resize(base, (B, n + 1, m + 1)))
    dims = np.tile(np.array([n, m, m], dtype=np.int32), (B, 1))
    return tabs, dims


def problems(tabs, n, m):
    return [(t[:n].tolist(), t[n, :m].tolist()) for t in tabs]


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as fh:
            fh.write(line + "\n")


def pop_out(args):
    """Take `--out FILE` out of args; returns FILE or None."""
    if "--out" not in args:
        return None
    k = args.index("--out")
    out = args[k + 1]
    del args[k:k + 2]
    return out


def kernel_ms(entry, tabs, dims, n, m, reps):
    """The library entry point `entry` (smx_batch_solve_wg / _gm) on resident buffers by HIP
    events: one warm-up launch, then `reps` back to back.  Returns (ms per launch, pivots per LP
    of one launch as a numpy array)."""
    from simplex_mi355x import _lib
    B = len(tabs)
    dt, dd = torch.from_numpy(tabs).cuda(), torch.from_numpy(dims).cuda()
    o = torch.empty_like(dt)
    rc = torch.zeros((B, CAP, 2), dtype=torch.int32, device="cuda")
    xv = torch.zeros((B, CAP, 2), dtype=torch.float64, device="cuda")
    s_ = torch.zeros(B, dtype=torch.int32, device="cuda")
    np_ = torch.zeros(B, dtype=torch.int32, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a = (dt.data_ptr(), dd.data_ptr(), B, n + 1, m + 1, CAP, o.data_ptr(), rc.data_ptr(),
         xv.data_ptr(), None, s_.data_ptr(), np_.data_ptr(),
         torch.cuda.current_stream().cuda_stream)
    solve = getattr(_lib.load(), entry)
    _lib.check(solve(*a), entry)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        solve(*a)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, np_.cpu().numpy()
