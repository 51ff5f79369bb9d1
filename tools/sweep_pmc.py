"""Driver for rocprofv3 counter passes on the block sweep (k_blk_sweep<P>) of a seeded N x N LP.

  python tools/sweep_pmc.py [--size 16384] [--pivots 8[,20,...]] [--k 32] [--reps 2] [--form 0] [--bpc 0]

Uploads the LP, runs `reps` timed block chains of k pivots (k = 0: --blocks blocks of that many pivots) from the
same start (HIP events around every sweep) for every pivot count given, prints one JSON line per
rep.  --form: smx_tune_block_form (0 the library's policy, 5 one row per lane, 7 row pairs, 8 row quads).  Small and deterministic so every `--pmc` pass sees
the same dispatches (tools/pmc_sweep.sh).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "simplex-method-solver_amd")]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--pivots", default="8")
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--form", type=int, default=0,
                    help="smx_tune_block_form (0 the library's policy; 4 / 5 / 6 / 7 / 8)")
    ap.add_argument("--blocks", type=int, default=1, help="with --k 0: blocks per chain")
    ap.add_argument("--bpc", type=int, default=0,
                    help="sweep workgroups per CU the grid is sized for (0: the library's 8)")
    a = ap.parse_args()
    import numpy as np
    from simplex_mi355x import _lib, lp
    from simplex_mi355x.device import DeviceTableau
    _lib.tune_resident(-1)
    n = m = a.size - 1
    T = lp.dense_tableau("uniform", 0, n, m)
    _lib.tune_block_form(a.form)
    if a.bpc:
        _lib.check(_lib.load().smx_tune_set(-2, a.bpc), "smx_tune_set")
    pivots = [int(x) for x in a.pivots.split(",")]
    dev = DeviceTableau(T, n, m, m, block=pivots[0])
    for P in pivots:
        k = a.k if a.k > 0 else P * a.blocks
        for rep in range(a.reps):
            dev.upload(T)
            sw, tot = dev.run_block_timed(k, P)
            ctl = dev.sync_state()
            print(json.dumps({"rep": rep, "size": a.size, "pivots": P, "k": k, "form": a.form, "bpc": a.bpc,
                              "npivots": int(ctl["npivots"]),
                              "sweep_us": [float(x) * 1e3 for x in sw],
                              "sweep_us_mean": float(np.mean(sw)) * 1e3,
                              "sweep_gbs": 16.0 * a.size * a.size / (float(np.mean(sw)) * 1e-3) / 1e9,
                              "total_ms": tot}), flush=True)


if __name__ == "__main__":
    main()
