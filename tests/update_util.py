"""What the tests of the one-pivot update kernel share (k_update, csrc/smx_update.hpp): its launch
geometry restated, the table of its selectable variants, the thresholds that choose its paths and
the case lists.  test_update_census.py checks all of it on the CPU against the sources and the
library's host-only entry points; test_gpu_update_variants.py runs the cases on the device.

The sweep: a unit is one row x one chunk of 128 columns, unit u = row * nchunks + chunk; wave w of
NW takes units w, w + NW, ... in batches of U.  Advancing a unit by NW advances (row, chunk) by
(qs, rs) = divmod(NW, nchunks): with rs == 0 a wave stays in one column chunk and keeps its slice
of the pivot row, otherwise it reloads the slice whenever the chunk changes.  A wave runs
ceil((units - w) / (U * NW)) batches, so the longest loop has ceil(units / (U * NW)) iterations.
"""
from __future__ import annotations

import functools
import math
from typing import NamedTuple

UPD_WAVES = 4                  # kUpdBlock / kWave: waves per workgroup
CHUNK = 128                    # doubles per unit: 64 lanes x 2
CACHE_TABLE = 16 << 20         # kCacheTable: automatic variant 0 up to here, 1 beyond
LA_SWEEP_TABLE = 256 << 20     # kLaSweepTable: beyond it the look-ahead workgroups sweep too
FIRST_DIAG_VARIANT = 10        # kFirstDiagVariant: refused unless SMX_ALLOW_DIAG=1
SMALL_VARIANT, LARGE_VARIANT = 0, 1

# (u, nts, ntl, pipe) of variants 0..9: units in flight, non-temporal stores, non-temporal loads,
# the next batch's loads issued before the current batch's arithmetic
VARIANTS = ((2, 1, 0, 0), (2, 1, 1, 0), (2, 1, 0, 1), (2, 1, 1, 1), (1, 1, 0, 1), (1, 1, 1, 1),
            (4, 1, 0, 0), (4, 1, 0, 1), (2, 0, 0, 0), (1, 1, 0, 0))
UNITS_IN_FLIGHT = (1, 2, 4)


def nt_bits(variant: int) -> int:
    """smx_tune_get's ``nt`` for a variant: nts | ntl << 1 | pipe << 2."""
    _, nts, ntl, pipe = VARIANTS[variant]
    return nts | ntl << 1 | pipe << 2


class Geometry(NamedTuple):
    blocks: int        # sweeping workgroups (the grid is blocks + reserved)
    NW: int            # sweeping waves
    nchunks: int
    units: int
    qs: int
    rs: int
    iters: dict        # {U: iterations of the longest batch loop}
    need: int          # workgroups that cover every unit once: the cap on blocks
    trimmed: bool      # the wave count was cut to a multiple of lcm(nchunks, waves per workgroup)


def geometry(rows: int, m: int, cus: int, bpc: int, reserved: int = 0, nparts: int = 1) -> Geometry:
    """update_grid (csrc/smx_kernels.hip) and the kernel's own NW, qs and rs for a table of
    ``rows`` constraint rows (the f-row is added here) and m + 1 columns on ``cus`` CUs with
    ``bpc`` workgroups per CU, ``reserved`` of them kept for the look-ahead records (the fused
    chain's nparts when they do not sweep, else 0).  ``nparts``: the launch never has fewer
    workgroups than that (launch_update_mode)."""
    R, C = rows + 1, m + 1
    nchunks = -(-C // CHUNK)
    units = nchunks * R
    blocks = max(cus * bpc - reserved, 1)
    lcm = nchunks // math.gcd(nchunks, UPD_WAVES) * UPD_WAVES
    waves = blocks * UPD_WAVES
    trimmed = False
    if waves >= lcm and (waves - waves % lcm) * 4 >= waves * 3:
        trimmed = waves % lcm != 0
        blocks = (waves - waves % lcm) // UPD_WAVES
    need = -(-units // UPD_WAVES)
    blocks = max(min(blocks, need), 1)
    grid = max(blocks + reserved, nparts, 1)
    NW = (grid - reserved) * UPD_WAVES
    iters = {U: -(-units // (U * NW)) for U in UNITS_IN_FLIGHT}
    return Geometry(grid - reserved, NW, nchunks, units, NW // nchunks, NW % nchunks, iters, need,
                    trimmed)


def leading_dim(m: int) -> int:
    """device.leading_dim at its default padding: m + 1 columns rounded up to 16 doubles."""
    return -(-(m + 1) // 16) * 16


def table_bytes(rows: int, m: int) -> int:
    """One buffer of the ping-pong pair, the f-row included: what the thresholds compare."""
    return (rows + 1) * leading_dim(m) * 8


def la_sweeps(rows: int, m: int) -> bool:
    """The fused chain's look-ahead workgroups join the sweep (launch_update_mode)."""
    return table_bytes(rows, m) > LA_SWEEP_TABLE


# ---------------------------------------------------------------------------------------------
# The shapes: (n, m) -> (workgroups per CU, the property the shape is there for).  The figures in
# CENSUS_256 are what the restatement gives on the 256 CUs of an MI355X without reserved
# workgroups (forced update, unfused chain), as (blocks, NW, nchunks, rs, iterations for U = 1,
# 2, 4); RESERVED_256 the same for the fused chain's launches, whose first nparts workgroups
# only write look-ahead records.
SHAPES = {
    (1, 1): (5, "tiny"),
    (5, 2): (5, "tiny"),
    (63, 64): (5, "exact"),
    (200, 300): (5, "need"),
    (1025, 777): (1, "ragged"),
    (40, 16500): (1, "walk"),
    (999, 3000): (5, "production"),
}
CENSUS_256 = {
    (1, 1): (1, 4, 1, 0, (1, 1, 1)),
    (5, 2): (2, 8, 1, 0, (1, 1, 1)),
    (63, 64): (16, 64, 1, 0, (1, 1, 1)),
    (200, 300): (151, 604, 3, 1, (1, 1, 1)),
    (1025, 777): (252, 1008, 7, 0, (8, 4, 2)),
    (40, 16500): (256, 1024, 129, 121, (6, 3, 2)),
    (999, 3000): (1278, 5112, 24, 0, (5, 3, 2)),
}
CHAIN_SHAPES = [(200, 300), (1025, 777), (40, 16500)]
RESERVED_256 = {   # (nparts, blocks, NW, rs, iterations)
    (200, 300): (2, 151, 604, 1, (1, 1, 1)),
    (1025, 777): (5, 245, 980, 0, (8, 4, 2)),
    (40, 16500): (64, 192, 768, 123, (7, 4, 2)),
}
CHAIN_PIVOTS = 12
KINDS = ("uniform", "mixed")
SHORT_LPS = ("C", "D")         # of test_gpu_chain_forms.py: they end inside a chain of 12

# row-sharded: (kind, n, m, ranks, workgroups per CU, pivots, property of every rank's launch).  At
# 256 CUs, per rank: 40 x 16500 on 13 / 13 / 14 rows, 64 look-ahead workgroups: NW 1024, rs 121,
# 2 / 1 / 1 iterations unfused and NW 768, rs 123, 3 / 2 / 1 fused; 1001 x 777 on 333 / 334 / 334
# rows, 4 look-ahead workgroups: NW 1008, rs 0, 3 / 2 / 1 iterations either way.
SHARD_CASES = [("mixed", 40, 16500, 3, 1, 12, "walk_rank"),
               ("uniform", 1001, 777, 3, 1, 12, "ragged_rank")]
SHARD_256 = {   # (fused, rows) -> (nparts, NW, rs, iterations)
    (40, 16500): {(0, 13): (64, 1024, 121, (2, 1, 1)), (0, 14): (64, 1024, 121, (2, 1, 1)),
                  (1, 13): (64, 768, 123, (3, 2, 1)), (1, 14): (64, 768, 123, (3, 2, 1))},
    (1001, 777): {(0, 333): (4, 1008, 0, (3, 2, 1)), (0, 334): (4, 1008, 0, (3, 2, 1)),
                  (1, 333): (4, 1008, 0, (3, 2, 1)), (1, 334): (4, 1008, 0, (3, 2, 1))},
}

# the look-ahead sweep: a table four rows past 256 MiB at ld = 8192, and the largest within it;
# (kind, variant or -1 for automatic, n), the cases on one table next to each other.  At 256 CUs
# and 5 workgroups per CU: n = 4099 sweeps with all 1280 workgroups (NW 5120, 52 / 26 / 13
# iterations), the first 32 of them writing the records first; n = 4095 keeps those 32 out of the
# sweep (NW 4992, 53 / 27 / 14).
LA_N, LA_M, LA_N_BELOW = 4099, 8191, 4095
LA_BPC = 5
LA_PIVOTS = 6
LA_CASES = [("uniform", -1, LA_N), ("uniform", 7, LA_N), ("mixed", -1, LA_N),
            ("uniform", -1, LA_N_BELOW)]


def check_property(shape, g: Geometry, what=None) -> None:
    """Assert what SHAPES says the shape is there for, on a geometry of it."""
    n, m = shape
    prop = what or SHAPES[shape][1]
    msg = (shape, prop, g)
    if prop == "tiny":
        # one chunk, C <= 2 or odd, more waves than units: whole waves have nothing to do
        assert g.nchunks == 1 and (m + 1 <= 2 or (m + 1) % 2 == 1) and g.NW > g.units, msg
    elif prop == "exact":
        # one unit per wave exactly: every batch slot past the first is out of range
        assert g.units == g.NW and set(g.iters.values()) == {1}, msg
    elif prop == "need":
        # capped by the unit count; waves on different chunks; a single batch
        assert g.blocks == g.need and g.rs != 0 and set(g.iters.values()) == {1}, msg
    elif prop == "ragged":
        # a wave keeps its chunk; several batches for every U, the last one of U = 4 ragged
        assert g.rs == 0, msg
        assert g.iters[4] >= 2 and g.units % (4 * g.NW) != 0, msg
    elif prop == "walk":
        # a wave changes chunk from unit to unit and owns two or more real units, so the chunk
        # changes inside a batch of real units for U = 2 and U = 4
        assert g.rs != 0 and g.nchunks > 1, msg
        assert g.units >= 2 * g.NW and g.iters[4] >= 2, msg
    elif prop == "production":
        # odd C at the production workgroup count, two or more batches for U = 4
        assert (m + 1) % 2 == 1 and g.iters[4] >= 2, msg
    elif prop == "walk_rank":
        # one rank's rows: some waves own two real units, in different chunks
        assert g.rs != 0 and g.units > g.NW, msg
    elif prop == "ragged_rank":
        # one rank's rows: a wave keeps its chunk over two or more batches, the last one ragged
        assert g.rs == 0 and g.iters[1] >= 2 and g.units % g.NW != 0, msg
    else:
        raise ValueError(prop)


def rank_rows(n: int, ranks: int):
    """Rows per rank of simplex_mi355x.sharded.row_range."""
    return [(p + 1) * n // ranks - p * n // ranks for p in range(ranks)]


def rank_geometry(rows: int, m: int, cus: int, bpc: int, fused: bool, nparts: int,
                  ranks: int) -> Geometry:
    """One rank's update launch: the fused form reserves the rank's nparts look-ahead workgroups
    (while they do not sweep); the unfused form's partial count is the rank count."""
    if fused:
        return geometry(rows, m, cus, bpc, 0 if la_sweeps(rows, m) else nparts, nparts)
    return geometry(rows, m, cus, bpc, 0, ranks)


# ---------------------------------------------------------------------------------------------
# Inputs and oracle results, computed once and shared read-only.
SEED = 4


@functools.lru_cache(maxsize=None)
def table(kind: str, n: int, m: int):
    from simplex_mi355x import lp
    T = lp.dense_tableau(kind, SEED, n, m)
    T.setflags(write=False)
    return T


@functools.lru_cache(maxsize=None)
def oracle(kind: str, n: int, m: int, pivots: int, threads: int = 8):
    """(final table, status, pivots done, log) of c_oracle.run on table(kind, n, m)."""
    from oracle import c_oracle
    out = c_oracle.run(table(kind, n, m), n, m, m, pivots, threads=threads)
    for a in (out[0], out[3]):
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=1)
def la_reference(kind: str, n: int):
    """(T, ring_util.Trajectory) of LA_PIVOTS pivots of the n x LA_M table: pivots, status and
    final table from c_oracle.run on 16 threads, the labels' rows and the x-history from stepping
    the oracle the way ring_util.trajectory does (its memo would keep every 256 MiB table alive),
    whose final table must be the run's.  One table at a time is kept."""
    import numpy as np
    import ring_util
    from oracle import c_oracle
    from simplex_mi355x import lp
    m = LA_M
    T = lp.dense_tableau(kind, SEED, n, m)
    Tref, status, done, log = c_oracle.run(T, n, m, m, LA_PIVOTS, threads=16)
    cur, where, xbits, rows = T, [-1, -2], [], []
    for t in range(done):
        st, r, c = c_oracle.pick(cur, n, m, m)
        assert st == 0 and (r, c) == tuple(log[t])
        cur = c_oracle.pivot(cur, r, c, threads=16)
        for q in (0, 1):
            if where[q] == -(c + 1):
                where[q] = r
            elif where[q] == r:
                where[q] = -(c + 1)
        rows.append([w if w >= 0 else -1 for w in where])
        xbits.append([int(cur[w:w + 1, m].view(np.int64)[0]) if w >= 0 else 0 for w in where])
    assert np.array_equal(cur.view(np.int64), Tref.view(np.int64))
    traj = ring_util.Trajectory(np.array(log, dtype=np.int32).reshape(-1, 2),
                                np.array(rows, dtype=np.int64).reshape(-1, 2),
                                np.array(xbits, dtype=np.int64).reshape(-1, 2), int(status), Tref)
    for a in (T, Tref, traj.pivots, traj.rows, traj.xbits):
        a.setflags(write=False)
    return T, traj


def rings_of(traj, log_cap: int):
    """ring_util's expectation of both whole rings after traj's pivots, guard bands included."""
    import ring_util
    log, xh = ring_util._simulate(traj, log_cap, ring_util.GUARD)
    return ring_util.Rings(traj, log_cap, ring_util.GUARD, log, xh)
