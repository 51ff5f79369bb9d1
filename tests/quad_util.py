"""The row-quad sweep layout (sweep form 8, blk_row_quads / quadf in csrc/smx_sweep.hpp) on the
CPU: which rows a wave takes four at a time, and a census, from the C oracle's tables alone, of
the path every quad takes.  test_quad_census.py checks QUAD_CONDITIONS at 256 CUs without a GPU;
test_gpu_block_quads.py checks them at the device's own CU count before each comparison, so a
geometry that moved fails by name and no comparison goes blind.

Restated here, in numpy: the grid of the LDS layouts (sweep_grid_lds, blk_geom_wg), the grouping
of a wave's rows into quads and a tail of 1-3 rows (blk_row_quads), the planner's row flags
(blk_rflag), the chunk flags (chunk_flags) and quadf's one vote over a lane's eight inputs.
"""
from __future__ import annotations

import functools

import numpy as np

import special_values as sv

QUAD_PHASE = 6    # kQuadPhase: pivots per phase of a quad's scalar operands
QUAD_MIN_P = 13   # kQuadMinP: a block of fewer pivots is swept by form 5's kernel under form 8


def quad_geometry(R: int, C: int, cus: int, bpc: int = 1):
    """(nchunks, qs): chunks of 128 columns and a wave's row stride.  The grid is per * nchunks
    workgroups of four waves, per = cus * bpc // nchunks held to [1, ceil(R / 4)]; workgroup b
    sweeps chunk b % nchunks and its wave w the rows (b // nchunks) * 4 + w + t * qs, qs = 4 per."""
    nchunks = -(-C // 128)
    per = min(max(cus * bpc // nchunks, 1), -(-R // 4))
    return nchunks, 4 * per


def wave_quads(R: int, qs: int):
    """([(r0, r1, r2, r3)], [tail rows]) over every wave of one chunk: a wave's rows base,
    base + qs, ... four at a time; what is left when fewer than four remain is the tail (1-3
    rows, swept one by one)."""
    quads, tails = [], []
    for base in range(min(qs, R)):
        rows = list(range(base, R, qs))
        nq = len(rows) // 4
        quads += [tuple(rows[4 * t:4 * t + 4]) for t in range(nq)]
        if len(rows) % 4:
            tails.append(rows[4 * nq:])
    return quads, tails


QUAD_COUNTS = ("fast4", "fast3", "fast2", "fast1", "fast0", "vote_only", "tail1", "tail2", "tail3",
               "tail_fast", "tail_slow", "free_chunks", "fast4_gt6", "fast4_gt12", "fast4_gt18",
               "flag0", "flag1", "flag2", "flag3", "quad_blocks")


def quad_census(T: np.ndarray, n: int, m: int, blocks, cus: int, bpc: int = 1) -> dict:
    """The path every row quad of the form-8 sweep takes over the chained blocks `blocks` (pivots
    per block).  Per block, from the oracle's pivots (r_q, c_q) and tables T_{k+q}: the
    multipliers mul[i][q] = T_{k+q}[i][c_q], the pivot rows' values, the elements e_q and the
    block's input T_k.  As the kernels decide:

    row flag    2 for a pivot row of the block, else 1 if every multiplier is bounded
                (|v| in [2^-100, 2^101)), else 3 if every one is bounded or +-0, else 0; every row
                of the table, the f-row too.
    chunk free  every e_q bounded and every pivot-row value in the chunk's columns (< C = m + 1).
    row fast    a (row, chunk) unit: the chunk free, the flag 1, every input of the row in the
                chunk finite with |x| < 2^101.
    quad fast   all four rows exist, four flags 1, the chunk free and ONE vote over the eight
                inputs of a lane: all four units fast.  Any other quad, and a tail, goes row by row.

    Only blocks of at least QUAD_MIN_P pivots are counted: a shorter one (the ragged block of 4 of
    every chain, the block of 12 after one of 13) is swept one row at a time by form 5's kernel.

    Returns QUAD_COUNTS summed over the counted blocks ("quad_blocks" of them): (quad, chunk)
    units by how many of their four rows are fast (fast4 .. fast0); vote_only, the quads of a free
    chunk with four flags 1 that the vote alone holds back; (tail, chunk) units by length (tail1 ..
    tail3) and their rows fast or not; free chunks; all-fast quads in blocks of more than 6, 12
    and 18 pivots (phases 2, 3 and 4); rows by flag.  Also "blocks" (the same per block, with
    pivot rows, flags and the unit mask), "quads", "tails", "geometry", "status", "done" and
    "final"."""
    from oracle import c_oracle
    R, C = n + 1, m + 1
    nchunks, qs = quad_geometry(R, C, cus, bpc)
    quads, tails = wave_quads(R, qs)
    qa = np.array(quads, dtype=np.int64).reshape(-1, 4)
    tl = [np.array(t, dtype=np.int64) for t in tails]
    cur = np.ascontiguousarray(T, dtype=np.float64).copy()
    out = dict({a: 0 for a in QUAD_COUNTS}, blocks=[], quads=quads, tails=tails, status=0, done=0,
               geometry=(nchunks, qs))
    for Pb in blocks:
        Tin = cur
        mul, prow, e, prows = np.empty((R, Pb)), np.empty((Pb, C)), np.empty(Pb), []
        for q in range(Pb):
            st, r, c = c_oracle.pick(cur, n, m, m)
            if st != 0:
                out["status"] = st
                break
            mul[:, q], prow[q], e[q] = cur[:, c], cur[r, :C], cur[r, c]
            prows.append(int(r))
            cur = c_oracle.pivot(cur, r, c, threads=8)
            out["done"] += 1
        if out["status"] != 0:
            break
        bnd = sv._bounded(mul)
        flag = np.where(bnd.all(axis=1), 1, np.where((bnd | (mul == 0)).all(axis=1), 3, 0))
        flag[prows] = 2
        free = np.array([sv._bounded(e).all() and
                         sv._bounded(prow[:, ch * 128:(ch + 1) * 128]).all()
                         for ch in range(nchunks)])
        with np.errstate(invalid="ignore"):
            xok = np.stack([(np.abs(Tin[:, ch * 128:min((ch + 1) * 128, C)]) < sv.HI).all(axis=1)
                            for ch in range(nchunks)], axis=1)
        fast = xok & free[None, :] & (flag == 1)[:, None]
        nfast = fast[qa].sum(axis=1) if len(quads) else np.zeros((0, nchunks), dtype=np.int64)
        flags4 = (flag[qa] == 1).all(axis=1) if len(quads) else np.zeros(0, dtype=bool)
        blk = {f"fast{j}": int((nfast == j).sum()) for j in range(5)}
        blk["vote_only"] = int((free[None, :] & flags4[:, None] & (nfast < 4)).sum())
        for j in (1, 2, 3):
            blk[f"tail{j}"] = nchunks * sum(len(t) == j for t in tl)
        tf = sum(int(fast[t].sum()) for t in tl)
        blk["tail_fast"] = tf
        blk["tail_slow"] = nchunks * sum(len(t) for t in tl) - tf
        blk["free_chunks"] = int(free.sum())
        for lim in (6, 12, 18):
            blk[f"fast4_gt{lim}"] = blk["fast4"] if Pb > lim else 0
        for f in range(4):
            blk[f"flag{f}"] = int((flag == f).sum())
        blk["quad_blocks"] = 1
        if Pb >= QUAD_MIN_P:
            for a in QUAD_COUNTS:
                out[a] += blk[a]
        blk.update(pivot_rows=prows, flags=flag, fast=fast)
        out["blocks"].append(blk)
    out["final"] = cur
    return out


# The scenario cases of the quad layout, (scenario, n, m, seed, pivots per sweep), each run as
# special_values.pair_chain(P) = [P, P - 1, 4] with one sweep workgroup per CU.  At 256 CUs:
#   700 x 900   701 rows, stride 128: 61 waves of a chunk own 6 rows (a quad and a tail of 2), 67
#               own 5 (a quad and a tail of 1); 901 columns: a ragged last chunk of 5.  The cases of
#               special_values.PAIRS, 13 (6 + 6 + 1) and 24 (four phases) pivots per sweep.
#   895 x 900   896 rows: every wave owns 7, a quad and a tail of 3.
#   1023^2      1024 rows: every wave owns 8, exactly two quads, no tail; 20 (6 + 6 + 6 + 2).
QUADS = [c for c in sv.PAIRS if c[1:3] == (700, 900)] + \
        [(name, 895, 900, 5, 24) for name in sv.SCENARIOS] + \
        [c for c in sv.PAIRS if c[1:3] == (1023, 1023)]

# What the quad census must find in the blocks that form 8 sweeps (conditions that keep the GPU
# comparisons from going blind; the counts measured at 256 CUs are in test_quad_census.py's
# docstring).  Every case besides: all pivots done, no terminal outcome.
QUAD_CONDITIONS = {
    "sharp": "inf_b and sprinkle at every shape, nan_later at 1023^2: >= 200 all-fast (quad, chunk) "
             "units, >= 50 with exactly 3 fast rows and >= 10 with exactly 2 (the quad fast path "
             "and its row-by-row fallback side by side); at least one quad that the vote alone "
             "holds back (chunk free, four flags 1: a vote over fewer than eight inputs would take "
             "it); all-fast quads in blocks of more than 6 and 12 pivots, and of more than 18 "
             "from 20 pivots per sweep on (a later phase reading another row's multipliers or "
             "another pivot's (e, y) would change bits)",
    "one_fast": "inf_b and nan_later, every case: at least one quad with exactly 1 fast row",
    "mixed_only": "nan_later at 700 x 900 and 895 x 900 (the first third of the rows has zero "
                  "multipliers, and every quad holds one of them): no all-fast quad, >= 100 quads "
                  "each with exactly 2 and exactly 1 fast rows",
    "fallback": "nan_first, cols150, rows150: no fast row in any quad (every quad goes row by row "
                "through the prefetch rotation)",
    "tails": "700 x 900: tails of 1 and of 2 rows; 895 x 900: tails of 3 rows, every wave; 1023^2: "
             "none.  Sharp and mixed_only cases with tails: tail rows fast and not",
    "edge_table": "fast_path_edge_table: at least one all-fast quad and one quad with 1 to 3 fast "
                  "rows, in blocks of more than 12 pivots and, from 20 per sweep on, of more than "
                  "18; tail rows of both kinds where the shape has tails",
    "mixed_table": "mixed_pair_table: no free chunk in the blocks form 8 sweeps, so every quad goes "
                   "row by row: pivot rows (flag 2) and rows with an unbounded multiplier (flag 0), through "
                   "the window-tracked and exact paths",
}


def check_quad_census(name: str, n: int, m: int, k: int, P: int, cen: dict) -> None:
    """Assert QUAD_CONDITIONS on a quad census of k pivots at P pivots per sweep (name: a
    scenario, "edge_table" or "mixed_table")."""
    what = (name, n, m, k, P, cen["geometry"], {a: cen[a] for a in QUAD_COUNTS})
    assert cen["status"] == 0 and cen["done"] == k, what
    assert cen["quad_blocks"] >= 1 and len(cen["quads"]) > 0, what
    has_tails = len(cen["tails"]) > 0
    mixed = cen["fast1"] + cen["fast2"] + cen["fast3"]
    both_tails = False
    if name == "edge_table":
        assert cen["fast4"] >= 1 and mixed >= 1, what
        assert cen["fast4_gt12"] >= 1 and (P < 20 or cen["fast4_gt18"] >= 1), what
        both_tails = True
    elif name == "mixed_table":
        assert cen["free_chunks"] == 0 and cen["fast4"] == 0 and mixed == 0, what
        assert min(cen["flag0"], cen["flag2"]) >= 1, what
    elif name in sv.SHARP and not (name == "nan_later" and n != 1023):
        assert cen["fast4"] >= 200 and cen["fast3"] >= 50 and cen["fast2"] >= 10, what
        assert cen["vote_only"] >= 1, what
        assert cen["fast4_gt6"] >= 1 and cen["fast4_gt12"] >= 1, what
        assert P < 20 or cen["fast4_gt18"] >= 1, what
        both_tails = True
    elif name == "nan_later":
        assert cen["fast4"] == 0 and cen["fast2"] >= 100 and cen["fast1"] >= 100, what
        both_tails = True
    elif name in sv.SCENARIOS:
        assert cen["fast4"] == 0 and mixed == 0, what
    else:
        raise ValueError(name)
    if name in ("inf_b", "nan_later"):
        assert cen["fast1"] >= 1, what
    if both_tails and has_tails:
        assert cen["tail_fast"] >= 1 and cen["tail_slow"] >= 1, what
    if (n, m) == (700, 900):
        assert cen["tail1"] >= 1 and cen["tail2"] >= 1 and cen["tail3"] == 0, what
    elif (n, m) == (895, 900):
        assert cen["tail3"] >= 1 and cen["tail1"] == cen["tail2"] == 0, what
    elif (n, m) == (1023, 1023):
        assert not has_tails, what


@functools.lru_cache(maxsize=None)
def quad_case_census(name: str, n: int, m: int, seed: int, P: int, cus: int) -> dict:
    """quad_census of a QUADS case over pair_chain(P), computed once per CU count."""
    return quad_census(sv.scenario(name, n, m, seed), n, m, sv.pair_chain(P), cus)
