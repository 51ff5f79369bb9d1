"""The row-quad sweep layout (sweep form 8) on the CPU: quad_util's census finds what
QUAD_CONDITIONS asks at 256 CUs (an MI355X) on every case test_gpu_block_quads.py runs, and the
census itself is checked on a geometry written out by hand and on a clean table.  Nothing here
touches a GPU.

Counts at 256 CUs, one sweep workgroup per CU, summed over the blocks form 8 sweeps (13 pivots or
more: one block at 13 pivots per sweep, two at 20 and 24), as (quad, chunk) units with 4 / 3 / 2 /
1 / 0 fast rows, then the quads the vote alone holds back, then tail rows fast / not:
  nan_first, cols150, rows150   every quad 0 fast rows, every tail row slow, at every shape
  700 x 900 (a quad and a tail of 1 or 2 per wave: 536 + 488 tails per block), seeds 5 / 6
    inf_b      P = 13   917, 80, 23, 4, 0; 75; 1449 / 63      904, 90, 28, 2, 0; 64; 1467 / 45
               P = 24   1796, 189, 54, 9, 0; 148; 2890 / 134  1778, 208, 58, 4, 0; 126; 2934 / 90
    sprinkle   P = 13   290, 83, 10, 1, 640; 61; 542 / 970    757, 240, 23, 4, 0; 203; 1389 / 123
               P = 24   400, 97, 15, 0, 1536; 60; 724 / 2300  1394, 469, 50, 6, 129; 362; 2610 / 414
    nan_later  P = 13   0, 62, 359, 417, 186; 0; 1437 / 75    0, 40, 300, 457, 227; 0; 1461 / 51
               P = 24   0, 227, 1190, 445, 186; 0; 2818 / 206 0, 221, 1083, 501, 243; 0; 2890 / 134
  895 x 900 (a quad and a tail of 3 per wave: 1024 tails per block), seed 5, P = 24
    inf_b      1780, 214, 44, 10, 0; 148; 5910 / 234
    sprinkle   579, 168, 17, 4, 1280; 111; 2182 / 3962
    nan_later  0, 0, 656, 360, 1032; 0; 2973 / 3171
  1023^2 (two quads per wave, no tail), P = 20, seeds 5 / 6
    inf_b      3645, 348, 87, 14, 2; 307           3666, 329, 92, 9, 0; 270
    nan_later  920, 95, 353, 664, 2064; 48         1261, 664, 591, 1140, 440; 67
    sprinkle   882, 346, 51, 1, 2816; 335          1293, 427, 67, 5, 2304; 411
  fast_path_edge_table, 4 P + 3 pivots, P = 13 / 20 / 24
    1023^2       2100, 460, 0, 0, 3584   2060, 500, 0, 0, 5632   2050, 510, 0, 0, 5632
    1000 x 1100  2154, 528, 6, 0, 3360   3180, 834, 18, 0, 4032  3168, 846, 18, 0, 4032
                 (tails of 1: rows fast / not 1260 / 1575, 1890 / 1890, 1890 / 1890)
  mixed_pair_table  no free chunk in a long block: 3728 (m = 1023) and 4032 (m = 1100) quads with
                 0 fast rows, 1974 to 1979 rows of flag 0 and 23 to 28 of flag 2 over two blocks.
Every all-fast quad of a sharp case lies in a block of more than 12 pivots, and at 20 and 24 per
sweep of more than 18: the counts above are those of phases 2, 3 and 4 too.
"""
from __future__ import annotations

import numpy as np
import pytest

import quad_util as qu
import special_values as sv

CUS = 256   # an MI355X; the GPU tests evaluate the same conditions at the device's own count

QUAD_IDS = ["{}-{}x{}-s{}-P{}".format(*c) for c in qu.QUADS]


@pytest.mark.parametrize("name,n,m,seed,P", qu.QUADS, ids=QUAD_IDS)
def test_quad_conditions(name, n, m, seed, P):
    """QUAD_CONDITIONS for every QUADS case, and the census's own run is the oracle's."""
    cen = qu.quad_case_census(name, n, m, seed, P, CUS)
    qu.check_quad_census(name, n, m, sv.block_k(P), P, cen)
    _, Tref, st, done, _ = sv.reference(name, n, m, seed, sv.block_k(P))
    assert (cen["status"], cen["done"]) == (st, done)
    assert sv.same_bits_or_nan(cen["final"], Tref)


def test_quads_list():
    """QUADS: the 700 x 900 and 1023^2 cases of special_values.PAIRS and every scenario at
    895 x 900; together they hold every class QUAD_CONDITIONS names."""
    assert len(set(qu.QUADS)) == len(qu.QUADS) == 24 + 6 + 6
    assert {c[0] for c in qu.QUADS if c[1:3] == (895, 900)} == set(sv.SCENARIOS)
    assert {c[4] for c in qu.QUADS} == {13, 20, 24}
    tot = {a: 0 for a in qu.QUAD_COUNTS}
    for c in qu.QUADS:
        cen = qu.quad_case_census(*c, CUS)
        for a in qu.QUAD_COUNTS:
            tot[a] += cen[a]
    for a in ("fast4", "fast3", "fast2", "fast1", "fast0", "vote_only", "tail1", "tail2", "tail3",
              "tail_fast", "tail_slow", "fast4_gt6", "fast4_gt12", "fast4_gt18"):
        assert tot[a] >= 1, (a, tot)


@pytest.mark.parametrize("P", [13, 20, 24])
@pytest.mark.parametrize("n,m", [(1023, 1023), (1000, 1100)])
def test_quad_conditions_edge_table(n, m, P):
    T = sv.fast_path_edge_table(n, m)
    cen = qu.quad_census(T, n, m, sv.edge_chain(P), CUS)
    qu.check_quad_census("edge_table", n, m, 4 * P + 3, P, cen)
    assert np.isfinite(cen["final"]).all()
    assert (len(cen["tails"]) > 0) == (n == 1000)


@pytest.mark.parametrize("n,m,seed,P", [(n, m, s, P) for (n, m), s in
                                        sorted(sv.MIXED_PAIR_SEEDS.items()) for P in (20, 24)] +
                         [(1000, 1023, 11, 13), (1000, 1100, 11, 13)])
def test_quad_conditions_mixed_table(n, m, seed, P):
    T = sv.mixed_pair_table(n, m, seed)
    cen = qu.quad_census(T, n, m, sv.pair_chain(P), CUS)
    qu.check_quad_census("mixed_table", n, m, 2 * P + 3, P, cen)
    assert cen["quad_blocks"] == (1 if P == 13 else 2)


def test_quad_geometry_by_hand():
    """The grid and the four-row grouping on small numbers, and the shapes the GPU tests use."""
    assert qu.quad_geometry(11, 200, 2) == (2, 4)
    assert qu.wave_quads(11, 4) == ([], [[0, 4, 8], [1, 5, 9], [2, 6, 10], [3, 7]])
    assert qu.wave_quads(9, 2) == ([(0, 2, 4, 6), (1, 3, 5, 7)], [[8]])
    assert qu.wave_quads(16, 2) == ([(0, 2, 4, 6), (8, 10, 12, 14), (1, 3, 5, 7), (9, 11, 13, 15)],
                                    [])
    assert qu.quad_geometry(5, 100, 256) == (1, 8)
    assert qu.wave_quads(5, 8) == ([], [[0], [1], [2], [3], [4]])
    assert qu.quad_geometry(701, 901, 256) == (8, 128)
    assert qu.quad_geometry(896, 901, 256) == (8, 128)
    assert qu.quad_geometry(1024, 1024, 256) == (8, 128)
    assert qu.quad_geometry(1001, 1101, 256) == (9, 112)
    assert qu.quad_geometry(1024, 1024, 256, 8) == (8, 1024)   # the default grid: single rows
    for R, qs, lens in [(701, 128, {1: 67, 2: 61}), (896, 128, {3: 128}), (1024, 128, {}),
                        (1001, 112, {1: 105})]:
        quads, tails = qu.wave_quads(R, qs)
        rows = sorted([r for q in quads for r in q] + [r for t in tails for r in t])
        assert rows == list(range(R))
        assert all(q[k + 1] - q[k] == qs for q in quads for k in range(3))
        assert all(t[k + 1] - t[k] == qs for t in tails for k in range(len(t) - 1))
        assert {j: sum(len(t) == j for t in tails) for j in (1, 2, 3)
                if any(len(t) == j for t in tails)} == lens
        # a tail follows its wave's last quad
        last = {q[0] % qs: q[3] for q in quads}
        assert all(t[0] == last[t[0] % qs] + qs for t in tails if t[0] % qs in last)


def test_quad_census_on_a_clean_table():
    """A uniform table (every value bounded, every chunk free): the rows that are not fast are
    exactly the pivot rows of each block, so a quad has 4 - (pivot rows it holds) fast rows in
    every chunk alike, nothing is held back by the vote, and a block below 13 pivots is not
    counted.  With 2 CUs the grouping is the one written out by hand."""
    from oracle import c_oracle
    from simplex_mi355x import lp
    n, m, blocks = 42, 300, [13, 12, 4]
    T = lp.dense_tableau("uniform", 3, n, m)
    cen = qu.quad_census(T, n, m, blocks, cus=2)
    assert cen["geometry"] == (3, 4) and cen["status"] == 0 and cen["done"] == 29
    assert cen["quads"] == [tuple(b + 4 * (4 * t + k) for k in range(4)) for b in range(4)
                            for t in range(2)]
    assert cen["tails"] == [[32, 36, 40], [33, 37, 41], [34, 38, 42], [35, 39]]
    Tref, st, done, log = c_oracle.run(T, n, m, m, 29)
    assert np.array_equal(cen["final"].view(np.int64), Tref.view(np.int64))
    assert cen["quad_blocks"] == 1
    for b, blk in enumerate(cen["blocks"]):
        prows = set(blk["pivot_rows"])
        assert blk["free_chunks"] == 3 and blk["vote_only"] == 0
        held = [len(prows & set(q)) for q in cen["quads"]]
        for j in range(5):
            assert blk[f"fast{4 - j}"] == 3 * held.count(j), (b, j)
        assert (blk["tail1"], blk["tail2"], blk["tail3"]) == (0, 3, 9)
        tail_rows = [r for t in cen["tails"] for r in t]
        assert blk["tail_slow"] == 3 * len(prows & set(tail_rows))
        assert blk["tail_fast"] == 3 * len(tail_rows) - blk["tail_slow"]
    first = cen["blocks"][0]
    for a in ("fast4", "fast3", "fast0", "tail_fast", "tail_slow", "flag1", "flag2"):
        assert cen[a] == first[a], a
    assert cen["fast4_gt12"] == first["fast4"] and cen["fast4_gt18"] == 0


def test_quad_census_vote_counts_one_planted_inf():
    """One block of 13 pivots with an inf planted in a row that is no pivot row and no candidate:
    its quad loses one fast row in that chunk, and the vote alone holds the quad back."""
    from simplex_mi355x import lp
    n, m, P = 42, 300, 13
    T = lp.dense_tableau("uniform", 3, n, m)
    base = qu.quad_census(T, n, m, [P], cus=2)
    prows = set(base["blocks"][0]["pivot_rows"])
    quad = next(q for q in base["quads"] if not prows & set(q))
    i, j = quad[2], 140   # chunk 1
    T2 = T.copy()
    T2[i, j] = np.inf
    cen = qu.quad_census(T2, n, m, [P], cus=2)
    blk = cen["blocks"][0]
    # the plant is no ratio candidate and in no pivot column: the same pivots, the row still flag 1
    assert blk["pivot_rows"] == base["blocks"][0]["pivot_rows"]
    assert blk["flags"][i] == 1 and blk["free_chunks"] == 3
    assert cen["vote_only"] == 1
    assert cen["fast3"] == base["fast3"] + 1 and cen["fast4"] == base["fast4"] - 1
