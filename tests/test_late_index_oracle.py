"""CPU: the late-index tables of late_index.py on the two oracles, the host engine and the numpy
stand-in of the shard kernels.

(a) The census conditions (late_index.CONDITIONS) for every chain that test_gpu_late_index.py
    runs, on the C oracle alone: every pivot of an embedded table inside its live block, every
    entering column of a steep table in its last columns, indices at or past 1024 where the case
    is there for them, phase-1 owners other than rank 0 and owner changes on the sharded ones.
(b) Every planted table gives the planted (status, r, c) on numpy_oracle.pick and on the C
    oracle.
(c) The host engine (smx_host_*, csrc/smx_host.hpp) gives the oracle's pivots and bits on every
    chain and every planted table.
(d) shard_numpy_backend, whose merge the decision code of the shard kernels shares, does the same
    for worlds 2 and 4 with the live rows owned by the last rank and straddling two ranks, and
    on the planted tables (the tie with r1 and r2 on different ranks, INCORRECT at a row of a
    rank other than 0).
(e) tests/golden/late.json: the reference's own pivots, outcome and final-table hash on small
    embedded and planted tables; both oracles match it.
Nothing here touches a GPU.
"""
from __future__ import annotations

import numpy as np
import pytest

import late_index as li
import special_values as sv
from golden_util import dense_hash, load

CHAINS = sorted(li.CASES)
SHARDS = sorted(li.SHARDED)
# the shapes the GPU file plants tables in: the launch chain's, the block pivots', the resident
# loop's small one, the three batch tiers' and the shards'
PLANT_SHAPES = [(1100, 1300), (1025, 1300), (100, 120), (63, 63), (130, 130), (200, 200),
                (130, 1100), (300, 260)]


# ----------------------------------------------------------------------------------------------
# (a) the census
@pytest.mark.parametrize("name", CHAINS)
def test_census_conditions(name):
    kind, args, k, need = li.CASES[name]
    n, m = li.dims(name)
    cen = li.census(li.table(name), n, m, k)
    li.check_census(kind, args, k, cen, need)
    ref = li.reference(name)
    assert (cen["status"], cen["done"]) == (ref[3], ref[4])
    assert [(r, c) for _, r, c in cen["steps"]] == [tuple(map(int, x)) for x in ref[5]]
    assert sv.same_bits_or_nan(cen["final"], ref[2])


@pytest.mark.parametrize("name", SHARDS)
def test_census_conditions_sharded(name):
    args, world, k, straddles = li.SHARDED[name]
    n, m = args[1:3]
    cen = li.census(li.embedded(*args), n, m, k, world=world)
    li.check_census(li.E, args, k, cen, (), world, straddles)
    r0, tr = args[3], args[5]
    lo, hi = li.owner_of(r0, n, world), li.owner_of(r0 + tr - 1, n, world)
    assert (lo != hi) == straddles and hi == world - 1 and lo >= 0
    assert hi != 0


def test_the_cases_cover_what_they_are_for():
    """Across the chains run with a grid past 1024 rows and columns there is a phase-1 row, a
    phase-1 column and an entering column at or past 1024; the resident, block and batch lists
    each hold an embedded phase-1 case and a phase-2 case; one block case starts at an odd row
    with r0 % 4 == 3; one case ends inside its chain; the live block of the wave-tier cases is
    lanes 40 to 62."""
    needs = {x for name in ("chain_u", "chain_m", "chain_steep") for x in li.CASES[name][3]}
    assert needs >= {"p1row1024", "p1col1024", "enter1024"}
    for prefix in ("chain", "res", "blk", "wave", "wg", "gm"):
        names = [x for x in li.CASES if x.startswith(prefix + "_")]
        assert any(li.CASES[x][0] == li.E and li.CASES[x][1][-1] for x in names), prefix
        assert any(li.CASES[x][0] == li.S or not li.CASES[x][1][-1] for x in names), prefix
    r0 = li.CASES["blk_m_odd"][1][3]
    assert r0 % 2 == 1 and r0 % 4 == 3
    assert "end" in li.CASES["blk_end"][3]
    assert li.CASES["wave_m"][1][3:7] == (40, 40, 23, 23) and li.dims("wave_m") == (63, 63)
    assert any(s for *_, s in li.SHARDED.values()) and not all(s for *_, s in li.SHARDED.values())
    assert {w for _, w, _, _ in li.SHARDED.values()} == {2, 4}


def test_census_counts_by_hand():
    """The census on a planted table whose two pivots are known: phases, late counts, owners."""
    T, flen, want = li.planted("phase1", 130, 130, (64, 129))
    cen = li.census(T, 130, 130, 1, world=2)
    assert cen["steps"] == [(1, 64, 129)] and (cen["late64"], cen["late1024"]) == (1, 0)
    assert cen["p1_rows"] == [64] and cen["p1_cols"] == [129] and cen["enter"] == []
    assert cen["owners"] == [0] and cen["owner_changes"] == 0
    assert [li.owner_of(r, 130, 2) for r in (0, 64, 65, 129)] == [0, 0, 1, 1]
    assert [li.owner_of(r, 300, 4) for r in (74, 75, 224, 225, 299)] == [0, 1, 2, 3, 3]
    T, flen, want = li.planted("fneg", 1100, 1300, (1024, 1299))
    cen = li.census(T, 1100, 1300, 1)
    assert cen["steps"] == [(2, 1024, 1299)] and (cen["late64"], cen["late1024"]) == (1, 1)
    assert cen["enter"] == [1299] and cen["p1_rows"] == []


# ----------------------------------------------------------------------------------------------
# (b) the planted decisions on both oracles
def test_planted_positions():
    """Every kind at every shape; the positions of the issue as the shape allows, r2 = r1 + 1024
    among the pairs of the largest one."""
    assert li.places(1100) == [0, 62, 63, 64, 255, 256, 1023, 1024, 1099]
    assert li.places(63) == [0, 62] and li.places(130) == [0, 62, 63, 64, 129]
    pairs = li.row_pairs(1100)
    assert {(0, 1024), (62, 1086), (62, 63), (63, 64), (255, 256), (1023, 1024)} <= set(pairs)
    for n, m in PLANT_SHAPES:
        cases = li.planted_cases(n, m)
        assert {k for k, _ in cases} == set(li.KINDS), (n, m)
        assert len(set(cases)) == len(cases)
        assert all(a < b for a, b in li.row_pairs(n))


@pytest.mark.parametrize("n,m", PLANT_SHAPES, ids=["{}x{}".format(*s) for s in PLANT_SHAPES])
def test_planted_picks_on_both_oracles(n, m):
    from oracle import c_oracle, numpy_oracle
    for kind, at in li.planted_cases(n, m):
        T, flen, want = li.planted(kind, n, m, at)
        assert numpy_oracle.pick(T, n, m, flen) == want, (kind, at, "numpy")
        assert c_oracle.pick(T, n, m, flen) == want, (kind, at, "C")


def test_planted_tables_are_what_they_say():
    """The construction itself, on the largest shape: one negative "-b" and one positive entry in
    its row; one negative f entry; two equal largest negative ratios; two zero ratios of which
    one is -0.0; the NaN where it belongs."""
    n, m = 1100, 1300
    for kind, at in li.planted_cases(n, m):
        T, flen, want = li.planted(kind, n, m, at)
        b, f = T[:n, m], T[n, :m]
        if kind in ("phase1", "incorrect"):
            assert list(np.flatnonzero(b < 0)) == [at[0]]
            assert list(np.flatnonzero(T[at[0], :m] > 0)) == ([at[1]] if kind == "phase1" else [])
            continue
        assert not (b < 0).any()
        neg = list(np.flatnonzero(f < 0))
        if kind == "optimum":
            assert neg == []
            continue
        if kind == "fshort":
            assert neg == [at[0]] and flen <= at[0] and flen < m
            continue
        c = at[-1]
        assert neg == [c] and flen == m
        col = T[:n, c]
        if kind == "notconv":
            assert not col.any() and np.signbit(col).any() and not np.signbit(col).all()
            continue
        with np.errstate(invalid="ignore", divide="ignore"):
            v = b / col
        if kind == "fneg":
            assert list(np.flatnonzero(v < 0)) == [at[0]]
        elif kind == "tie":
            top = np.flatnonzero(v == v[v < 0].max())
            assert list(top) == [at[0], at[1]] and v[at[0]] == -0.25
        elif kind in ("zero", "zero_neg"):
            z = np.flatnonzero(v == 0)
            assert list(z) == [at[0], at[1]] and not (v < 0).any()
            assert list(np.signbit(v[z])) == ([False, True] if kind == "zero" else [True, False])
        elif kind == "nan_first":
            assert not col[:at[0]].any() and col[at[0]] != 0 and np.isnan(b[at[0]])
            assert list(np.flatnonzero(np.isnan(v))) == [at[0]] and v[at[1]] < 0
        elif kind == "nan_later":
            assert col[0] != 0 and list(np.flatnonzero(np.isnan(v))) == [at[0]] and at[0] != 0
            assert list(np.flatnonzero(v < 0)) == [at[1]]
        else:
            raise AssertionError(kind)


# ----------------------------------------------------------------------------------------------
# (c) the host engine
def _host(T, n, m, flen):
    from simplex_mi355x.host import HostTableau
    return HostTableau(np.array(T), n, m, flen)


@pytest.mark.parametrize("name", CHAINS)
def test_host_engine_chains_vs_oracle(name):
    n, m = li.dims(name)
    ref = li.reference(name)
    dev = _host(ref[0], n, m, m)
    dev.run(li.CASES[name][2])
    li.same_as_oracle(dev, ref, n, m, name)


@pytest.mark.parametrize("n,m", [(1100, 1300), (130, 130)])
def test_host_engine_planted_vs_oracle(n, m):
    """One pick and at most one pivot of every planted table; the pick alone as well
    (smx_host_select)."""
    for kind, at in li.planted_cases(n, m):
        ref = li.planted_reference(kind, n, m, at)
        dev = _host(ref[0], n, m, ref[1])
        st, r, c = dev.pick()[:3]
        want = ref[6]
        assert st == want[0], (kind, at)
        if want[1] >= 0:
            assert r == want[1], (kind, at)
        if want[2] >= 0:
            assert c == want[2], (kind, at)
        dev.run(1)
        li.same_as_oracle(dev, ref, n, m, (kind, at))


# ----------------------------------------------------------------------------------------------
# (d) the numpy stand-in of the shard kernels
def _numpy_shards(T, n, m, flen, world, k):
    """k lockstep pivots of `world` NumpyShardBackend ranks (the all-gather is a copy): the
    ranks' states, logs and the table put together again."""
    import torch
    from shard_numpy_backend import NumpyShardBackend
    from simplex_mi355x.sharded import row_range
    bes = []
    for p in range(world):
        lo, hi = row_range(n, p, world)
        local = np.concatenate([T[lo:hi], T[n:n + 1]], axis=0)
        bes.append(NumpyShardBackend(local, n, m, flen, lo, world))
    for _ in range(k):
        for be in bes:
            be.begin()
        allsend = torch.cat([be.send for be in bes])
        for be in bes:
            be.recv.copy_(allsend)
        for be in bes:
            be.finish()
    tables = [be.local_table() for be in bes]
    full = np.concatenate([t[:-1] for t in tables] + [tables[0][-1:]], axis=0)
    return [be.state() for be in bes], [be.log(0, be.npivots) for be in bes], tables, full


def _shards_same_as_oracle(res, ref, n, m, what):
    states, logs, tables, full = res
    Tref, st, done, log = ref[2:6]
    for s, lg in zip(states, logs):
        assert s["npivots"] == done, (what, s)
        assert np.array_equal(lg, log), (what, lg.tolist(), log.tolist())
        assert bool(s["term"]) == (st != 0), (what, s)
        if st != 0:
            assert s["status"] == st, (what, s)
    for t in tables[1:]:
        assert sv.same_bits_or_nan(t[-1, :m], tables[0][-1, :m]), what
    sv.same_table_as_oracle(full, Tref, n, m, what)


@pytest.mark.parametrize("name", SHARDS)
def test_numpy_shards_chains_vs_oracle(name):
    args, world, k, _ = li.SHARDED[name]
    n, m = args[1:3]
    ref = li.reference(name)
    _shards_same_as_oracle(_numpy_shards(ref[0], n, m, m, world, k), ref, n, m, name)


@pytest.mark.parametrize("world", [2, 4])
def test_numpy_shards_planted_vs_oracle(world):
    """Every planted table at 300 x 260 (ranks of 150 and of 75 rows): the tie at rows 62 and 63
    inside one rank, at 0 and 299, 255 and 256, 256 and 299 on different ones; INCORRECT and the
    lone negative "-b" at rows of every rank."""
    n, m = 300, 260
    cases = li.planted_cases(n, m)
    ties = [at for kind, at in cases if kind == "tie"]
    assert any(li.owner_of(a, n, world) != li.owner_of(b, n, world) for a, b, _ in ties)
    assert any(li.owner_of(at[0], n, world) not in (0,) for kind, at in cases
               if kind == "incorrect")
    for kind, at in cases:
        ref = li.planted_reference(kind, n, m, at)
        res = _numpy_shards(ref[0], n, m, ref[1], world, 1)
        _shards_same_as_oracle(res, ref, n, m, (kind, at, world))


# ----------------------------------------------------------------------------------------------
# (e) the reference's own answers
OUTCOME = {"cap": 0, "optimum": 1, "incorrect system": 2, "simplex method does not converge": 3,
           "IndexError": 4}


def _status_of(outcome):
    return OUTCOME[outcome.get("message") or outcome.get("type") or outcome["kind"]]


GOLDEN = load("late.json")


def test_late_json_is_the_case_list():
    assert [(g["name"], g["kind"], g["cap"]) for g in GOLDEN] == \
        [(name, kind, cap) for name, kind, _, cap in li.LATE_CASES]
    seen = {_status_of(g["outcome"]) for g in GOLDEN}
    assert seen >= {0, 2, 3, 4}
    by = {g["name"]: g for g in GOLDEN}
    # both phases, a chain of some length in each, and the planted picks as the reference made
    # them
    assert len(by["emb_m"]["pivots"]) >= 20 and len(by["emb_u_wide"]["pivots"]) >= 20
    for name, kind, args, cap in li.LATE_CASES:
        if kind != "planted":
            _, _, _, r0, c0, tr, tc, _ = args
            assert all(r0 <= r < r0 + tr and c0 <= c < c0 + tc for r, c in by[name]["pivots"])
            continue
        st, r, c = li.planted(args[0], args[1], args[2], tuple(args[3]))[2]
        assert _status_of(by[name]["outcome"]) == st or st == 0, name
        if st == 0:
            assert by[name]["pivots"][0] == [r, c], name


@pytest.mark.parametrize("g", GOLDEN, ids=[g["name"] for g in GOLDEN])
def test_both_oracles_match_the_reference(g):
    from oracle import c_oracle, numpy_oracle
    name, kind, args, cap = next(x for x in li.LATE_CASES if x[0] == g["name"])
    T, n, m, flen = li.late_table(kind, args)
    want = (_status_of(g["outcome"]), len(g["pivots"]), [tuple(p) for p in g["pivots"]])
    Tc, st, done, log = c_oracle.run(T, n, m, flen, cap)
    assert (st, done, [tuple(map(int, x)) for x in log]) == want
    assert dense_hash(Tc, n, flen) == g["final_hash"]
    nlog = []
    with np.errstate(all="ignore"):
        Tn, st, done = numpy_oracle.run(T.copy(), n, m, flen, cap, log=nlog)
    assert (st, done, nlog) == want
    assert dense_hash(Tn, n, flen) == g["final_hash"]
