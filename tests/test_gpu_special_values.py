"""GPU: NaN, inf and extreme-exponent tables at sizes past one wavefront, through every pivot path
(launch chain, resident loop, block pivots with each planner and sweep form, the three batch
kernels, block pivots on simulated ranks, the forced update) against the C oracle.

The scenarios (special_values.scenario) put a non-finite or extreme value in a different lane,
wave, workgroup, chunk or rank from the value that would otherwise win: the `First` reductions
and their merge with `Cand`, the exponent-window tests on raw high dwords (win_term, bnd_term,
the row flags) and the zero shortcuts (row flag 3, fd_zero / fd_zneg, chunk_zok) see them here.
test_special_values_oracle.py checks on the CPU that every table used below still produces its
event on the oracle.  Pivot log, pivot count and status compare exactly, tables with
special_values.same_bits_or_nan (NaN payload and sign are outside the contract, DESIGN.md
section 1).  Shapes: more than 256 rows span several k_select workgroups and resident row blocks,
n // 3 >= 64 puts the first candidate past the first wave, 1023 columns make 8 sweep chunks of
128, 65 rows or more is past one wave for k_batch_wg, 200 or more past the LDS edge.
"""
from __future__ import annotations

import numpy as np
import pytest

import special_values as sv
from batch_util import solve as _solve, xv_follows_the_labels

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


@pytest.fixture
def knobs():
    """Set smx_tune_resident / smx_tune_block for one test; both policies restored afterwards."""
    from simplex_mi355x import _lib
    prev_b = _lib.tune_block(-1)
    prev_r = _lib.tune_resident(-2)

    def set_(resident, block=None):
        _lib.tune_resident(resident)
        if block is not None:
            _lib.tune_block(block)
    yield set_
    _lib.tune_block(prev_b)
    _lib.tune_resident(prev_r)


@pytest.fixture
def planner():
    """Set smx_tune_block_planner (planner, window slots) for one test."""
    from simplex_mi355x import _lib
    prev = _lib.tune_block_planner(-1, -1)
    yield _lib.tune_block_planner
    _lib.tune_block_planner(prev, 0)


@pytest.fixture
def sweep_form():
    from simplex_mi355x import _lib
    prev = _lib.tune_block_form(-1)
    yield _lib.tune_block_form
    _lib.tune_block_form(prev)


@pytest.fixture
def overlap():
    from simplex_mi355x import _lib
    prev = _lib.tune_resident_overlap(-1)
    yield _lib.tune_resident_overlap
    _lib.tune_resident_overlap(prev)


def _device(name, n, m, seed):
    from simplex_mi355x.device import DeviceTableau
    T = sv.scenario(name, n, m, seed)
    return DeviceTableau(T, n, m, m)


def _run_and_compare(dev, name, n, m, seed, k, graph=False):
    T, Tref, st, done, log = sv.reference(name, n, m, seed, k)
    dev.run(k, graph=graph)
    ctl = dev.sync_state()
    what = (name, n, m, seed, k)
    assert int(ctl["npivots"]) == done, what
    assert np.array_equal(dev.read_log(0, done), log), what
    assert bool(ctl["term"]) == (st != 0), what
    if st != 0:
        assert int(ctl["sel_status"]) == st, what
    sv.same_table_as_oracle(dev.download(), Tref, n, m, what)


# ----------------------------------------------------------------------------------------------
# the launch chain: k_select / k_finalize / update, lookahead
CHAIN_CASES = sv.chain_cases()


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("name,n,m,seed,k", CHAIN_CASES,
                         ids=["{}-{}x{}-s{}".format(*c[:4]) for c in CHAIN_CASES])
def test_launch_chain_vs_oracle(knobs, name, n, m, seed, k, graph):
    knobs(-1, 1)
    dev = _device(name, n, m, seed)
    assert dev.resident_plan() is None and dev.block_plan() is None
    _run_and_compare(dev, name, n, m, seed, k, graph=graph)


# ----------------------------------------------------------------------------------------------
# the resident loop
@pytest.mark.parametrize("name", sv.SCENARIOS)
def test_resident_vs_oracle(knobs, name):
    n, m, k = sv.CHAIN[0]
    knobs(0)
    dev = _device(name, n, m, 5)
    assert dev.resident_plan() is not None
    _run_and_compare(dev, name, n, m, 5, k)
    assert dev.resident_fallbacks == 0


@pytest.mark.parametrize("wg", [1, 7, 256])
@pytest.mark.parametrize("name", ["nan_first", "inf_b"])
def test_resident_workgroup_counts(knobs, name, wg):
    """One workgroup holds the whole table, 7 and 100 split the candidates over workgroups."""
    n, m, k = sv.RESIDENT_SMALL
    knobs(wg)
    dev = _device(name, n, m, 5)
    G, rpw = dev.resident_plan()[1][:2]
    assert G <= wg and G * rpw >= n > (G - 1) * rpw
    _run_and_compare(dev, name, n, m, 5, k)
    assert dev.resident_fallbacks == 0


@pytest.mark.parametrize("ovl", [0, 1], ids=["round3", "overlapped"])
def test_resident_overlap_settings_nan_first(knobs, overlap, ovl):
    n, m, k = sv.CHAIN[0]
    knobs(0)
    overlap(ovl)
    dev = _device("nan_first", n, m, 5)
    assert dev.resident_plan() is not None
    _run_and_compare(dev, "nan_first", n, m, 5, k)
    assert dev.resident_fallbacks == 0


# ----------------------------------------------------------------------------------------------
# block pivots
@pytest.mark.parametrize("P,form", sv.BLOCK)
@pytest.mark.parametrize("plan", [0, 2, 1, "shard1"],
                         ids=["wplan", "wstep", "register", "shard1"])
@pytest.mark.parametrize("name", sv.SCENARIOS)
def test_block_vs_oracle(knobs, planner, sweep_form, name, plan, P, form):
    """Two whole blocks and a ragged one of 3: planner chains and sweep units that leave their
    fast paths and come back to them.  smx_tune_block_planner's settings, and "shard1": the same
    table, pivots per sweep and sweep form on ONE simulated rank of the row-sharded chain."""
    n, m, _ = sv.CHAIN[0]
    knobs(-1, P)
    sweep_form(form)
    if plan == "shard1":
        from test_gpu_block_sharded import _one_rank_vs_oracle
        k = sv.block_k(P)
        T, *ref = sv.reference(name, n, m, 5, k)
        _one_rank_vs_oracle(T, n, m, k, P, ref, (name, n, m, 5, k, "shard1"))
        return
    planner(plan, 0)
    dev = _device(name, n, m, 5)
    assert dev.block_plan()[1] == P
    _run_and_compare(dev, name, n, m, 5, sv.block_k(P))


@pytest.mark.parametrize("nwin", [2, 17])
@pytest.mark.parametrize("plan", [0, 2], ids=["wplan", "wstep"])
@pytest.mark.parametrize("name", ["nan_first", "cols150", "sprinkle"])
def test_block_small_window_vs_oracle(knobs, planner, name, plan, nwin):
    """The window planner with a window of a few columns: entering, phase-1 and pivot columns
    past it take the fallbacks from the block's input table."""
    n, m, _ = sv.CHAIN[0]
    P = 8
    knobs(-1, P)
    planner(plan, nwin)
    dev = _device(name, n, m, 5)
    assert dev.block_plan()[1] == P
    _run_and_compare(dev, name, n, m, 5, sv.block_k(P))


# ----------------------------------------------------------------------------------------------
# the batch kernels
def _batch_refs(name, n, m, k, seeds=sv.SEEDS):
    return [sv.reference(name, n, m, s, k) for s in seeds]


def _batch_check(out, members, what):
    """members: [(n, m, reference)] in launch order; xv after the last pivot against the oracle's
    "-b" entries (NaN-aware: golden_util.same_value)."""
    for q, (n, m, ref) in enumerate(members):
        sv.batch_same_as_oracle(out, q, n, m, ref, (what, q))
    for q, (n, m, ref) in enumerate(members):
        T, Tref, st, done, log = ref
        xv_follows_the_labels({"xv": out["xv"][q:q + 1]}, [(T, m, Tref, st, done, log)], m)


@pytest.mark.parametrize("n,m,k", sv.WAVE)
@pytest.mark.parametrize("name", sv.UNIFORM)
def test_batch_wave_vs_oracle(name, n, m, k):
    """k_batch: seeds 5 and 6 in one launch."""
    refs = _batch_refs(name, n, m, k)
    out = _solve([(r[0], n, m, m) for r in refs], k, kernel="wave")
    _batch_check(out, [(n, m, r) for r in refs], (name, n, m))


@pytest.mark.parametrize("n,m,k", sv.WORKGROUP)
@pytest.mark.parametrize("name", sv.UNIFORM)
def test_batch_workgroup_vs_oracle(name, n, m, k):
    """k_batch_wg: candidates in more than one wave; nan_first with history, the snapshots
    replaying the oracle step by step."""
    from oracle import c_oracle
    from simplex_mi355x.batch import wg_lds_bytes
    assert wg_lds_bytes(n + 1, m + 1) >= 0
    refs = _batch_refs(name, n, m, k)
    history = name == "nan_first"
    out = _solve([(r[0], n, m, m) for r in refs], k, kernel="workgroup", history=history)
    _batch_check(out, [(n, m, r) for r in refs], (name, n, m))
    if not history:
        return
    assert out["snaps"].shape[1:] == (n + 1, m + 1)
    for q, (T, Tref, st, done, log) in enumerate(refs):
        snaps = out["snaps"][out["snap_off"][q]:out["snap_off"][q + 1]]
        assert len(snaps) == done == k
        cur = np.array(T)
        for step, (r, c) in enumerate(log):
            cur = c_oracle.pivot(cur, int(r), int(c))
            assert sv.same_bits_or_nan(snaps[step], cur), \
                (q, step, sv.first_difference(snaps[step], cur))


def test_batch_workgroup_mixed_dims_in_one_launch():
    """65 x 65 and 120 x 8 members of every uniform scenario in one launch, padded to 121 x 66:
    each LP's own n, m inside the launch's padding."""
    members = []
    for name in sv.UNIFORM:
        for n, m, k in sv.WORKGROUP_MIXED:
            members.append((n, m, sv.reference(name, n, m, 5, k)))
    k = sv.WORKGROUP_MIXED[0][2]
    out = _solve([(ref[0], n, m, m) for n, m, ref in members], k, Rmax=121, ldb=66,
                 kernel="workgroup")
    assert out["final"].shape[1:] == (121, 66)
    _batch_check(out, members, "mixed")


@pytest.mark.parametrize("n,m,k", sv.GLOBAL)
@pytest.mark.parametrize("name", sv.UNIFORM)
def test_batch_global_vs_oracle(name, n, m, k):
    """k_batch_gm: past the LDS edge."""
    from simplex_mi355x.batch import wg_lds_bytes
    assert wg_lds_bytes(n + 1, m + 1) == -1
    refs = _batch_refs(name, n, m, k)
    out = _solve([(r[0], n, m, m) for r in refs], k, kernel="global")
    _batch_check(out, [(n, m, r) for r in refs], (name, n, m))


# ----------------------------------------------------------------------------------------------
# block pivots on row shards, simulated ranks
@pytest.mark.parametrize("light", [False, True])
@pytest.mark.parametrize("name", ["nan_first", "inf_b", "rows150"])
def test_block_shards_vs_oracle(name, light):
    """3 ranks of 100 rows: the NaN-first row (row 100 on) and the first candidates belong to the
    second rank, the zero rows to the first."""
    from test_gpu_block_sharded import _backends, _lockstep, _result
    n, m, k = sv.SHARDED
    P, world = 3, 3
    T, Tref, st, done, log = sv.reference(name, n, m, 5, k)
    bes = _backends(np.array(T), n, m, world, P)
    _lockstep(bes, k, P, light)
    states, logs, tables, full = _result(bes)
    for s, lg in zip(states, logs):
        assert s["npivots"] == done
        assert np.array_equal(lg, log)
        assert bool(s["term"]) == (st != 0)
    for t in tables[1:]:   # every f-row replica identical
        assert sv.same_bits_or_nan(t[-1, :m], tables[0][-1, :m])
    sv.same_table_as_oracle(full, Tref, n, m, (name, light))


# ----------------------------------------------------------------------------------------------
# the forced update alone
@pytest.mark.parametrize("n,m", [(63, 64), (200, 129), (1025, 777)])
def test_forced_update_vs_oracle(n, m):
    from oracle import c_oracle
    from simplex_mi355x.device import DeviceTableau
    T, pivots = sv.forced_update_input(n, m)
    dev = DeviceTableau(T, n, m, m + 1)
    for (r, c, plant) in pivots:
        if sv.forced_plant(T, r, c, plant):
            dev.upload(T)
        ref = c_oracle.pivot(T, r, c)
        dev.forced(r, c)
        got = dev.download()
        assert sv.same_bits_or_nan(got, ref), ((r, c), sv.first_difference(got, ref))
        T = ref
        dev.upload(T)
