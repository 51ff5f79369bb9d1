"""GPU: the pivot-log and x-history rings of every chain form against the C oracle's simulation of
them (tests/ring_util.py), as whole arrays of bit patterns.  The rings start as sentinels between
poisoned guard bands, so one comparison sees a wrong slot, a wrong value, a stray write, a missed
write (the "non-basic: 0.0" stores included, which zero-initialised rings hide) and a slot written
too early.  Ring sizes 1, 5, 8 and 64 under 40 pivots asked as 1 + 9 + 30: every ``k % log_cap``
of the kernels wraps, inside one launch as well, and the host readers (``DeviceTableau._ring``,
``MultiTableau.read_xhist``) read across the wrap.

The inputs and what the labels x1 / x2 do in them are pinned by tests/test_ring_oracle.py.
Workgroups: ``smx_nparts_for`` gives 1 for the 37 x 45, 96 x 70 and 150 x 130 LPs and 2 for the
300 x 260 ones (asserted below); the resident loop's grid is taken from ``_lib.resident_plan`` per
test.  ``_lib.block_plan`` exposes the pivots per sweep only, so the block tests run the 300 x 260
LPs next to the small ones without a count of their own.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import ring_util
from golden_util import same_value, table_hash
from ring_util import LPS, check, expected, install, lp_case, poison

pytestmark = pytest.mark.gpu

SCHEDULE = (1, 9, 30)       # a lead pivot, a chain from parity 1, a chain from parity 0
CAPS = (1, 5, 8, 64)        # every pivot in slot 0; coprime to every chunk and block; a block; no wrap


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


@pytest.fixture(params=[0, 1], ids=["unfused", "fused"])
def fused(request):
    """smx_tune_fused for one test: select + update per pivot, or one fused kernel."""
    from simplex_mi355x import _lib
    prev = _lib.load().smx_tune_fused(request.param)
    yield request.param
    _lib.load().smx_tune_fused(prev)


@pytest.fixture
def resident_mode():
    """Set smx_tune_resident for one test and restore the policy afterwards."""
    from simplex_mi355x import _lib
    prev = _lib.tune_resident(-2)
    yield _lib.tune_resident
    _lib.tune_resident(prev)


@pytest.fixture(params=[0, 1], ids=["round3", "overlapped"])
def overlap(request):
    """Both update orders of the resident loop (smx_tune_resident_overlap)."""
    from simplex_mi355x import _lib
    prev = _lib.tune_resident_overlap(-1)
    _lib.tune_resident_overlap(request.param)
    yield request.param
    _lib.tune_resident_overlap(prev)


@pytest.fixture(params=[0, 2, 1], ids=["wplan", "wstep", "register"])
def planner(request):
    """The block chain's three planners (smx_tune_block_planner)."""
    from simplex_mi355x import _lib
    prev = _lib.tune_block_planner(request.param, 0)
    yield request.param
    _lib.tune_block_planner(prev, 0)


@pytest.fixture
def block_mode():
    """The resident loop off, so small tables take the block path; both policies restored."""
    from simplex_mi355x import _lib
    prev_b = _lib.tune_block(-1)
    prev_r = _lib.tune_resident(-2)
    _lib.tune_resident(-1)
    yield _lib.tune_block
    _lib.tune_block(prev_b)
    _lib.tune_resident(prev_r)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _fresh(name, cap, **kw):
    """A fresh DeviceTableau of LPS[name] whose rings are poisoned views between guard bands."""
    from simplex_mi355x.device import DeviceTableau
    T, n, m = lp_case(name)
    dev = DeviceTableau(T.copy(), n, m, m, **kw)    # (the shared table is read-only)
    install(dev, cap)
    return dev


def _settled(dev, name, asked, cap):
    """After chains that asked for ``asked`` pivots in all: the control block, both whole rings
    and the host reader's view of what the ring still holds."""
    exp = expected(name, asked, cap)
    ctl = dev.sync_state()
    assert int(ctl["npivots"]) == exp.done
    assert bool(ctl["term"]) == (exp.traj.status != 0)
    if exp.traj.status:
        assert int(ctl["sel_status"]) == exp.traj.status
    check(dev, exp)
    w = min(cap, exp.done)
    assert np.array_equal(dev.read_log(exp.done - w, exp.done), exp.traj.pivots[exp.done - w:])
    assert np.array_equal(_bits(dev.read_xhist(exp.done - w, exp.done)),
                          exp.traj.xbits[exp.done - w:])
    return exp


def _table_is(dev, exp, name):
    _, n, m = lp_case(name)
    got = dev.download()
    assert np.array_equal(_bits(got[:n]), _bits(exp.traj.table[:n]))
    assert np.array_equal(_bits(got[n, :m]), _bits(exp.traj.table[n, :m]))


def test_select_workgroups_of_the_inputs():
    from simplex_mi355x import _lib
    got = {name: _lib.load().smx_nparts_for(n, m) for name, (_, _, n, m) in LPS.items()}
    assert got == {"u0": 1, "u3": 1, "u1": 2, "m2": 1, "m0": 2, "d1": 1, "dm1": 1, "d0": 1,
                   "C": 1, "D": 1}


# -- one pivot per launch ---------------------------------------------------------------------------
def _one_pivot(name, cap, asks):
    for form in ("eager", "graph", "timed"):
        dev = _fresh(name, cap, resident=False, block=0)
        asked = 0
        for k in asks:
            if form == "timed":
                dev.run_timed(k)
            else:
                dev.run(k, graph=form == "graph")
            asked += k
            exp = _settled(dev, name, asked, cap)
        assert bool(dev._graphs) == (form == "graph")
        _table_is(dev, exp, name)
        dev.close()


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("name", ["u0", "u3", "u1", "m2", "m0", "d1", "dm1", "d0"])
def test_one_pivot_chain(fused, name, cap):
    """Eager, graph and run_timed, each from a fresh tableau, checked after every chain."""
    _one_pivot(name, cap, SCHEDULE)


@pytest.mark.parametrize("cap", [5, 64])
@pytest.mark.parametrize("name", ["C", "D"])
def test_one_pivot_chain_ends_inside_itself(fused, name, cap):
    """12 pivots asked: nothing is written for the pivots that did not happen."""
    _one_pivot(name, cap, (12,))


@pytest.mark.parametrize("cap", [1, 5, 8])
def test_cached_graph_replayed_after_the_ring_wrapped(fused, cap):
    """Chains of 9 from parity 1, 0, 1, 0: the third and fourth replay the graphs the first two
    captured, at pivot counts whose slots differ from those of the capture -- the slot comes from
    the device's pivot counter, not from the capture."""
    dev = _fresh("m0", cap, resident=False, block=0)
    dev.run(1, graph=False)
    asked = 1
    for _ in range(4):
        dev.run(9)
        asked += 9
        assert sorted(dev._graphs) == [(0, 9), (1, 9)][-len(dev._graphs):]
        exp = _settled(dev, "m0", asked, cap)
    assert sorted(dev._graphs) == [(0, 9), (1, 9)]
    _table_is(dev, exp, "m0")
    dev.close()


@pytest.mark.parametrize("cap", [5, 64])
@pytest.mark.parametrize("name", ["u0", "m0"])
def test_host_stepped_pivots_between_two_chains(fused, name, cap):
    """10 chained pivots, three of pick + apply_selected (smx_update alone), 27 chained."""
    dev = _fresh(name, cap, resident=False, block=0)
    dev.run(1, graph=False)
    dev.run(9)
    _settled(dev, name, 10, cap)
    for t in range(3):
        st, r, c, _e = dev.pick()
        assert st == 0
        dev.apply_selected()
        exp = _settled(dev, name, 11 + t, cap)
        assert (r, c) == tuple(int(x) for x in exp.traj.pivots[-1])
    dev.run(27)
    _table_is(dev, _settled(dev, name, 40, cap), name)
    dev.close()


# -- the resident loop --------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("name,wg", [("u0", 1), ("u0", 0), ("u3", 3), ("u1", 0), ("m0", 0),
                                     ("d1", 0), ("dm1", 2), ("d0", 0)])
def test_resident_loop(resident_mode, overlap, name, wg, cap):
    """One persistent launch per chain; one workgroup (wg = 1), a few, and the automatic grid
    (_lib.resident_plan: 10 workgroups of 4 rows at 37 x 45, 75 at 300 x 260).

    This test found the rings' one kernel bug: with two or more workgroups and a ring shorter
    than the chain, a slot written by one workgroup and, log_cap pivots later in the same launch,
    by another (the label's row changed owner, or the label left the basis and workgroup 0 wrote
    its 0.0) could end up holding the older value -- plain stores of workgroups behind different
    L2s reach memory in either order (smx_resident.hpp, the x-history stores after the update;
    u0 with 10 workgroups at log_cap 1, 5, 8 and u3 with 3 at 1, 5 failed, log_cap 64 and one
    workgroup passed).  Such rings are now written through and drained before the next hand-off."""
    resident_mode(wg)
    dev = _fresh(name, cap)
    G = dev.resident_plan()[1][0]
    assert (G == 1) if wg == 1 else (G >= 2)
    asked = 0
    for k in SCHEDULE:
        dev.run(k)
        asked += k
        exp = _settled(dev, name, asked, cap)
    assert dev.resident_fallbacks == 0 and dev.resident_plan() is not None
    _table_is(dev, exp, name)
    dev.close()


@pytest.mark.parametrize("cap", [5, 64])
@pytest.mark.parametrize("name", ["C", "D"])
def test_resident_loop_ends_inside_itself(resident_mode, overlap, name, cap):
    resident_mode(0)
    dev = _fresh(name, cap)
    assert dev.resident_plan()[1][0] >= 2
    dev.run(12)
    _table_is(dev, _settled(dev, name, 12, cap), name)
    assert dev.resident_fallbacks == 0
    dev.close()


@pytest.mark.parametrize("name", ["u0", "m0"])
def test_resident_hand_off_tags_wrap(resident_mode, name):
    """The other ring no test wraps: the hand-off tags (_next_epoch, 1..4095).  After one chain
    the host's tag counter is put at the end of its cycle, a state the class reaches by itself at
    its 4 095th launch; three more chains run under tags 4095, 1 (the exchange buffer re-zeroed)
    and 2.  Pivots, rings and table as the oracle's, no fallback to the launch chain."""
    from simplex_mi355x import _lib
    resident_mode(0)
    dev = _fresh(name, 8)
    assert dev.resident_plan()[1][0] >= 2
    dev.run(4)
    _settled(dev, name, 4, 8)
    assert dev._epoch == 1
    dev._epoch = _lib.RESIDENT_EPOCHS - 1
    tags = []
    for j in (1, 2, 3):
        dev.run(4)
        tags.append(dev._epoch)
        exp = _settled(dev, name, 4 + 4 * j, 8)
    assert tags == [_lib.RESIDENT_EPOCHS, 1, 2]
    assert dev.resident_fallbacks == 0 and dev.resident_plan() is not None
    _table_is(dev, exp, name)
    dev.close()


# -- the block chain ------------------------------------------------------------------------------------
def _block(name, cap, P, asks):
    for form in ("eager", "graph", "timed"):
        dev = _fresh(name, cap, resident=False, block=P)
        assert dev.block_plan()[1] == P
        asked = 0
        for k in asks:
            if form == "timed":
                dev.run_block_timed(k, P)
            else:
                dev.run(k, graph=form == "graph")
            asked += k
            exp = _settled(dev, name, asked, cap)
        _table_is(dev, exp, name)
        dev.close()


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("P", [3, 8])
@pytest.mark.parametrize("name", ["u0", "m0", "dm1", "d0"])
def test_block_chain(block_mode, planner, name, P, cap):
    """Blocks of 3 and 8: 30 = 8 + 8 + 8 + 6 ends on a ragged block, log_cap = 5 < 8 wraps inside
    one planner launch, log_cap = 8 is one block.  The persistent planner (wplan) had the resident
    loop's bug (smx_wplan.hpp: the row pass's x-history stores and workgroup 0's zeros): u0 failed
    at (P, log_cap) = (3, 1), (8, 1) and (8, 5), the rings shorter than a block; the planners
    with one launch per pivot never did."""
    _block(name, cap, P, SCHEDULE)


@pytest.mark.parametrize("cap", [5, 64])
@pytest.mark.parametrize("name", ["C", "D"])
def test_block_chain_ends_inside_a_block(block_mode, planner, name, cap):
    _block(name, cap, 8, (12,))


# -- three simulated ranks, block protocol ---------------------------------------------------------------
def _bshards(name, world, P, cap):
    from simplex_mi355x.sharded import BlockShardBackend, row_range
    T, n, m = lp_case(name)
    bes = []
    for p in range(world):
        lo, hi = row_range(n, p, world)
        local = np.concatenate([T[lo:hi], T[n:n + 1]], axis=0)
        bes.append(BlockShardBackend(local, n, m, m, lo, world, log_cap=cap, pivots=P))
        poison(bes[-1].dev)       # the rings of construction, in place: no guard bands
    return bes


def _ranks_settled(devs, name, asked, cap, xhist=True):
    exp = expected(name, asked, cap, lead=0, world=len(devs))
    for p, d in enumerate(devs):
        ctl = d.sync_state()
        assert int(ctl["npivots"]) == exp.done, p
        assert bool(ctl["term"]) == (exp.traj.status != 0), p
        check(d, exp, rank=p, xhist=xhist)     # every rank logs the merged decision
    return exp


@pytest.mark.parametrize("light", [False, True], ids=["full", "light"])
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("P", [3, 8])
@pytest.mark.parametrize("name", ["u0", "u3", "dm1"])
def test_block_shards(name, P, cap, light):
    """BlockShardBackend in lockstep, both exchanges.  Every rank's x-history against its own
    simulation: the value of a basic label only from the rank that owns its row, the slot left as
    it stood on the others (a sentinel, or what that rank wrote there a lap earlier), +0.0 from
    every rank for a non-basic label; every rank's log holds every pivot."""
    from test_gpu_block_sharded import _lockstep
    bes = _bshards(name, 3, P, cap)
    asked = 0
    for k in SCHEDULE:
        _lockstep(bes, k, P, light)
        asked += k
        _ranks_settled([be.dev for be in bes], name, asked, cap)
    for be in bes:
        be.close()


@pytest.mark.parametrize("cap", [5, 64])
@pytest.mark.parametrize("name", ["C", "D"])
def test_block_shards_end_inside_a_block(name, cap):
    from test_gpu_block_sharded import _lockstep
    bes = _bshards(name, 3, 8, cap)
    _lockstep(bes, 12, 8)
    _ranks_settled([be.dev for be in bes], name, 12, cap)


# -- MultiTableau -----------------------------------------------------------------------------------------
def _multi(name, world, cap, **kw):
    from simplex_mi355x.multi import MultiTableau
    T, n, m = lp_case(name)
    mt = MultiTableau(T, n, m, m, [0] * world, log_cap=cap, **kw)
    for be in mt.ranks:
        poison(be.dev)            # the rank table took the ring pointers at construction
    return mt


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph_chain"])
@pytest.mark.parametrize("cap", [5, 64])
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", ["u0", "u3"])
def test_multi_rings(name, world, cap, graph):
    """smx_mshard_run (8 pivots per sweep) on ranks sharing device 0: per-rank rings."""
    mt = _multi(name, world, cap, graph_chain=graph)
    assert mt.exchange == "copy" and mt.graph_chain == graph
    asked = 0
    for k in SCHEDULE:
        mt.run(k)
        asked += k
        mt.sync_state()
        _ranks_settled([be.dev for be in mt.ranks], name, asked, cap)
    assert bool(mt._graphs) == graph
    mt.close()


@pytest.mark.parametrize("cap", [5, 64])
def test_multi_rccl_world1_rings(cap):
    """exchange="rccl" at world size 1 (the branch distinct devices take)."""
    mt = _multi("u0", 1, cap, exchange="rccl")
    assert mt.exchange == "rccl"
    asked = 0
    for k in SCHEDULE:
        mt.run(k)
        asked += k
        mt.sync_state()
        exp = _ranks_settled([mt.ranks[0].dev], "u0", asked, cap)
        assert np.array_equal(exp.ranks[0][1], exp.xhist)      # one rank owns every row
    mt.close()


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph_chain"])
@pytest.mark.parametrize("cap,chunks", [(5, (1, 4, 5, 3, 5, 5, 2, 5, 5, 5)), (64, SCHEDULE)])
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", ["u0", "u3"])
def test_multi_read_xhist_takes_each_value_from_its_owner(name, world, cap, chunks, graph):
    """read_xhist(before, done) after every chunk equals the single-device expectation: the
    owner look-up picks ranks other than 0 here (test_ring_oracle.py), across the wrap too."""
    mt = _multi(name, world, cap, graph_chain=graph)
    tr = expected(name, 40, cap, lead=0).traj
    for k in chunks:
        before = mt.step
        mt.run(k)
        mt.sync_state()
        assert mt.step == before + k
        assert np.array_equal(mt.read_log(before, mt.step), tr.pivots[before:mt.step])
        assert np.array_equal(_bits(mt.read_xhist(before, mt.step)), tr.xbits[before:mt.step])
    assert mt.step == 40
    mt.close()


def test_multi_read_xhist_refuses_pivots_that_left_the_ring():
    """Label positions at `start` are replayed from the device log: a window whose earlier pivots
    were overwritten raises instead of returning values of the wrong owner."""
    mt = _multi("u0", 3, 5)
    mt.run(1)
    mt.sync_state()
    mt.read_xhist(0, 1)
    mt.run(9)
    mt.sync_state()
    with pytest.raises(RuntimeError, match="no longer in the device log ring"):
        mt.read_xhist(6, 10)
    mt.close()


# -- one-pivot shards ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fused", "unfused"])
@pytest.mark.parametrize("cap", [5, 64])
def test_one_pivot_shards_log_ring(cap, mode):
    """HipShardBackend takes no x-history ring: its log against the simulation on every rank, and
    every element of xhist still its sentinel."""
    import torch
    from simplex_mi355x.sharded import HipShardBackend, row_range
    from test_gpu_sharded import MODES
    T, n, m = lp_case("u0")
    bes = []
    for p in range(3):
        lo, hi = row_range(n, p, 3)
        local = np.concatenate([T[lo:hi], T[n:n + 1]], axis=0)
        bes.append(HipShardBackend(local, n, m, m, lo, 3, log_cap=cap, fused=MODES[mode]))
        poison(bes[-1].dev)
    asked = 0
    for k in (10, 30):
        # the steps of test_gpu_sharded._simulate (which then reads the whole log back: more
        # than a ring of 5 holds)
        for _ in range(k):
            for be in bes:
                with be.stream_ctx():
                    be.begin()
            torch.cuda.synchronize()
            allsend = torch.cat([be.send for be in bes])
            for be in bes:
                be.recv.copy_(allsend)
            torch.cuda.synchronize()
            for be in bes:
                with be.stream_ctx():
                    be.finish()
        asked += k
        _ranks_settled([be.dev for be in bes], "u0", asked, cap, xhist=False)


# -- the engine on a small ring ---------------------------------------------------------------------------------
def _small_rings(monkeypatch, cap=5):
    from simplex_mi355x import engine, multi
    monkeypatch.setattr(engine, "DeviceTableau",
                        functools.partial(engine.DeviceTableau, log_cap=cap))
    monkeypatch.setattr(multi, "MultiTableau", functools.partial(multi.MultiTableau, log_cap=cap))


def _solver(name, devices):
    import simplex
    T, n, m = lp_case(name)
    return simplex.SimplexMethod(T[:n].tolist(), T[n, :m].tolist(), devices=devices)


def _oracle_table(name, step):
    from oracle import c_oracle
    T, n, m = lp_case(name)
    Tref, _, done, _ = c_oracle.run(T, n, m, m, step)
    assert done == step
    return table_hash(Tref[:n].tolist() + [Tref[n, :m].tolist()])


ENGINE_CASES = [("u0", None), ("m0", None), ("u0", [0, 0, 0])]


@pytest.mark.parametrize("chunk", [4, 7])
@pytest.mark.parametrize("name,devices", ENGINE_CASES, ids=["u0", "m0", "u0x3"])
def test_engine_lazy_history_on_a_ring_of_5(monkeypatch, name, devices, chunk):
    """get_solution(lazy=True) with log_cap = 5 gives the steps of a default-ring run and the
    oracle's x1 / x2 bit for bit; chunks are cut to the ring (chunk = 7 runs 5 + 2), so History's
    checkpoints fall inside chunks: tables at steps 0, 13 and 40 against the oracle."""
    ref = _solver(name, devices).get_solution(lazy=True, chunk=chunk, max_pivots=40)
    _small_rings(monkeypatch)
    sm = _solver(name, devices)
    assert sm._dev.log_cap == 5
    got = sm.get_solution(lazy=True, chunk=chunk, max_pivots=40)
    tr = expected(name, 40, 64).traj
    assert len(got) == len(ref) == 41 and sm.status == "cap"
    for t, (a, b) in enumerate(zip(got, ref)):
        assert (a.i, a.j, a.row, a.column) == (b.i, b.j, b.row, b.column), t
        for key in ("x1", "x2", "optimum"):
            assert same_value(getattr(a, key), getattr(b, key)), (t, key)
        if t:
            assert same_value(float(a.x1), float(tr.x[t - 1, 0])), t
            assert same_value(float(a.x2), float(tr.x[t - 1, 1])), t
        if t < 40:
            assert (a.i, a.j) == tuple(int(x) for x in tr.pivots[t]), t
    for step in (0, 13, 40):
        assert table_hash(got[step].table) == _oracle_table(name, step), step
    assert table_hash(got[40].table) == table_hash(ref[40].table)


@pytest.mark.parametrize("name,devices", ENGINE_CASES, ids=["u0", "m0", "u0x3"])
def test_engine_solve_on_a_ring_of_5(monkeypatch, name, devices):
    """solve(record_history=False, chunk=7): chunks of 5 on the small ring."""
    ref_sm = _solver(name, devices)
    ref = ref_sm.solve(record_history=False, chunk=7, max_pivots=40)
    _small_rings(monkeypatch)
    sm = _solver(name, devices)
    got = sm.solve(record_history=False, chunk=7, max_pivots=40)
    tr = expected(name, 40, 64).traj
    assert sm.pivot_log == ref_sm.pivot_log == [tuple(int(x) for x in p) for p in tr.pivots]
    assert len(got) == len(ref) == 2 and sm.status == ref_sm.status == "cap"
    for a, b in zip(got, ref):
        assert (a.i, a.j, a.row, a.column) == (b.i, b.j, b.row, b.column)
        for key in ("x1", "x2", "optimum"):
            assert same_value(getattr(a, key), getattr(b, key)), key
    assert same_value(float(got[-1].x1), float(tr.x[-1, 0]))
    assert same_value(float(got[-1].x2), float(tr.x[-1, 1]))
    assert table_hash(got[-1].table) == table_hash(ref[-1].table) == _oracle_table(name, 40)


# -- the host reader ------------------------------------------------------------------------------------------------
def test_reading_a_window_that_was_overwritten_is_refused():
    """read_log(0, 5) at step 20 with log_cap = 5: those pivots left the ring three laps ago.  The
    reader raises its "pivot log overrun" error instead of answering with pivots 15..19 (it did
    answer, before DeviceTableau._ring compared `start` with the step counter); the newest
    window it still holds is answered."""
    dev = _fresh("u0", 5, resident=False, block=0)
    dev.run(20, graph=False)
    tr = expected("u0", 20, 5).traj
    for read in (dev.read_log, dev.read_xhist):
        with pytest.raises(RuntimeError, match="pivot log overrun"):
            read(0, 5)
        with pytest.raises(RuntimeError, match="pivot log overrun"):
            read(14, 19)
    assert np.array_equal(dev.read_log(15, 20), tr.pivots[15:20])
    assert np.array_equal(_bits(dev.read_xhist(17, 20)), tr.xbits[17:20])
    dev.close()
