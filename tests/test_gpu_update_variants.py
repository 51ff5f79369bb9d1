"""GPU: every selectable variant of the one-pivot update kernel (k_update, csrc/smx_update.hpp:
U = 1, 2 or 4 units in flight, non-temporal or plain stores and loads, the pipelined batch walk) in
every mode -- the forced update, the unfused and the fused chain, both shard forms -- and the fused
chain's look-ahead sweep past 256 MiB, against the C oracle, bit for bit.

On its own the library picks variant 0 or 1; ``smx_tune_set(variant, blocks_per_cu)`` selects the
others, as tools/tune_update.py does.  The shapes (update_util.SHAPES) are chosen for the grid
they give at an explicit workgroup count per CU: more waves than units, one unit per wave exactly,
a single batch with out-of-range slots, several batches with a ragged last one, and waves that
change column chunk between two real units (the pivot-row slice reloaded inside a batch).  Every
test first asserts, with update_util.geometry at the device's own CU count, that its shape still
gives the launch that property; test_update_census.py pins the figures at 256 CUs on the CPU.

Every case takes a fresh DeviceTableau with the resident loop and block pivots off, and runs its
chain eagerly: a cached graph is bound to the variant it was captured with.
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

import ring_util
import special_values as sv
import update_util as uu

pytestmark = pytest.mark.gpu

VARIANTS = list(range(len(uu.VARIANTS)))
LOG_CAP = 64


def _id(shape):
    return "{}x{}".format(*shape)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


@functools.lru_cache(maxsize=None)
def _cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.fixture
def tune():
    """smx_tune_set(variant, workgroups per CU) for one test (variant -1: automatic); automatic
    and the previous workgroup override afterwards."""
    from simplex_mi355x import _lib
    L = _lib.load()
    prev = ctypes.c_int32()
    _lib.check(L.smx_tune_get(None, ctypes.byref(prev), None, None, None, None), "smx_tune_get")

    def set_(variant, bpc):
        assert bpc in (1, 5)
        _lib.check(L.smx_tune_set(variant if variant >= 0 else -2, bpc), "smx_tune_set")
        got = ctypes.c_int32()
        _lib.check(L.smx_tune_get(ctypes.byref(got), None, None, None, None, None), "smx_tune_get")
        assert got.value == variant
    yield set_
    _lib.check(L.smx_tune_set(-2, prev.value), "smx_tune_set")


@pytest.fixture(params=[0, 1], ids=["unfused", "fused"])
def fused(request):
    """smx_tune_fused for one test: select + update per pivot, or one fused kernel."""
    from simplex_mi355x import _lib
    prev = _lib.load().smx_tune_fused(request.param)
    yield request.param
    _lib.load().smx_tune_fused(prev)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _fresh(T, n, m):
    """A fresh tableau on the launch chain, its rings poisoned between guard bands."""
    from simplex_mi355x.device import DeviceTableau
    dev = DeviceTableau(np.array(T), n, m, m, resident=False, block=0)
    assert dev.resident_plan() is None and dev.block_plan() is None
    ring_util.install(dev, LOG_CAP)
    return dev


def _chain_is_the_oracles(dev, n, m, asked, ref, rings):
    """Pivot count, terminal state, log, whole table and both whole rings after an eager chain
    that asked for ``asked`` pivots; ``ref`` = (final table, status, done, log) of the oracle."""
    Tref, status, done, log = ref
    dev.run(asked, graph=False)
    assert not dev._graphs
    ctl = dev.sync_state()
    assert int(ctl["npivots"]) == done
    assert bool(ctl["term"]) == (status != 0)
    if status:
        assert int(ctl["sel_status"]) == status
    assert np.array_equal(dev.read_log(0, done), log)
    got = dev.download()
    sv.same_table_as_oracle(got, Tref, n, m)
    assert np.array_equal(_bits(got[:n]), _bits(Tref[:n]))
    assert np.array_equal(_bits(got[n, :m]), _bits(Tref[n, :m]))
    assert rings.done == done
    assert np.array_equal(_bits(dev.read_xhist(0, done)), rings.traj.xbits)
    ring_util.check(dev, rings)
    dev.close()


# -- the forced update --------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _forced_steps(n, m):
    """special_values.forced_update_input as (input, r, c, oracle result) per step, made once per
    shape: the four pivot positions ("-b" column included), the 2^-150 element and the inf one."""
    from oracle import c_oracle
    T, pivots = sv.forced_update_input(n, m)
    steps = []
    for r, c, plant in pivots:
        T = np.array(T)
        sv.forced_plant(T, r, c, plant)
        ref = c_oracle.pivot(T, r, c)
        for a in (T, ref):
            a.setflags(write=False)
        steps.append((T, r, c, ref))
        T = ref
    return steps


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", list(uu.SHAPES), ids=_id)
def test_forced_update_every_variant(tune, shape, variant):
    from simplex_mi355x.device import DeviceTableau
    n, m = shape
    bpc = uu.SHAPES[shape][0]
    tune(variant, bpc)
    dev = DeviceTableau(np.array(_forced_steps(n, m)[0][0]), n, m, m + 1, resident=False, block=0)
    uu.check_property(shape, uu.geometry(n, m, _cus(), bpc, 0, dev.nparts))
    for k, (T, r, c, ref) in enumerate(_forced_steps(n, m)):
        dev.upload(np.array(T))
        dev.forced(r, c)
        got = dev.download()
        assert sv.same_bits_or_nan(got, ref), (k, (r, c), sv.first_difference(got, ref))
    dev.close()


# -- the one-pivot chain ------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("kind", uu.KINDS)
@pytest.mark.parametrize("shape", uu.CHAIN_SHAPES, ids=_id)
def test_chain_every_variant(tune, fused, shape, kind, variant):
    """12 eager pivots: phase 2 throughout (uniform) and phase 1 first (mixed)."""
    n, m = shape
    bpc = uu.SHAPES[shape][0]
    tune(variant, bpc)
    T = uu.table(kind, n, m)
    dev = _fresh(T, n, m)
    assert not uu.la_sweeps(n, m)
    g = uu.geometry(n, m, _cus(), bpc, dev.nparts if fused else 0, dev.nparts)
    uu.check_property(shape, g)
    ref = uu.oracle(kind, n, m, uu.CHAIN_PIVOTS)
    assert ref[1:3] == (0, uu.CHAIN_PIVOTS)
    rings = ring_util.expected_rings(T, n, m, m, uu.CHAIN_PIVOTS, LOG_CAP, ring_util.GUARD)
    _chain_is_the_oracles(dev, n, m, uu.CHAIN_PIVOTS, ref, rings)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", uu.SHORT_LPS)
def test_chain_ends_inside_itself_every_variant(tune, fused, name, variant):
    """12 pivots asked of the 9 x 5 LPs that reach the optimum after 7 (C) and end "incorrect"
    after 10 (D): the kernels after the terminal one leave everything as it is."""
    from oracle import c_oracle
    tune(variant, 5)
    T, n, m = ring_util.lp_case(name)
    ref = c_oracle.run(T, n, m, m, uu.CHAIN_PIVOTS)
    assert ref[1:3] == {"C": (1, 7), "D": (2, 10)}[name]
    rings = ring_util.expected(name, uu.CHAIN_PIVOTS, LOG_CAP)
    _chain_is_the_oracles(_fresh(T, n, m), n, m, uu.CHAIN_PIVOTS, ref, rings)


# -- both shard forms ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("mode", ["fused", "unfused"])
@pytest.mark.parametrize("case", uu.SHARD_CASES, ids=lambda c: "{}-{}x{}".format(*c[:3]))
def test_shards_every_variant(tune, case, mode, variant):
    """k_update<kShard> / <kShardFused> on 3 simulated ranks, as test_hip_shards_match_oracle."""
    from simplex_mi355x.sharded import HipShardBackend, row_range
    from test_gpu_sharded import MODES, _simulate
    kind, n, m, ranks, bpc, k, prop = case
    tune(variant, bpc)
    T = uu.table(kind, n, m)
    bes = []
    for p in range(ranks):
        lo, hi = row_range(n, p, ranks)
        local = np.concatenate([T[lo:hi], T[n:n + 1]], axis=0)
        bes.append(HipShardBackend(local, n, m, m, lo, ranks, fused=MODES[mode]))
        d = bes[-1].dev
        uu.check_property((n, m), uu.rank_geometry(d.rows, m, _cus(), bpc, MODES[mode], d.nparts,
                                                   ranks), prop)
    states, logs, tables, full, _ = _simulate(T, n, m, k, ranks, mode, bes=bes)
    Tref, st, done, log = uu.oracle(kind, n, m, k)
    assert (st, done) == (0, k)
    for s, lg in zip(states, logs):
        assert s["npivots"] == done and not s["term"]
        assert np.array_equal(lg, log)
    for t in tables[1:]:   # every f-row replica identical
        assert np.array_equal(_bits(t[-1, :m]), _bits(tables[0][-1, :m]))
    assert np.array_equal(_bits(full[:n]), _bits(Tref[:n]))
    assert np.array_equal(_bits(full[n, :m]), _bits(Tref[n, :m]))
    for be in bes:
        be.dev.close()


# -- the look-ahead sweep -----------------------------------------------------------------------
@pytest.mark.parametrize("kind,variant,n", uu.LA_CASES,
                         ids=["{}-v{}-n{}".format(k, "auto" if v < 0 else v, n)
                              for k, v, n in uu.LA_CASES])
def test_look_ahead_sweep_past_256_mib(tune, kind, variant, n):
    """The fused chain on a table past 256 MiB (n = 4099): the first nparts workgroups write the
    next step's look-ahead records and then sweep with the rest (k_update<kFused> with
    forced_r = 1).  n = 4095 is 256 MiB exactly: the same chain with those workgroups reserved."""
    from simplex_mi355x import _lib
    m = uu.LA_M
    assert _lib.fused_enabled()
    tune(variant, uu.LA_BPC)
    T, traj = uu.la_reference(kind, n)
    dev = _fresh(T, n, m)
    ld, rows = dev.shape[0], dev.shape[1]
    assert ld == 8192 and rows == n
    if n == uu.LA_N:
        assert (rows + 1) * ld * 8 > uu.LA_SWEEP_TABLE
    else:
        assert (rows + 1) * ld * 8 == uu.LA_SWEEP_TABLE
    sweeps = uu.la_sweeps(n, m)
    assert sweeps == (n == uu.LA_N)
    g = uu.geometry(n, m, _cus(), uu.LA_BPC, 0 if sweeps else dev.nparts, dev.nparts)
    # the look-ahead workgroups are some of the sweeping ones, or none of them; many batches
    assert g.blocks > dev.nparts and g.iters[4] >= 2 and dev.nparts > 1
    assert traj.status == 0 and traj.done == uu.LA_PIVOTS
    if kind == "mixed":   # phase 1: the records of the look-ahead workgroups decide the row
        assert (np.array(T[:n, m]) < 0).any()
    ref = (traj.table, traj.status, traj.done, traj.pivots)
    _chain_is_the_oracles(dev, n, m, uu.LA_PIVOTS, ref, uu.rings_of(traj, LOG_CAP))
