"""The three forms of a pivot chain -- enqueued (``run(k, graph=False)``), captured as a hipGraph
(``run(k)``) and enqueued with HIP events (``run_timed`` / ``run_block_timed``) -- are one
enqueue function behind three wrappers: each must leave the same pivots, log, x-history and table
as the C oracle, bit for bit.  Small LPs whose rows are padded past their columns (C = 46 ->
ld = 48), chains that start on either buffer parity, both phases, and chains that end inside
themselves.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# kind, seed, n, m.  By the C oracle: A and B take every pivot asked of them here (up to 28), C
# reaches the optimum after 7 pivots, D ends "incorrect" after 10.
LPS = {"A": ("uniform", 3, 37, 45), "B": ("mixed", 3, 37, 45),
       "C": ("uniform", 0, 9, 5), "D": ("mixed", 0, 9, 5)}


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


@functools.lru_cache(maxsize=None)
def _lp(name):
    from simplex_mi355x import lp
    kind, seed, n, m = LPS[name]
    return lp.dense_tableau(kind, seed, n, m), n, m


@functools.lru_cache(maxsize=None)
def _oracle(name, pivots):
    from oracle import c_oracle
    T, n, m = _lp(name)
    return c_oracle.run(T, n, m, m, pivots)


def _start(name, block, lead):
    """A fresh tableau; after ``lead`` = 1 leading pivot the next chain starts on parity 1."""
    from simplex_mi355x.device import DeviceTableau
    T, n, m = _lp(name)
    dev = DeviceTableau(T, n, m, m, resident=False, block=block)
    if lead:
        dev.run(lead, graph=False)
        dev.sync_state()
    assert dev.step == lead and (dev.step & 1) == lead
    return dev


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _same_as_oracle(name, dev, asked):
    """The device's state against the oracle run of ``asked`` pivots; returns the x-history."""
    T, n, m = _lp(name)
    Tref, status, done, log = _oracle(name, asked)
    ctl = dev.sync_state()
    assert int(ctl["npivots"]) == done
    assert bool(ctl["term"]) == (status != 0)
    if status:
        assert int(ctl["sel_status"]) == status
    assert np.array_equal(dev.read_log(0, done), log)
    got = dev.download()
    assert np.array_equal(_bits(got[:n]), _bits(Tref[:n]))
    assert np.array_equal(_bits(got[n, :m]), _bits(Tref[n, :m]))
    return _bits(dev.read_xhist(0, done))


def _times_ok(times, total, count):
    """``count`` finite times >= 0 inside the total's interval (the events sit on one stream)."""
    assert times.shape == (count,) and np.isfinite(times).all() and (times >= 0).all()
    assert np.isfinite(total) and total > 0 and total >= float(times.sum())


def _three_forms(name, block, lead, k, timed):
    """k pivots enqueued, replayed from a graph and timed, each from a fresh tableau."""
    xh = []
    for form in ("eager", "graph", "timed"):
        dev = _start(name, block, lead)
        if form == "timed":
            times, total = timed(dev, k)
        else:
            dev.run(k, graph=form == "graph")
            assert len(dev._graphs) == (form == "graph")
        xh.append(_same_as_oracle(name, dev, lead + k))
        dev.close()
    assert np.array_equal(xh[0], xh[1]) and np.array_equal(xh[0], xh[2])
    return times, total


@pytest.mark.parametrize("name", ["A", "B"])
def test_one_pivot_chain_from_parity_1(fused, name):
    times, total = _three_forms(name, 0, 1, 9, lambda dev, k: dev.run_timed(k))
    _times_ok(times, total, 9)


@pytest.mark.parametrize("name", ["C", "D"])
def test_one_pivot_chain_ends_inside_itself(fused, name):
    """12 pivots asked from parity 0: the optimum after 7 (C), "incorrect" after 10 (D); the
    timed form still returns one time per pivot asked."""
    assert _oracle(name, 12)[1:3] == {"C": (1, 7), "D": (2, 10)}[name]
    times, total = _three_forms(name, 0, 0, 12, lambda dev, k: dev.run_timed(k))
    _times_ok(times, total, 12)


@pytest.mark.parametrize("name", ["A", "B"])
def test_block_chain_from_parity_1(name):
    """7 pivots in sweeps of 3 (3 + 2 + 2), the planner at its default."""
    times, total = _three_forms(name, 3, 1, 7, lambda dev, k: dev.run_block_timed(k, 3))
    _times_ok(times, total, 3)


def test_graph_replay(fused):
    """A cached graph replayed.  A graph is bound to the parity it was captured on and 9 is odd,
    so the chain after the first (parity 1) captures a second graph (parity 0); the third chain
    is on parity 1 again and replays the first: the cache does not grow, and the table equals
    the oracle's after 1 + 9 + 9 = 19 and after 28 pivots."""
    assert _oracle("A", 28)[1:3] == (0, 28)
    dev = _start("A", 0, 1)
    dev.run(9)
    dev.run(9)
    assert sorted(dev._graphs) == [(0, 9), (1, 9)]
    _same_as_oracle("A", dev, 19)
    dev.run(9)
    assert sorted(dev._graphs) == [(0, 9), (1, 9)]
    _same_as_oracle("A", dev, 28)
    dev.close()
