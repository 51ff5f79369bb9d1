"""The pivot-log and x-history rings (include/smx.h: ``log[k % log_cap] = (r, c)``,
``xhist[k % log_cap] = (x1, x2)``) restated on the C oracle, and what the ring tests share:

* :func:`trajectory` steps the oracle one pivot at a time and follows the labels x1 / x2 the way
  ``batch_util.label_places`` does (simplex.py:152);
* :func:`expected_rings` simulates both rings from sentinels: every slot a pivot reaches holds that
  pivot, every other element -- guard bands included -- still holds its sentinel;
* :func:`install` / :func:`poison` put those sentinels on the device, :func:`check` compares the
  whole arrays as bit patterns: right slot, right value, no stray and no missed write in one
  comparison.

Sentinels: ``log`` element ``e`` of the whole array holds ``-(1000 + e)`` (no row or column is
negative); ``xhist`` element ``e`` holds a quiet NaN whose payload is ``e + 1``, so a right value
in a wrong slot, or one sentinel copied over another, is seen as well.
"""
from __future__ import annotations

import hashlib
from dataclasses import dataclass

import numpy as np

GUARD = 64            # elements of the ring's type on either side of an installed ring
QNAN = 0x7FF8000000000000


def log_sentinels(count: int) -> np.ndarray:
    """int32[count]: element e holds -(1000 + e)."""
    return (-(1000 + np.arange(count, dtype=np.int64))).astype(np.int32)


def xhist_sentinels(count: int) -> np.ndarray:
    """int64[count] bit patterns: element e is a quiet NaN with payload e + 1."""
    return np.int64(QNAN) | (np.arange(count, dtype=np.int64) + 1)


# The LPs of the ring tests: kind, seed, n, m (lp.dense_tableau).  By the C oracle the first eight
# take all 40 pivots asked of them (tests/test_ring_oracle.py keeps a census of what the labels do
# in them); C reaches the optimum after 7 pivots and D ends "incorrect" after 10, as in
# tests/test_gpu_chain_forms.py.
LPS = {
    "u0": ("uniform", 0, 37, 45), "u3": ("uniform", 3, 96, 70), "u1": ("uniform", 1, 300, 260),
    "m2": ("mixed", 2, 150, 130), "m0": ("mixed", 0, 300, 260),
    "d1": ("degenerate", 1, 37, 45), "dm1": ("degenerate_mixed", 1, 37, 45),
    "d0": ("degenerate", 0, 37, 45),
    "C": ("uniform", 0, 9, 5), "D": ("mixed", 0, 9, 5),
}
PIVOTS = 40
_LP: dict[str, tuple] = {}


def lp_case(name: str):
    """(T, n, m) of LPS[name], made once and read-only."""
    if name not in _LP:
        from simplex_mi355x import lp
        kind, seed, n, m = LPS[name]
        T = lp.dense_tableau(kind, seed, n, m)
        T.setflags(write=False)
        _LP[name] = (T, n, m)
    return _LP[name]


def expected(name: str, asked: int, log_cap: int, lead: int = GUARD, world: int = 0) -> "Rings":
    """expected_rings for LPS[name]; ``world`` > 0: per-rank rings for the project's row_range."""
    T, n, m = lp_case(name)
    ranges = None
    if world:
        from simplex_mi355x.sharded import row_range
        ranges = [row_range(n, p, world) for p in range(world)]
    return expected_rings(T, n, m, m, asked, log_cap, lead, ranges)


@dataclass(frozen=True)
class Trajectory:
    """The oracle's pivots from one table.  ``rows[t, q]``: the row label q is basic in after
    pivot t, -1 when it is not basic; ``xbits[t, q]``: the bits of (x1, x2) after pivot t -- the
    "-b" entry of that row in T_{t+1}, +0.0 (bits 0) for a non-basic label (simplex.py:51-68)."""
    pivots: np.ndarray     # int32[done][2]
    rows: np.ndarray       # int64[done][2]
    xbits: np.ndarray      # int64[done][2]
    status: int            # the terminal pick that ended it; 0 when every pivot asked was taken
    table: np.ndarray      # the table after the last pivot

    @property
    def done(self) -> int:
        return len(self.pivots)

    @property
    def x(self) -> np.ndarray:
        return self.xbits.view(np.float64)


_TRAJ: dict[tuple, Trajectory] = {}


def trajectory(T, n: int, m: int, flen: int, asked: int) -> Trajectory:
    """Up to ``asked`` pivots of c_oracle.pick + c_oracle.pivot from T (memoised)."""
    from oracle import c_oracle
    T = np.ascontiguousarray(T, dtype=np.float64)
    key = (hashlib.sha1(T.tobytes()).hexdigest(), T.shape, n, m, flen, asked)
    if key in _TRAJ:
        return _TRAJ[key]
    cur = T.copy()
    where = [-1, -2]       # multi._move's codes: row p >= 0, column j as -(j + 1)
    pivots, rows, xbits = [], [], []
    status = 0
    for _ in range(asked):
        status, r, c = c_oracle.pick(cur, n, m, flen)
        if status != 0:
            break
        cur = c_oracle.pivot(cur, r, c)
        for q in (0, 1):
            if where[q] == -(c + 1):
                where[q] = r
            elif where[q] == r:
                where[q] = -(c + 1)
        pivots.append((r, c))
        rows.append([w if w >= 0 else -1 for w in where])
        xbits.append([int(cur[w:w + 1, m].view(np.int64)[0]) if w >= 0 else 0 for w in where])
    else:
        status = 0         # the chain was not asked for the pick after its last pivot
    out = Trajectory(np.array(pivots, dtype=np.int32).reshape(-1, 2),
                     np.array(rows, dtype=np.int64).reshape(-1, 2),
                     np.array(xbits, dtype=np.int64).reshape(-1, 2), int(status), cur)
    for a in (out.pivots, out.rows, out.xbits, out.table):
        a.setflags(write=False)
    _TRAJ[key] = out
    return out


@dataclass
class Rings:
    traj: Trajectory
    log_cap: int
    lead: int
    log: np.ndarray               # int32, the whole array (bands included), one device
    xhist: np.ndarray             # int64 bit patterns, the whole array
    ranks: list | None = None     # per rank of a sharded run: (log, xhist) like the two above

    @property
    def done(self) -> int:
        return self.traj.done


def _simulate(traj: Trajectory, cap: int, lead: int, own=None):
    """Both rings after traj's pivots, from sentinels.  ``own``: the (lo, hi) rows of one rank of
    a sharded run -- that rank writes a basic label's value only for a row it owns and leaves the
    slot as it stood otherwise (include/smx.h, smx_bshard_*)."""
    log = log_sentinels(2 * cap + 2 * lead)
    xh = xhist_sentinels(2 * cap + 2 * lead)
    for t in range(traj.done):
        s = lead + 2 * (t % cap)
        log[s:s + 2] = traj.pivots[t]
        for q in (0, 1):
            i = int(traj.rows[t, q])
            if i < 0:
                xh[s + q] = 0
            elif own is None or own[0] <= i < own[1]:
                xh[s + q] = traj.xbits[t, q]
    return log, xh


def expected_rings(T, n: int, m: int, flen: int, asked: int, log_cap: int, lead_sentinels: int,
                   ranges=None) -> Rings:
    """The rings after a chain (or several) that asked for ``asked`` pivots in all from T, as
    whole arrays with ``lead_sentinels`` guard elements on either side.  With ``ranges`` (the
    row_range blocks of a sharded run) ``.ranks`` holds one pair per rank; every rank logs every
    pivot.  Nothing is written for a pivot that did not happen."""
    traj = trajectory(T, n, m, flen, asked)
    log, xh = _simulate(traj, log_cap, lead_sentinels)
    out = Rings(traj, log_cap, lead_sentinels, log, xh)
    if ranges is not None:
        out.ranks = [_simulate(traj, log_cap, lead_sentinels, own=tuple(rg)) for rg in ranges]
    return out


def owners(traj: Trajectory, ranges) -> np.ndarray:
    """int64[done][2]: the rank that owns each label's row after every pivot, -1 if non-basic."""
    out = np.full(traj.rows.shape, -1, dtype=np.int64)
    for p, (lo, hi) in enumerate(ranges):
        out[(traj.rows >= lo) & (traj.rows < hi)] = p
    return out


# -- the device side ------------------------------------------------------------------------------
def install(dev, log_cap: int) -> None:
    """Replace the rings of a fresh DeviceTableau by interior views of poisoned tensors with
    GUARD elements on either side (256 B / 512 B: the views stay contiguous and 16-byte aligned).
    Before the first run / prepare: graphs capture the ring pointers."""
    import torch
    assert dev.step == 0 and not dev._graphs and not dev._pending
    with torch.cuda.stream(dev.stream):
        log = torch.from_numpy(log_sentinels(2 * log_cap + 2 * GUARD)).to(dev.device)
        xh = torch.from_numpy(xhist_sentinels(2 * log_cap + 2 * GUARD)).to(dev.device)
        dev.log = log[GUARD:GUARD + 2 * log_cap]
        dev.xhist = xh.view(torch.float64)[GUARD:GUARD + 2 * log_cap]
    assert dev.log.is_contiguous() and dev.xhist.is_contiguous()
    assert dev.log.data_ptr() % 16 == 0 and dev.xhist.data_ptr() % 16 == 0
    dev.log_cap = log_cap
    dev._ring_whole = (log, xh, GUARD)


def poison(dev) -> None:
    """The same sentinels written into the rings a DeviceTableau was built with (``log_cap=``),
    for owners whose ring pointers are taken at construction; no guard bands."""
    import torch
    assert dev.step == 0
    assert dev.log.numel() == 2 * dev.log_cap and dev.xhist.numel() == 2 * dev.log_cap
    with torch.cuda.stream(dev.stream):
        dev.log.copy_(torch.from_numpy(log_sentinels(2 * dev.log_cap)))
        dev.xhist.view(torch.int64).copy_(torch.from_numpy(xhist_sentinels(2 * dev.log_cap)))
    dev.stream.synchronize()
    dev._ring_whole = (dev.log, dev.xhist.view(torch.int64), 0)


def read_whole(dev):
    """(log int32, xhist int64 bits, guard) of a DeviceTableau after install / poison."""
    import torch
    log, xh, lead = dev._ring_whole
    torch.cuda.synchronize(dev.device)
    return log.cpu().numpy().copy(), xh.cpu().numpy().copy(), lead


def _diff(name, got, exp, lead):
    bad = np.nonzero(got != exp)[0]
    if len(bad) == 0:
        return None
    e = int(bad[0])
    return (f"{name}: {len(bad)} elements differ, first at element {e} (ring slot "
            f"{(e - lead) // 2}, field {(e - lead) % 2}): got {int(got[e]):#x}, "
            f"expected {int(exp[e]):#x}")


def check(dev_or_rank, expected, rank: int | None = None, xhist: bool = True) -> None:
    """The whole ``log`` and ``xhist`` arrays of a DeviceTableau (or of a shard backend's
    ``.dev``) equal the simulation, bit for bit.  ``rank``: compare with that rank's rings of a
    sharded expectation.  ``xhist=False``: the form under test takes no x-history ring, so every
    element of it must still be its sentinel."""
    dev = getattr(dev_or_rank, "dev", dev_or_rank)
    log, xh, lead = read_whole(dev)
    assert lead == expected.lead and len(log) == len(expected.log)
    elog, exh = (expected.log, expected.xhist) if rank is None else expected.ranks[rank]
    if not xhist:
        exh = xhist_sentinels(len(exh))
    errs = [_diff("log", log, elog, lead), _diff("xhist", xh, exh, lead)]
    errs = [e for e in errs if e]
    assert not errs, "; ".join(errs)
