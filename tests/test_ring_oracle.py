"""CPU: the ring simulation of tests/ring_util.py pinned to the reference's fixtures, and a census of
the LPs that tests/test_gpu_rings.py runs -- asserted, so that those inputs keep the edges the GPU
tests rely on (labels that leave and re-enter the basis inside a wrapped ring, basic values that
are exactly zero, labels owned by different ranks of a sharded run).
"""
from __future__ import annotations

import numpy as np
import pytest

import ring_util
from golden_util import dec, same_value, trajectory_cap, trajectory_cases
from oracle import numpy_oracle
from ring_util import LPS, PIVOTS, expected, lp_case, owners, trajectory

CASES = [c for c in trajectory_cases()
         if c[3]["outcome"]["kind"] != "exception" and len(c[2]) >= 2
         and len(c[2]) in (len(c[1][0]) - 1, len(c[1][0]))]


def test_fixture_filter_keeps_most_cases():
    assert len(CASES) > 250


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_helper_matches_fixture_x_history(case):
    """Per pivot, the helper's (x1, x2) -- read back from a ring that never wraps -- and its
    (r, c) equal the values the reference recorded for that step."""
    label, cons, func, rec = case
    T, n, m, flen = numpy_oracle.to_dense(cons, func)
    cap = trajectory_cap(rec)
    steps = rec["steps"]
    rings = ring_util.expected_rings(T, n, m, flen, cap, max(cap, 1), 3)
    assert rings.done == len(steps) - 1, label
    log = rings.log[3:-3].reshape(-1, 2)
    xs = rings.xhist[3:-3].view(np.float64).reshape(-1, 2)
    for t in range(rings.done):
        assert (int(log[t, 0]), int(log[t, 1])) == (steps[t]["i"], steps[t]["j"]), (label, t)
        assert same_value(float(xs[t, 0]), dec(steps[t + 1]["x1"])), (label, t)
        assert same_value(float(xs[t, 1]), dec(steps[t + 1]["x2"])), (label, t)
    kind = rec["outcome"]["kind"]
    assert (rings.traj.status == 0) == (kind == "cap"), label
    # the guard elements and the slots no pivot reached still hold their sentinels
    assert np.array_equal(rings.log[:3], ring_util.log_sentinels(3))
    assert np.array_equal(rings.xhist[:3], ring_util.xhist_sentinels(3))
    tail = 3 + 2 * rings.done
    assert np.array_equal(rings.log[tail:], ring_util.log_sentinels(len(rings.log))[tail:])
    assert np.array_equal(rings.xhist[tail:], ring_util.xhist_sentinels(len(rings.log))[tail:])


@pytest.mark.parametrize("name", list(LPS))
def test_small_ring_is_the_rotated_tail_of_the_unbounded_one(name):
    """log_cap = 5: slot s holds the last pivot t with t % 5 == s -- the last five rows of a ring
    that never wraps, rotated; bands untouched.  Per rank of three as well: a slot a rank last
    left alone (a basic label another rank owns) keeps what that rank wrote there before."""
    asked = PIVOTS if name not in ("C", "D") else 12
    full = expected(name, asked, 64, lead=0, world=3)
    small = expected(name, asked, 5, lead=7, world=3)
    done = full.done
    assert done == small.done and done >= 7
    flog = full.log.reshape(-1, 2)
    fx = full.xhist.reshape(-1, 2)
    slog = small.log[7:-7].reshape(-1, 2)
    sx = small.xhist[7:-7].reshape(-1, 2)
    for t in range(done - 5, done):
        assert np.array_equal(slog[t % 5], flog[t]) and np.array_equal(sx[t % 5], fx[t])
    assert np.array_equal(small.log[:7], ring_util.log_sentinels(7))
    assert np.array_equal(small.log[-7:], ring_util.log_sentinels(24)[-7:])
    assert np.array_equal(small.xhist[:7], ring_util.xhist_sentinels(7))
    assert np.array_equal(small.xhist[-7:], ring_util.xhist_sentinels(24)[-7:])
    own = owners(full.traj, _ranges(name, 3))
    for p, (rlog, rx) in enumerate(small.ranks):
        assert np.array_equal(rlog, small.log)
        rx = rx[7:-7].reshape(-1, 2)
        for s in range(5):
            for q in (0, 1):
                # the last pivot in this slot at which rank p wrote label q
                ts = [t for t in range(s, done, 5) if own[t, q] in (-1, p)]
                want = fx[ts[-1], q] if ts else ring_util.xhist_sentinels(24)[7 + 2 * s + q]
                assert rx[s, q] == want, (p, s, q)


def _ranges(name, world):
    from simplex_mi355x.sharded import row_range
    n = LPS[name][2]
    return [row_range(n, p, world) for p in range(world)]


def _census(name):
    """(pivots, pivots with x1 / x2 basic, basis <-> non-basis moves of x1 / x2)."""
    T, n, m = lp_case(name)
    tr = trajectory(T, n, m, m, PIVOTS)
    basic = tr.rows >= 0
    prev = np.vstack([[False, False], basic[:-1]])
    moves = (basic != prev).sum(axis=0)
    return tr.done, tuple(int(x) for x in basic.sum(axis=0)), tuple(int(x) for x in moves)


# name: (pivots with x1 / x2 basic, basis <-> non-basis moves), all of 40 pivots, by the C oracle
CENSUS = {
    "u0": ((9, 36), (6, 4)), "u3": ((28, 4), (7, 6)), "u1": ((1, 20), (2, 7)),
    "m2": ((22, 19), (5, 5)), "m0": ((29, 18), (7, 7)),
    "d1": ((36, 37), (5, 3)), "dm1": ((32, 29), (5, 5)), "d0": ((20, 0), (40, 0)),
}


@pytest.mark.parametrize("name", list(CENSUS))
def test_census_of_the_gpu_inputs(name):
    done, basic, moves = _census(name)
    assert done == PIVOTS
    assert (basic, moves) == CENSUS[name]


def test_terminal_inputs():
    """C: the optimum after 7 pivots; D: "incorrect" after 10 (12 asked)."""
    for name, want in (("C", (1, 7)), ("D", (2, 10))):
        T, n, m = lp_case(name)
        tr = trajectory(T, n, m, m, 12)
        assert (tr.status, tr.done) == want


def _trajs():
    return {name: trajectory(*lp_case(name), LPS[name][3], PIVOTS) for name in CENSUS}


@pytest.mark.parametrize("cap", [5, 8])
def test_labels_basic_and_non_basic_inside_the_last_ring(cap):
    """Over the set, inside the last ``cap`` pivots (what a wrapped ring still holds) each label
    is basic in some LP and non-basic in some LP; some LP has a label doing both there."""
    seen = {(q, b): 0 for q in (0, 1) for b in (False, True)}
    both = 0
    for name, tr in _trajs().items():
        tail = tr.rows[-cap:] >= 0
        for q in (0, 1):
            for b in (False, True):
                seen[q, b] += bool((tail[:, q] == b).any())
            both += bool(tail[:, q].any() and not tail[:, q].all())
    assert all(v > 0 for v in seen.values()), seen
    assert both > 0


def test_each_label_re_enters_after_leaving():
    """basic -> non-basic -> basic for x1 and for x2, in at least one LP each."""
    found = [0, 0]
    for tr in _trajs().values():
        for q in (0, 1):
            b = (tr.rows[:, q] >= 0).astype(int)
            flips = np.nonzero(np.diff(np.concatenate([[0], b])))[0]
            found[q] += len(flips) >= 3      # in, out, in
    assert found[0] > 0 and found[1] > 0


def test_a_basic_label_is_exactly_zero():
    """A basic label whose value is +-0.  +0.0 has the bits a non-basic label gets: d1 has one
    such pivot for each label (pivot 4), dm1 one for x1 (pivot 29).  -0.0 differs from them in
    the sign alone: x1 of d0 on each of the 20 pivots it is basic after."""
    trs = _trajs()
    zeros = {}
    for name, tr in trs.items():
        zero = (tr.rows >= 0) & (tr.x == 0.0)
        zeros[name] = tuple(int(v) for v in zero.sum(axis=0))
        neg = zero & (tr.xbits != 0)
        assert bool(neg.any()) == (name == "d0"), name
    assert zeros == {"u0": (0, 0), "u3": (0, 0), "u1": (0, 0), "m2": (0, 0), "m0": (0, 0),
                     "d1": (1, 1), "dm1": (1, 0), "d0": (20, 0)}


def test_a_label_enters_in_the_pivot_row():
    """A label is basic in the pivot row of the same pivot (it entered at this step): the new
    value is the pivot row's own new "-b" entry, not a row updated from it."""
    for q in (0, 1):
        assert any((tr.rows[:, q] == tr.pivots[:, 0]).any() for tr in _trajs().values()), q


def test_a_label_moves_on_every_pivot():
    tr = _trajs()["d0"]
    b = tr.rows[:, 0] >= 0
    assert np.array_equal(b, np.arange(PIVOTS) % 2 == 0)


# the LPs whose labels change owner among three ranks (ring_util.owners with row_range)
TWO_OWNERS = ("u0", "u3")


def _owner_sets(name, cap):
    """Per label, the ranks of three that own it inside the windows the GPU tests check (the
    last ``cap`` pivots before the checks after 1, 10 and 40 pivots), and whether x1 and x2
    have different owners at some pivot there."""
    T, n, m = lp_case(name)
    own = owners(trajectory(T, n, m, m, PIVOTS), _ranges(name, 3))
    ranks, differ = [set(), set()], False
    for stop in (1, 10, PIVOTS):
        win = own[max(0, stop - cap):stop]
        for q in (0, 1):
            ranks[q] |= set(win[:, q][win[:, q] >= 0].tolist())
        differ = differ or bool(((win[:, 0] >= 0) & (win[:, 1] >= 0)
                                 & (win[:, 0] != win[:, 1])).any())
    return ranks, differ


def test_three_ranks_share_the_labels():
    """World 3 with the project's row_range.  A ring that never wraps (log_cap 64): in u0 and in
    u3 each label is owned by two or more ranks and x1 and x2 have different owners at some
    pivot -- the `row * 3 // n` estimate holds with row_range, no other seed was needed.  With
    log_cap 5 a check sees the last five pivots only: no single LP keeps both labels on two
    ranks inside those windows, but over u0 and u3 together each label is on two ranks and both
    LPs have a pivot with different owners.  dm1 moves x1 from rank 0 to rank 1 (a mixed LP:
    the older sharded tests' mixed inputs keep both labels on rank 0)."""
    for name in TWO_OWNERS:
        ranks, differ = _owner_sets(name, 64)
        assert len(ranks[0]) >= 2 and len(ranks[1]) >= 2 and differ, name
    union = [set(), set()]
    for name in TWO_OWNERS:
        ranks, differ = _owner_sets(name, 5)
        assert differ, name
        union = [union[q] | ranks[q] for q in (0, 1)]
    assert len(union[0]) >= 2 and len(union[1]) >= 2
    assert _owner_sets("dm1", 64)[0][0] == {0, 1}
