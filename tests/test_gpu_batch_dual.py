"""GPU: the dual-simplex selection rule (SMX_RULE_DUAL, include/smx.h) on the device -- one step of
each of the three dual batch kernels on the hand-made tables with the winner and its runner-up
placed across lanes, waves and walks; whole chains from warm tables; the `_rule` entries under
rule 0 against the entries without a rule; their refusals; and the public calls with
warm_rule="dual" / rule="dual" -- against dual_util's restatement by bit pattern."""
from __future__ import annotations

import numpy as np
import pytest

import cuts_util as cu
import dual_util as du
import ranging_util as ru
import scenario_util as scu
import solution_util as su
from batch_util import case

pytestmark = pytest.mark.gpu

ENTRY = {"wave": "smx_batch_solve", "workgroup": "smx_batch_solve_wg",
         "global": "smx_batch_solve_gm"}
GUARD = 64
P_OUT, P_INT = 7.0, 77


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


# ----------------------------------------------------------------------------------------------
# one launch through the C ABI
def _block(T, n, m, Rmax, ldb):
    """T in an Rmax x ldb block whose padding would show: +9 to the right of the constraint rows
    (a candidate with a small ratio if a dual step read it), -9 to the right of the f-row (a
    negative cost if the f-row scan overran, the smallest ratio if a dual step read it) and -9
    below the f-row (a negative constant if the row scan overran)."""
    blk = np.full((Rmax, ldb), 9.0)
    blk[n:, :] = -9.0
    blk[:n + 1, :m + 1] = np.asarray(T, dtype=np.float64)[:n + 1, :m + 1]
    return blk


def _guarded(torch, shape, dtype, poison):
    count = int(np.prod(shape))
    whole = torch.full((count + 2 * GUARD,), poison, dtype=dtype, device="cuda")
    return whole, whole[GUARD:GUARD + count]


def _launch(tier, lps, Rmax, ldb, cap, rule):
    """lps: [(T, n, m, flen)], or None for an LP whose dims lie outside the block -> the outputs
    of one launch of `tier`'s `_rule` entry (rule None: the entry without a rule).  Every output
    starts poisoned and stands between poisoned guard bands that must come back untouched."""
    import torch
    from simplex_mi355x import _lib
    B = len(lps)
    tabs = np.full((B, Rmax, ldb), 3.25)
    dims = np.zeros((B, 3), dtype=np.int32)
    for q, lp_ in enumerate(lps):
        if lp_ is None:
            dims[q] = (Rmax, ldb, ldb)
            continue
        T, n, m, flen = lp_
        tabs[q] = _block(T, n, m, Rmax, ldb)
        dims[q] = (n, m, flen)
    d_tabs = torch.from_numpy(tabs).to("cuda")
    d_dims = torch.from_numpy(dims).to("cuda")
    P = max(cap, 1)
    bufs = {"out": _guarded(torch, (B, Rmax, ldb), torch.float64, P_OUT),
            "rc": _guarded(torch, (B, P, 2), torch.int32, P_INT),
            "xv": _guarded(torch, (B, P, 2), torch.float64, P_OUT),
            "status": _guarded(torch, (B,), torch.int32, P_INT),
            "npivots": _guarded(torch, (B,), torch.int32, P_INT)}
    args = (d_tabs.data_ptr(), d_dims.data_ptr(), B, Rmax, ldb, cap, bufs["out"][1].data_ptr(),
            bufs["rc"][1].data_ptr(), bufs["xv"][1].data_ptr(), None,
            bufs["status"][1].data_ptr(), bufs["npivots"][1].data_ptr())
    stream = torch.cuda.current_stream().cuda_stream
    L = _lib.load()
    if rule is None:
        err = getattr(L, ENTRY[tier])(*args, stream)
    else:
        err = getattr(L, ENTRY[tier] + "_rule")(*args, rule, stream)
    torch.cuda.synchronize()
    res = {"err": int(err)}
    shapes = {"out": (B, Rmax, ldb), "rc": (B, P, 2), "xv": (B, P, 2), "status": (B,),
              "npivots": (B,)}
    for key, (whole, view) in bufs.items():
        h = whole.cpu().numpy()
        poison = P_OUT if h.dtype == np.float64 else P_INT
        assert (h[:GUARD] == poison).all() and (h[-GUARD:] == poison).all(), (key, "guard band")
        res[key] = view.cpu().numpy().reshape(shapes[key])
    return res


def _same_lp(res, q, lp_, cap, rule, what, nan_aware=False, exp=None):
    """LP q of a launch against the restatement: status, pivot count, log (the slots past it
    untouched) and the whole Rmax x ldb output block (untouched outside rows 0..n, columns 0..m)."""
    T, n, m, flen = lp_
    exp = exp or du.run(T, n, m, flen, cap, rule)
    final, st, done, log, _ = exp
    assert int(res["status"][q]) == st and int(res["npivots"][q]) == done, \
        (what, int(res["status"][q]), int(res["npivots"][q]), st, done)
    assert np.array_equal(res["rc"][q, :done], log), (what, res["rc"][q, :done].tolist(), log.tolist())
    assert (res["rc"][q, done:] == P_INT).all(), (what, "log slots past the run")
    want = np.full(res["out"][q].shape, P_OUT)
    want[:n + 1, :m + 1] = final
    assert su.same_floats(res["out"][q], want, nan_aware), \
        (what, np.argwhere(su.bits(res["out"][q]) != su.bits(want))[:4].tolist())
    return exp


def _idle_lp(res, q, what):
    assert int(res["status"][q]) == du.IDLE and int(res["npivots"][q]) == 0, what
    assert (res["out"][q] == P_OUT).all() and (res["rc"][q] == P_INT).all(), what


def _filler(n, m, nb):
    """A primal- and dual-feasible table: `optimum` without a pivot under either rule."""
    T = du.blank(n, m, nb)
    T[:n, m] = 2.0
    return T


def _cols(m, turn):
    """Six columns for dual_util.handmade's events at width m: the tie's two columns (and so the
    winner and its runner-up) at the two ends, then the two swapped with the ends moved inwards."""
    if m < 6:
        return ((2, 1, 0, 1, 0, 0), (0, 2, 1, 2, 1, 1))[turn]
    if turn == 0:
        return (m - 1, 1, 0, m - 2, 2, 3)
    return (2, m - 2, m // 2, 0, 1, m - 1)


def _one_step(tier, n, m, nb, Rmax=None, ldb=None):
    """Every hand-made case at two placements: the case's table as LPs 0, 1 and 4 of a five-LP
    launch, LP 2 with dims outside the block (on the wave tier, whose kernel states no rule for
    such dims, a second filler) and LP 3 a filler; max_pivots = 1."""
    Rmax, ldb = Rmax or n + 2, ldb or m + 3
    fill = (_filler(n, m, nb), n, m, m)
    seen = set()
    for turn in (0, 1):
        for name, T, _, _, flen, want, dual in du.handmade(n, m, nb, _cols(m, turn)):
            lp_ = (T, n, m, flen)
            res = _launch(tier, [lp_, lp_, fill if tier == "wave" else None, fill, lp_], Rmax, ldb,
                          1, du.DUAL)
            assert res["err"] == 0
            exp = None
            for q in (0, 1, 4):
                exp = _same_lp(res, q, lp_, 1, du.DUAL, (tier, n, m, name, turn, q), True, exp)
            assert (exp[1], exp[2]) == ((du.PIVOT, 1) if want[0] == du.PIVOT else (want[0], 0))
            if want[0] == du.PIVOT:
                assert tuple(exp[3][0]) == want[1:], (name, exp[3], want)
                seen.add(want[2])
            _same_lp(res, 3, fill, 1, du.DUAL, (tier, name, "filler"))
            if tier == "wave":
                _same_lp(res, 2, fill, 1, du.DUAL, (tier, name, "filler"))
            else:
                _idle_lp(res, 2, (tier, name, "dims outside"))
    return seen


WAVE = [(n, m) for m in (3, 7, 15, 31, 63) for n in (1, 63)]


@pytest.mark.parametrize("n,m", WAVE, ids=[f"{n}x{m}" for n, m in WAVE])
def test_one_step_wave(n, m):
    """One m per CMAX instantiation (ldb = m + 1 = 4, 8, 16, 32, 64), one row and a full
    wavefront of rows with the offending row the last constraint."""
    seen = _one_step("wave", n, m, n - 1, Rmax=n + 1, ldb=m + 1)
    assert {0, m - 1} <= seen or m < 6


WORKGROUP = [(71, 63, 70), (71, 64, 70), (71, 65, 70), (5, 255, 2), (5, 256, 2), (5, 257, 2),
             (71, 257, 70)]


@pytest.mark.parametrize("n,m,nb", WORKGROUP, ids=[f"{n}x{m}" for n, m, _ in WORKGROUP])
def test_one_step_workgroup(n, m, nb):
    """Columns one short of a wave, a wave and one past it at 256 threads; 255, 256 and 257 columns
    at 256 threads (column 256 is a thread's second walk) and 257 at 1024 (five waves hold
    candidates); the offending row past the first wave of rows where the table has them."""
    from simplex_mi355x.batch import wg_lds_bytes
    assert wg_lds_bytes(n + 2, m + 3) >= 0
    seen = _one_step("workgroup", n, m, nb)
    assert {1, m - 2} <= seen


GLOBAL = [(142, 142, 70), (3, 1100, 2)]


@pytest.mark.parametrize("n,m,nb", GLOBAL, ids=[f"{n}x{m}" for n, m, _ in GLOBAL])
@pytest.mark.parametrize("knobs", ((1024, 0, 8), (256, 1, 4)), ids=("default", "mirrors"))
def test_one_step_global(n, m, nb, knobs):
    """Past the LDS edge, and a 3 x 1100 table whose column walk passes 1024 threads; under the
    default knobs and with 256 threads, the LDS mirrors and 4 loads ahead."""
    from simplex_mi355x import _lib
    L = _lib.load()
    prev = L.smx_tune_batch_gm(*knobs)
    try:
        seen = _one_step("global", n, m, nb)
    finally:
        L.smx_tune_batch_gm(prev & 0xffff, (prev >> 16) & 0xf, prev >> 20)
    assert L.smx_tune_batch_gm(-1, -1, -1) == prev
    assert {1, m - 2} <= seen


# ----------------------------------------------------------------------------------------------
# whole chains
CHAINS = [("wave", 20, 3, (0, 2, 3), 64), ("workgroup", 65, 65, (0, 1), 1024),
          ("global", 142, 142, (1, 2), 4096)]
WARM_CAP = 48


def _base(n, m, seed, cap):
    ref = case("uniform", n, m, seed, cap, m)
    assert ref[3] == 1, (n, m, seed, "the base run ends at `optimum`")
    basis, nonbasis, _ = su.replay(ref[5], n, m)
    return ref, basis, nonbasis


def _warm_lps(n, m, seed, cap):
    """Warm tables of one base LP: two rhs-only scenarios, one cut, the scenario with its cost
    deltas kept, and the cold LP itself (which takes no dual step)."""
    ref, basis, nonbasis = _base(n, m, seed, cap)
    T0, _, Tf = ref[0], ref[1], ref[2]
    lps = []
    for s in (0, 1):
        drhs, dcost = scu.deltas(T0, n, m, seed, s, 0.2, 0.5)
        S, _ = scu.restate(Tf, n, m, basis, nonbasis, T0[n, :m], drhs, np.zeros(m))
        lps.append((S, n, m, m))
    _, E, _, _, _ = cu.cuts_of_case(ref, n, m, seed, 0, 1, viol=0.2)
    lps.append((E, n + 1, m, m))
    drhs, dcost = scu.deltas(T0, n, m, seed, 0, 0.2, 0.5)
    S, _ = scu.restate(Tf, n, m, basis, nonbasis, T0[n, :m], drhs, dcost)
    lps.append((S, n, m, m))
    lps.append((np.array(T0), n, m, m))
    return lps


@pytest.mark.parametrize("tier,n,m,seeds,cap", CHAINS, ids=[c[0] for c in CHAINS])
def test_whole_chains(tier, n, m, seeds, cap):
    """One mixed launch per tier: log, status, pivot count and final block of every LP against the
    restatement, bit for bit.  Some LPs take dual steps only, some none at all."""
    lps = [lp_ for seed in seeds for lp_ in _warm_lps(n, m, seed, cap)]
    res = _launch(tier, lps, n + 2, m + 1 + (2 if m + 3 <= 64 or tier != "wave" else 0), WARM_CAP,
                  du.DUAL)
    assert res["err"] == 0
    only, none, pivots = 0, 0, 0
    for q, lp_ in enumerate(lps):
        exp = _same_lp(res, q, lp_, WARM_CAP, du.DUAL, (tier, q))
        only += exp[2] > 0 and exp[4] == exp[2]
        none += exp[2] > 0 and exp[4] == 0
        pivots += exp[2]
    assert only >= 2 and none >= 1 and pivots > 0, (only, none, pivots)


@pytest.mark.parametrize("tier,n,m,seeds,cap", CHAINS, ids=[c[0] for c in CHAINS])
def test_rule_zero_is_the_entry_without_a_rule(tier, n, m, seeds, cap):
    """The `_rule` entry under SMX_RULE_REFERENCE and the entry without a rule on the same input:
    every output byte equal."""
    lps = [lp_ for seed in seeds for lp_ in _warm_lps(n, m, seed, cap)]
    a = _launch(tier, lps, n + 2, m + 1, 24, du.REFERENCE)
    b = _launch(tier, lps, n + 2, m + 1, 24, None)
    assert a["err"] == b["err"] == 0
    for key in ("out", "rc", "xv", "status", "npivots"):
        assert a[key].tobytes() == b[key].tobytes(), (tier, key)
    assert int(b["npivots"].sum()) > 0
    ref = du.run(*lps[0], 24, du.REFERENCE)
    _same_lp(a, 0, lps[0], 24, du.REFERENCE, (tier, "reference"), exp=ref)


_GM_CASE = {}


def _gm_case(rule):
    """The global tier's LPs for the knob sweep and their restated runs under `rule`, made once:
    the ("global", 142, 142, ...) chain's warm tables and the (142, 142, 70) hand-made one-step
    tables, all capped at 24 pivots."""
    if not _GM_CASE:
        _, n, m, seeds, cap = CHAINS[2]
        _GM_CASE["chain"] = [lp_ for seed in seeds for lp_ in _warm_lps(n, m, seed, cap)]
        n, m, nb = GLOBAL[0]
        _GM_CASE["hand"] = [(T, n, m, flen)
                            for _, T, _, _, flen, _, _ in du.handmade(n, m, nb, _cols(m, 0))]
    if rule not in _GM_CASE:
        _GM_CASE[rule] = [du.run(*lp_, 24, rule) for lp_ in _GM_CASE["chain"] + _GM_CASE["hand"]]
    return _GM_CASE["chain"], _GM_CASE["hand"], _GM_CASE[rule]


@pytest.mark.parametrize("mirrors,unroll", [(mi, u) for mi in (0, 1) for u in (1, 4, 8)])
def test_every_global_knob_pair_under_both_rules(mirrors, unroll):
    """smx_batch_solve_gm_rule picks one of twelve instantiations from (mirrors, unroll, rule):
    each of them on one launch of the chain's warm tables and the hand-made one-step tables, at 256
    threads (80 elements a thread: every look-ahead depth runs and leaves a tail), against the
    restatement bit for bit."""
    from simplex_mi355x import _lib
    L = _lib.load()
    _, n, m, _, _ = CHAINS[2]
    prev = L.smx_tune_batch_gm(256, mirrors, unroll)
    try:
        for rule in (du.REFERENCE, du.DUAL):
            chain, hand, exps = _gm_case(rule)
            res = _launch("global", chain + hand, n + 2, m + 3, 24, rule)
            assert res["err"] == 0
            for q, (lp_, exp) in enumerate(zip(chain + hand, exps)):
                _same_lp(res, q, lp_, 24, rule, (mirrors, unroll, rule, q), q >= len(chain), exp)
            assert all(sum(e[2] for e in part) > 0 for part in (exps[:len(chain)], exps[len(chain):]))
            assert (sum(e[4] for e in exps) > 0) == (rule == du.DUAL)
    finally:
        L.smx_tune_batch_gm(prev & 0xffff, (prev >> 16) & 0xf, prev >> 20)
    assert L.smx_tune_batch_gm(-1, -1, -1) == prev


def test_rule_entries_refuse():
    """Every refusal of the `_rule` entries with real device pointers: an unknown rule, a bad
    shape, a negative count or cap -- hipErrorInvalidValue, nothing launched, nothing written."""
    fill = (_filler(5, 6, 2), 5, 6, 6)
    for tier, good, bad in (("wave", (7, 8), ((65, 8), (7, 65), (0, 8))),
                            ("workgroup", (7, 8), ((1, 8), (7, 1), (400, 400))),
                            ("global", (7, 8), ((1, 8), (7, 1), (800, 800)))):
        for rule in (2, -1, 1 << 16):
            res = _launch(tier, [fill, fill], *good, 4, rule)
            assert res["err"] == 1, (tier, rule)
            assert (res["out"] == P_OUT).all() and (res["status"] == P_INT).all(), (tier, rule)
        assert _launch(tier, [fill, fill], *good, -1, du.DUAL)["err"] == 1
        assert _launch(tier, [fill, fill], *good, 4, du.DUAL)["err"] == 0
    from simplex_mi355x import _lib
    L = _lib.load()
    null = [None] * 6
    for tier, good, bad in (("wave", (7, 8), ((65, 8), (7, 65), (0, 8))),
                            ("workgroup", (7, 8), ((1, 8), (7, 1), (400, 400))),
                            ("global", (7, 8), ((1, 8), (7, 1), (800, 800)))):
        ruled = getattr(L, ENTRY[tier] + "_rule")
        for shp in bad:
            assert ruled(None, None, 2, *shp, 4, *null, du.DUAL, None) == 1, (tier, shp)
        assert ruled(None, None, -1, *good, 4, *null, du.DUAL, None) == 1
        assert ruled(None, None, 0, *good, 4, *null, du.DUAL, None) == 0


# ----------------------------------------------------------------------------------------------
# the public calls
def _pack(refs, n, m, Rmax, ldb):
    tabs = np.zeros((len(refs), Rmax, ldb))
    dims = np.zeros((len(refs), 3), dtype=np.int32)
    for q, ref in enumerate(refs):
        tabs[q, :n + 1, :m + 1] = ref[0]
        dims[q] = (n, m, m)
    return tabs, dims


def _set_view(out, s):
    return {k: v[:, s] for k, v in out.items() if k != "base"}


def _same_base(a, b):
    assert list(a) == list(b)
    for key in a:
        assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), key


@pytest.mark.parametrize("tier,n,m,seeds,cap", CHAINS, ids=[c[0] for c in CHAINS])
def test_scenarios_arrays_with_the_dual_rule(tier, n, m, seeds, cap):
    """solve_batch_scenarios_arrays(warm_rule="dual"): S = 3 scenarios per LP, two rhs-only and
    one with its cost deltas; status, warm pivot count, x, duals, objective and labels of every
    scenario against the restatement's run on the restated table; with ranging on the workgroup
    tier.  `base` is the dict of the call without a warm rule, byte for byte."""
    from simplex_mi355x.batch import solve_batch_scenarios_arrays
    ranging = tier == "workgroup"
    bases = [_base(n, m, seed, cap) for seed in seeds]
    Rmax, ldb = n + 1, m + 1
    tabs, dims = _pack([b[0] for b in bases], n, m, Rmax, ldb)
    S = 3
    drhs = np.zeros((len(seeds), S, n))
    dcost = np.zeros((len(seeds), S, m))
    for q, seed in enumerate(seeds):
        for s in range(S):
            drhs[q, s], dc = scu.deltas(bases[q][0][0], n, m, seed, s, 0.2, 0.5)
            if s == 2:
                dcost[q, s] = dc
    out = solve_batch_scenarios_arrays(tabs, dims, drhs, dcost, cap, WARM_CAP, kernel=tier,
                                       ranging=ranging, warm_rule="dual")
    ref_out = solve_batch_scenarios_arrays(tabs, dims, drhs, dcost, cap, WARM_CAP, kernel=tier,
                                           ranging=ranging)
    _same_base(out["base"], ref_out["base"])
    assert set(out) == set(ref_out)
    dual_steps = 0
    for q, (ref, basis, nonbasis) in enumerate(bases):
        for s in range(S):
            St, func_s = scu.restate(ref[2], n, m, basis, nonbasis, ref[0][n, :m], drhs[q, s],
                                     dcost[q, s])
            Tw, wst, wdone, wlog, wdual = du.run(St, n, m, m, WARM_CAP, du.DUAL)
            dual_steps += wdual
            assert int(out["status"][q, s]) == wst, (tier, q, s)
            wb, wn = scu.warm_labels(basis, nonbasis, wlog, n, m)
            view = _set_view(out, s)
            su.same_arrays(view, q, n, m, scu.expected_solution(Tw, wb, wn, n, m, func_s, wdone),
                           (tier, q, s))
            if ranging:
                ru.same_arrays(view, q, n, m, ru.expected(Tw, wb, wn, n, m), (tier, q, s))
    assert dual_steps > 0


CUTS = CHAINS + [("wave", 62, 8, (0, 2), 256)]


@pytest.mark.parametrize("tier,n,m,seeds,cap", CUTS, ids=[c[0] for c in CHAINS] + ["crossing"])
def test_cuts_arrays_with_the_dual_rule(tier, n, m, seeds, cap):
    """solve_batch_cuts_arrays(warm_rule="dual", log=True): sets of one cut and of two per LP
    against the restatement's run on the restated extended table; the last case has 63 rows and
    leaves the wave tier for the workgroup tier with its first cut."""
    from simplex_mi355x.batch import solve_batch_cuts_arrays, warm_kernel
    bases = [_base(n, m, seed, cap) for seed in seeds]
    Rmax, ldb = n + 1, m + 1
    tabs, dims = _pack([b[0] for b in bases], n, m, Rmax, ldb)
    S, K = 2, 2
    if n == 62:
        assert warm_kernel("wave", Rmax + K, ldb) == "workgroup"
    cuts = np.zeros((len(seeds), S, K, ldb))
    ncuts = np.zeros((len(seeds), S), dtype=np.int32)
    sets = {}
    for q, seed in enumerate(seeds):
        _, _, x = cu.base_of_case(bases[q][0], n, m)
        for s in range(S):
            G = cu.cut_set(bases[q][0][0], n, m, seed, s, s + 1, 0.2, x)
            cuts[q, s, :s + 1] = G
            ncuts[q, s] = s + 1
            sets[q, s] = G
    out = solve_batch_cuts_arrays(tabs, dims, cuts, ncuts, cap, WARM_CAP, kernel=tier, log=True,
                                  warm_rule="dual")
    ref_out = solve_batch_cuts_arrays(tabs, dims, cuts, ncuts, cap, WARM_CAP, kernel=tier, log=True)
    _same_base(out["base"], ref_out["base"])
    dual_steps = 0
    for q, (ref, basis, nonbasis) in enumerate(bases):
        for s in range(S):
            k = s + 1
            E, basis_c = cu.restate(ref[2], n, m, basis, nonbasis, sets[q, s])
            Tw, wst, wdone, wlog, wdual = du.run(E, n + k, m, m, WARM_CAP, du.DUAL)
            assert wdual == wdone
            dual_steps += wdual
            assert int(out["status"][q, s]) == wst, (tier, q, s)
            assert np.array_equal(out["rc"][q, s, :wdone], wlog), (tier, q, s)
            wb, wn = cu.warm_labels(basis_c, nonbasis, wlog, n + k, m)
            su.same_arrays(_set_view(out, s), q, n + k, m,
                           cu.expected_solution(Tw, wb, wn, n + k, m, ref[0][n, :m], wdone),
                           (tier, q, s))
    assert dual_steps > 0


def _lists(T0, n, m):
    return T0[:n, :m + 1].tolist(), T0[n, :m].tolist()


def _bag():
    """A mixed bag: three wave LPs, one workgroup LP and one with int entries (routed "single":
    it goes through SimplexMethod on the device backend)."""
    bag = [(20, 3, 0, 64), (20, 3, 2, 64), (62, 8, 0, 256), (65, 65, 0, 1024)]
    probs = [_lists(case("uniform", n, m, seed, cap, m)[0], n, m) for n, m, seed, cap in bag]
    probs.append(([[-1, -1, 4], [-1, 0, 3], [0, -1, 2]], [-1, -2]))
    shapes = [(n, m) for n, m, _, _ in bag] + [(3, 2)]
    return probs, shapes


def _cold_table(cons, func):
    n, m = len(cons), len(func)
    T = np.zeros((n + 1, m + 1))
    T[:n] = cons
    T[n, :m] = func
    return T


def _expected_warm(cons, func, make, cap):
    """(status name, Expected) of one warm set of one problem: base run by the oracle, the warm
    table by `make(Tf, basis, nonbasis)` -> (table, rows, start labels, function), the warm run by
    the restatement under the dual rule."""
    from oracle import c_oracle
    n, m = len(cons), len(func)
    Tf, st, _, log = c_oracle.run(_cold_table(cons, func), n, m, m, cap)
    assert st == 1
    basis, nonbasis, _ = su.replay(log, n, m)
    W, rows, labels, function = make(Tf, basis, nonbasis)
    Tw, wst, wdone, wlog, _ = du.run(W, rows, m, m, WARM_CAP, du.DUAL)
    wb, wn = scu.warm_labels(labels[0], labels[1], wlog, rows, m)
    name = {0: "cap", 1: "optimum", 2: "error", 3: "error"}[wst]
    return name, scu.expected_solution(Tw, wb, wn, rows, m, function, wdone)


def _same_answer(sol, exp, what, ints):
    """By bit pattern; for the problem given in ints by value, since the reference's first pivot
    in int arithmetic gives some zeros the other sign (smx_int_first_fix) and the restatement
    starts from floats."""
    if not ints:
        return su.same_solution(sol, exp, what)
    assert np.array_equal(sol.basis, exp.basis) and np.array_equal(sol.nonbasis, exp.nonbasis), what
    assert np.array_equal(sol.x, exp.x) and np.array_equal(sol.duals, exp.duals), what
    assert sol.objective == exp.objective and sol.pivots == exp.pivots, what


def test_solve_batch_scenarios_and_cuts_over_a_mixed_bag():
    from simplex_mi355x.batch import route, solve_batch_cuts, solve_batch_scenarios
    probs, shapes = _bag()
    assert sorted(set(route(c, f) for c, f in probs)) == ["single", "wave", "workgroup"]
    scen, sets = [], []
    for k, ((cons, func), (n, m)) in enumerate(zip(probs, shapes)):
        T0 = _cold_table(cons, func)
        scen.append([(scu.deltas(T0, n, m, k, s, 0.2, 0.5)[0], None) for s in range(2)])
        from oracle import c_oracle
        Tf, _, _, log = c_oracle.run(T0, n, m, m, 1024)
        x = su.expected(Tf, log, n, m, T0[n]).x
        sets.append([cu.cut_set(T0, n, m, k, s, 1, 0.2, x).tolist() for s in range(2)])
    got_s = solve_batch_scenarios(probs, scen, 1024, WARM_CAP, cold_fallback=False,
                                  warm_rule="dual")
    got_c = solve_batch_cuts(probs, sets, 1024, WARM_CAP, cold_fallback=False, warm_rule="dual")
    for k, ((cons, func), (n, m)) in enumerate(zip(probs, shapes)):
        fl = [float(v) for v in func]
        for s in range(2):
            drhs = scen[k][s][0]
            name, exp = _expected_warm(
                cons, func, lambda Tf, b, nb: (scu.restate(Tf, n, m, b, nb, fl, drhs,
                                                           np.zeros(m))[0], n, (b, nb), fl), 1024)
            sc = got_s[k][1][s]
            assert (sc.status, sc.warm) == (name, True), (k, s, sc.status, name)
            _same_answer(sc.solution, exp, ("scenario", k, s), k == len(probs) - 1)
            G = sets[k][s]

            def ext(Tf, b, nb):
                E, bc = cu.restate(Tf, n, m, b, nb, G)
                return E, n + 1, (bc, nb), fl
            name, exp = _expected_warm(cons, func, ext, 1024)
            sc = got_c[k][1][s]
            assert (sc.status, sc.warm) == (name, True), (k, s, sc.status, name)
            _same_answer(sc.solution, exp, ("cuts", k, s), k == len(probs) - 1)


def test_the_case_the_reference_rule_does_not_finish():
    """Uniform 60 x 12, seed 5, scenario 1 at frac 0.2 with its cost deltas zeroed, through
    solve_batch_scenarios(cold_fallback=False) at a warm cap of 512: "cap" under the default
    rule, "optimum" after 2 pivots under the dual rule, with the cold run's objective."""
    from oracle import c_oracle
    from simplex_mi355x.batch import solve_batch_scenarios
    n, m, seed = 60, 12, 5
    T0 = case("uniform", n, m, seed, 256, m)[0]
    prob = _lists(T0, n, m)
    drhs, _ = scu.deltas(T0, n, m, seed, 1, 0.2, 0.5)
    kept = solve_batch_scenarios([prob], [[(drhs, None)]], 512, cold_fallback=False)
    assert kept[0][1][0].status == "cap" and kept[0][1][0].solution.pivots == 512
    dual = solve_batch_scenarios([prob], [[(drhs, None)]], 512, cold_fallback=False,
                                 warm_rule="dual")
    sc = dual[0][1][0]
    assert (sc.status, sc.warm, sc.solution.pivots) == ("optimum", True, 2)
    P = np.array(T0)
    P[:n, m] = np.where(drhs != 0, P[:n, m] + drhs, P[:n, m])
    Tc, cst, cdone, clog = c_oracle.run(P, n, m, m, 512)
    cold = su.expected(Tc, clog, n, m, T0[n]).objective
    assert (cst, cdone) == (1, 22)
    assert abs(sc.solution.objective - cold) <= 1e-9 * abs(cold)
    su.same_solution(dual[0][0], kept[0][0], "the base answer does not depend on the warm rule")


def test_solve_batch_arrays_with_the_dual_rule_on_cold_lps():
    """Cold LPs given with negative constants and non-negative costs (dual feasible from the
    start) through solve_batch_arrays(rule="dual") on all three tiers, and through solve_batch /
    solve_batch_solutions: the restatement's run, all of it in dual steps."""
    from simplex_mi355x.batch import solve_batch_arrays, solve_batch_solutions
    g = np.random.default_rng(11)
    for tier, n, m in (("wave", 12, 5), ("workgroup", 70, 20), ("global", 150, 150)):
        T = np.zeros((n + 1, m + 1))
        T[:n, :m] = g.normal(size=(n, m))
        T[:n, m] = g.normal(size=n)                          # some negative, some not
        T[n, :m] = np.abs(g.normal(size=m))
        exp = du.run(T, n, m, m, 40, du.DUAL)
        assert exp[2] > 0 and exp[4] == exp[2], (tier, exp[1:3], exp[4])
        tabs, dims = T[None].copy(), np.array([[n, m, m]], dtype=np.int32)
        out = solve_batch_arrays(tabs, dims, 40, kernel=tier, solution=True, rule="dual")
        assert int(out["status"][0]) == exp[1] and int(out["npivots"][0]) == exp[2]
        assert np.array_equal(out["rc"][0, :exp[2]], exp[3])
        assert su.same_floats(out["final"][0], exp[0])
        su.same_arrays(out, 0, n, m, su.expected(exp[0], exp[3], n, m, T[n]), tier)
        plain = solve_batch_arrays(tabs, dims, 40, kernel=tier, solution=True)
        assert list(plain) == list(out)
        assert all(plain[k].shape == out[k].shape and plain[k].dtype == out[k].dtype for k in out)
        if tier == "wave":
            sols, sts = solve_batch_solutions([_lists(T, n, m)], 40, rule="dual")
            su.same_solution(sols[0], su.expected(exp[0], exp[3], n, m, T[n]), "solutions")
            assert sts == [{0: "cap", 1: "optimum", 2: "error", 3: "error"}[exp[1]]]


def test_simplex_method_with_the_dual_rule_on_the_device_backend():
    """what_if(drhs).solve(rule="dual") and add_constraints(rows).solve(rule="dual") on a device
    tableau: the table comes down, the host twin runs, the result goes back up -- log, status,
    labels, table, solution() and ranging() against the restatement."""
    import simplex
    n, m, seed, cap = 40, 7, 1, 64
    ref, basis, nonbasis = _base(n, m, seed, cap)
    cons, func = _lists(ref[0], n, m)
    sm = simplex.SimplexMethod(cons, func, device="cuda:0")
    assert sm.backend == "hip"
    sm.solve(record_history=False, max_pivots=cap)
    assert sm.pivots == ref[4]
    drhs, _ = scu.deltas(ref[0], n, m, seed, 0, 0.5, 0.5)
    _, _, x = cu.base_of_case(ref, n, m)
    G = cu.cut_set(ref[0], n, m, seed, 0, 2, 0.2, x)
    S, func_s = scu.restate(ref[2], n, m, basis, nonbasis, func, drhs, np.zeros(m))
    E, basis_c = cu.restate(ref[2], n, m, basis, nonbasis, G)
    total = 0
    for warm, W, rows, labels, function in (
            (sm.what_if(drhs), S, n, (basis, nonbasis), func_s),
            (sm.add_constraints(G.tolist()), E, n + 2, (basis_c, nonbasis), np.asarray(func))):
        assert warm.backend == "hip"
        Tw, wst, wdone, wlog, wdual = du.run(W, rows, m, m, cap, du.DUAL)
        total += wdual
        warm.solve(record_history=False, max_pivots=cap, rule="dual")
        assert warm.pivot_log == [tuple(map(int, rc)) for rc in wlog]
        assert warm.status == {0: "cap", 1: "optimum", 2: "error", 3: "error"}[wst]
        wb, wn = scu.warm_labels(labels[0], labels[1], wlog, rows, m)
        assert su.label_codes(warm.column[:-1], m) == wb.tolist()
        assert su.label_codes(warm.row[:-1], m) == wn.tolist()
        scu.same_table(warm._dev.download()[:rows + 1, :m + 1], Tw, "table")
        su.same_solution(warm.solution(), scu.expected_solution(Tw, wb, wn, rows, m, function,
                                                                wdone), "solution")
        ru.same_ranges(warm.ranging(), ru.expected(Tw, wb, wn, rows, m), "ranging")
        # the reference rule carries on from the uploaded table
        warm.solve(record_history=False, max_pivots=4)
        assert warm.status in ("optimum", "cap", "error")
    assert total > 0
    with pytest.raises(ValueError, match="rule must be"):
        sm.solve(rule="primal")
