"""Batched small LPs: many ``get_solution`` runs in one kernel launch.

The reference UI solves 2-variable LPs with a handful of constraints (main.py:309-313); on the
GPU one such solve is pure launch latency.  ``solve_batch`` packs up to millions of small problems
(n <= 63 constraints, m + 1 <= 64 columns) and runs each one's whole pivot loop inside one
wavefront of ``k_batch`` (csrc/smx_batch.hpp).  Per problem the result is exactly what
``SimplexMethod(constraints, function).get_solution()`` returns (simplex.py:179-199): the list of
``Info`` snapshots (labels, table, i/j, x1/x2/optimum) with the trailing ``Error`` on the two
``ValueError`` outcomes.  Problems past that envelope whose table still fits one CU's LDS (to
about 140 x 140, 300 x 40 or 40 x 300) run one workgroup each in ``k_batch_wg``
(csrc/smx_batch_wg.hpp), grouped into launches of similar size (``wg_launches``).  Problems
past the LDS edge, up to a 724 x 724 table, run one workgroup each with the table in global memory
(``k_batch_gm``, csrc/smx_batch_gm.hpp; launches from ``gm_launches``) once a call holds
``GM_MIN_BATCH`` of them.  Problems outside all three envelopes (bigger, ragged, int entries, or
with a ``len(function)`` the reference would index out of range) go through ``SimplexMethod``
one by one -- still on the device.

``solve_batch_solutions`` (and ``solve_batch_arrays(solution=True)``) answer with every LP's whole
solution -- all of x, the duals, the objective, the labels -- formed on the device by
``k_batch_solution`` (csrc/smx_solution.hpp) from the final tables and pivot logs; with
``tables=False`` only that comes back, not the tables.  ``solve_batch_ranges`` (and
``solve_batch_arrays(solution=True, ranging=True)``) add how far each constraint's constant and
each cost can move before that final basis changes, formed on the device by ``k_batch_ranging``
(csrc/smx_ranging.hpp) from the final tables and the labels.

``solve_batch_scenarios`` (and ``solve_batch_scenarios_arrays``) answer "the constants and costs
move: what is the optimum now?" without solving the perturbed problems from scratch:
``k_batch_scenario`` (csrc/smx_scenario.hpp) re-expresses every scenario under its LP's final
basis on the device, and the same solve kernel carries on from that table -- a handful of pivots
where a cold solve takes hundreds.  Under the default selection rule such a warm run need not
terminate: every scenario reports its status, and the object-level call falls back to
a cold solve.  ``warm_rule="dual"`` runs the warm solve under the dual-simplex rule of
include/smx.h (SMX_RULE_DUAL): from a dual-feasible table -- constants moved, costs
not, after a base run that ended at an optimum -- it terminates, up to degenerate cycling; status
and cap remain.

``solve_batch_cuts`` (and ``solve_batch_cuts_arrays``) answer "I have new constraints: what is the
optimum now?" in the same way: ``k_batch_cuts`` (csrc/smx_cuts.hpp) writes every cut, given in the
original variables, as one more row under its LP's final basis, and the solve kernel that takes
the enlarged block carries on from there.  The same caveat holds under the default
rule and the same cold fallback answers it; an extended table keeps its base run's f-row, so after
an optimum ``warm_rule="dual"`` applies to every cut set.

``solve_batch_columns`` (and ``solve_batch_columns_arrays``) answer "I have new variables: what is
the optimum now?" -- column generation: ``k_batch_cols`` (csrc/smx_cols.hpp) writes every new
variable, given by its coefficients in the original constraints and its cost, as one more column
under its LP's final basis, and the solve kernel that takes the widened block carries on from
there.  A new variable leaves the constants alone, so after an optimum the widened
table is primal feasible and the default rule is an ordinary primal simplex from it.

``solve_batch_integer`` (and ``solve_batch_integer_arrays``) answer "these variables must be whole
numbers" by branch and bound, level by level, the tables never leaving the device:
``k_batch_branch_pick`` (csrc/smx_branch.hpp) finds the variable to branch on in every solved
node, the host keeps incumbents and lists the nodes to expand (``branch.Tree``, shared with
``SimplexMethod.solve_integer``), ``k_batch_branch`` writes both children of each -- a bound row
under the parent's final basis -- and one warm solve under the dual rule re-solves them all; a
child is a node, so the chain goes on.

The host side of all this is stated once.  Array level: ``_launch_arrays`` and
``_launch_tier`` check a launch, ``_device_solve`` / ``_device_solution`` / ``_device_ranging``
enqueue one kernel each on fresh outputs, ``_enqueue_base`` and ``_base_arrays`` are
``solve_batch_arrays`` (and so the ``base`` of the warm calls), and ``_warm_chain`` is everything
the warm calls share: a warm feature hands it the callable that enqueues its table-making
kernel.  Object level: ``_drive`` routes, falls back and launches for all six ``solve_batch*``
calls, ``_solution_at`` builds a ``Solution``, ``_status_name`` names a status, ``_warm_answers``
and ``_cold_tail`` serve scenarios, cuts and columns alike.  Cuts and columns, which differ in the
axis that grows, share both levels: ``_grown_arrays`` (with ``_enqueue_cuts`` / ``_enqueue_cols``
for the one library call each has of its own) and ``_solve_batch_grown``.
"""
from __future__ import annotations

import gc

import numpy as np
import torch

from . import _lib
from .engine import MESSAGES, Error, Info, Ranging, Scenario, SimplexMethod, Solution

# The wave kernel's envelope (k_batch): past it a launch goes to the workgroup kernel
# (k_batch_wg), whose own envelope -- what one CU's LDS holds -- only the library states
# (smx_batch_wg_lds_bytes).
MAX_ROWS = 64      # one wavefront: rows 0..n (f-row = lane n)
MAX_COLS = 64      # register-resident row of at most 64 doubles

KERNELS = ("auto", "wave", "workgroup", "global")
ENVELOPE_ERROR = "a problem is outside the batch kernel's envelope"
# history=True: one workgroup launch's snapshot buffer ([B][max_pivots][Rmax][ldb] doubles; a
# 128 x 128 LP with max_pivots=256 is 32 MiB) stays under this many bytes -- a bucket is split
# into as many launches as that takes (a single LP is never split).
SNAP_BUDGET = 1 << 30
# One global-memory launch's tables ([B][Rmax][ldb] doubles, in and out each) stay under this.
GM_TABLE_BUDGET = 1 << 30
# solve_batch(kernel="auto") takes the global-memory kernel only when a call holds at least this
# many problems routed "global"; fewer go through SimplexMethod one by one.  The smallest measured
# batch at which the kernel path's wall time per LP is at or under the one-by-one path's at every
# measured shape inside the envelope (profiles/batch_gm.json): a single LP already is,
# by 10 to 23 % of that path's best time at tables of 142^2, 256^2, 512^2 and 724^2.
GM_MIN_BATCH = 1


def _envelope(query: str, Rmax: int, ldb: int, outside):
    """What the library's envelope query ``query`` says of Rmax x ldb blocks; ``outside`` where
    either is no int32, the C argument type.  The library is the one source of every rule."""
    if not (0 <= Rmax < 1 << 31 and 0 <= ldb < 1 << 31):
        return outside
    return getattr(_lib.load(), query)(int(Rmax), int(ldb))


def wg_lds_bytes(Rmax: int, ldb: int) -> int:
    """Dynamic LDS one workgroup of k_batch_wg needs for a launch of Rmax x ldb blocks, -1 when
    the shape is outside that kernel's envelope."""
    return int(_envelope("smx_batch_wg_lds_bytes", Rmax, ldb, -1))


def gm_fits(Rmax: int, ldb: int) -> bool:
    """Whether a launch of Rmax x ldb blocks is inside k_batch_gm's envelope."""
    return bool(_envelope("smx_batch_gm_fits", Rmax, ldb, False))


def solution_lds_bytes(Rmax: int, ldb: int) -> int:
    """Dynamic LDS one block of k_batch_solution needs for a launch of Rmax x ldb blocks, -1 when
    the shape is outside that kernel's envelope."""
    return int(_envelope("smx_batch_solution_lds_bytes", Rmax, ldb, -1))


def ranging_fits(Rmax: int, ldb: int) -> bool:
    """Whether a launch of Rmax x ldb blocks is inside k_batch_ranging's envelope."""
    return bool(_envelope("smx_batch_ranging_fits", Rmax, ldb, False))


def scenario_fits(Rmax: int, ldb: int) -> bool:
    """Whether a launch of Rmax x ldb blocks is inside k_batch_scenario's envelope."""
    return bool(_envelope("smx_batch_scenario_fits", Rmax, ldb, False))


def cuts_fits(Rmax_out: int, ldb: int) -> bool:
    """Whether output blocks of Rmax_out x ldb are inside k_batch_cuts's envelope."""
    return bool(_envelope("smx_batch_cuts_fits", Rmax_out, ldb, False))


def cols_fits(Rmax: int, ldb_out: int) -> bool:
    """Whether output blocks of Rmax x ldb_out are inside k_batch_cols's envelope."""
    return bool(_envelope("smx_batch_cols_fits", Rmax, ldb_out, False))


def _shape(cons, func):
    """(n, m, flen) of a problem the batch kernels can take if it holds floats only (rectangular,
    a ``len(function)`` the reference does not index out of range), else None."""
    if not cons:
        return None
    m = len(cons[0]) - 1
    n = len(cons)
    if m < 1 or any(len(r) != m + 1 for r in cons):
        return None
    flen = len(func)
    if flen not in (m, m + 1) or flen < 2:
        return None
    return n, m, flen


def _eligible(cons, func) -> bool:
    if not cons:
        return False
    if len(cons) + 1 > MAX_ROWS or len(cons[0]) > MAX_COLS:
        return False
    # int entries: the reference's first pivot runs in int arithmetic, whose zero signs differ
    # from fp64's (engine._int_entries); SimplexMethod applies that fix, the batch kernels do not
    return _shape(cons, func) is not None and not _has_ints(cons, func)


def route(constraints, function) -> str:
    """Where ``solve_batch`` sends a problem: ``"wave"`` (k_batch, one wavefront per LP),
    ``"workgroup"`` (k_batch_wg, one workgroup per LP, tableau in LDS), ``"global"`` (k_batch_gm,
    one workgroup per LP, tableau in global memory: past one CU's LDS and inside
    ``smx_batch_gm_fits``) or ``"single"`` (``SimplexMethod``, one by one: int entries, ragged
    rows, tables past the global-memory kernel's envelope and the reference's IndexError cases).
    Host only."""
    if _eligible(constraints, function):
        return "wave"
    shp = _shape(constraints, function)
    if shp is None:
        return "single"
    if wg_lds_bytes(shp[0] + 1, shp[1] + 1) >= 0:
        return "single" if _has_ints(constraints, function) else "workgroup"
    if gm_fits(shp[0] + 1, shp[1] + 1) and not _has_ints(constraints, function):
        return "global"
    return "single"


def choose_kernel(Rmax: int, ldb: int, kernel: str = "auto") -> str:
    """The kernel a launch of Rmax x ldb blocks runs on: ``"auto"`` takes the wave kernel inside
    its envelope and the workgroup kernel past it; ``"wave"`` / ``"workgroup"`` / ``"global"``
    force one.  ``"auto"`` never answers ``"global"``: past the LDS edge it refuses, and the
    global-memory kernel is reached only by name.
    Raises ValueError when the shape fits none of the kernels allowed."""
    _kernel_name(kernel)
    if kernel == "global":
        if gm_fits(Rmax, ldb):
            return "global"
        raise ValueError(ENVELOPE_ERROR)
    if kernel != "workgroup" and Rmax <= MAX_ROWS and ldb <= MAX_COLS:
        return "wave"
    if kernel != "wave" and wg_lds_bytes(Rmax, ldb) >= 0:
        return "workgroup"
    raise ValueError(ENVELOPE_ERROR)


def _has_ints(cons, func) -> bool:
    """Any entry an int (Python int / bool, numpy integer scalar or integer row), as
    engine._int_entries counts them."""
    for row in (*cons, func):
        if isinstance(row, np.ndarray):
            if row.dtype.kind in "iub":
                return True
            continue
        # by the set of element types: a 100 x 100 LP is 10 000 entries and almost always all float
        for t in set(map(type, row)):
            if t is not float and issubclass(t, (int, np.integer)):
                return True
    return False


def _labels(n, m):
    row = ['x' + str(k) for k in range(1, m + 1)] + ['-b']
    col = ['y' + str(k) for k in range(1, n + 1)] + ['f']
    return row, col


def _kernel_name(kernel):
    if kernel not in KERNELS:
        raise ValueError(f"kernel must be one of {KERNELS}, not {kernel!r}")


def _need_device():
    if not torch.cuda.is_available():
        raise RuntimeError("simplex_mi355x needs an MI355X (HIP device); there is no CPU path")


def _launch_arrays(tabs, dims):
    """The first half of the launch check every array-level call makes: ``tabs`` and ``dims`` as
    contiguous float64 / int32 arrays and (B, Rmax, ldb).  Refuses a ``dims`` of another shape."""
    tabs = np.ascontiguousarray(tabs, dtype=np.float64)
    dims = np.ascontiguousarray(dims, dtype=np.int32)
    B, Rmax, ldb = tabs.shape
    if dims.shape != (B, 3):
        raise ValueError("dims must be int32 [B][3]")
    return tabs, dims, (B, Rmax, ldb)


def _launch_tier(dims, shape, kernel):
    """The second half (the calls differ in what they refuse between the two): the tier
    ``kernel`` puts a launch of this shape on (``choose_kernel``).  Refuses a problem of ``dims``
    that lies outside the launch's Rmax x ldb blocks."""
    B, Rmax, ldb = shape
    which = choose_kernel(Rmax, ldb, kernel) if B else "wave"
    if B and ((dims[:, 0] + 1 > Rmax).any() or (dims[:, 1] + 1 > ldb).any() or
              (dims[:, 1] < 1).any() or (dims[:, 0] < 1).any()):
        raise ValueError(ENVELOPE_ERROR)
    return which


# the library's solve entry point of every tier
_SOLVERS = {"wave": "smx_batch_solve_rule", "workgroup": "smx_batch_solve_wg_rule",
            "global": "smx_batch_solve_gm_rule"}


def _device_solve(L, stream, tier, d_tabs, d_dims, cap, history=False, rule=_lib.RULE_REFERENCE):
    """Enqueue the solve kernel of ``tier`` on fresh outputs, capped at ``cap`` pivots; returns
    the device tensors (final, rc, xv, status, npivots, snaps), ``snaps`` None without
    ``history``.  ``rule`` is an SMX_RULE_* code for the tier's ``_rule`` entry, which under the
    reference rule is the entry point without a rule."""
    count, rows, ldb = d_tabs.shape
    dev = d_tabs.device
    d_out = torch.empty_like(d_tabs)
    d_rc = torch.zeros((count, max(cap, 1), 2), dtype=torch.int32, device=dev)
    d_xv = torch.zeros((count, max(cap, 1), 2), dtype=torch.float64, device=dev)
    d_snaps = (torch.empty((count, max(cap, 1), rows, ldb), dtype=torch.float64, device=dev)
               if history else None)
    d_st = torch.zeros(count, dtype=torch.int32, device=dev)
    d_np = torch.zeros(count, dtype=torch.int32, device=dev)
    what = _SOLVERS[tier]
    args = (d_tabs.data_ptr(), d_dims.data_ptr(), count, rows, ldb, cap, d_out.data_ptr(),
            d_rc.data_ptr(), d_xv.data_ptr(), d_snaps.data_ptr() if history else None,
            d_st.data_ptr(), d_np.data_ptr())
    _lib.check(getattr(L, what)(*args, int(rule), stream.cuda_stream), what)
    return d_out, d_rc, d_xv, d_st, d_np, d_snaps


def _device_solution(L, stream, d_final, d_dims, P, d_rc, d_np, d_func, start=None):
    """Enqueue smx_batch_solution (``start`` = (basis0, nonbasis0, group): smx_batch_solution_from)
    on fresh outputs; returns the device tensors (x, duals, objective, basis, nonbasis)."""
    B, Rmax, ldb = d_final.shape
    dev = d_final.device
    d_x = torch.empty((B, ldb), dtype=torch.float64, device=dev)
    d_du = torch.empty((B, Rmax), dtype=torch.float64, device=dev)
    d_obj = torch.empty(B, dtype=torch.float64, device=dev)
    d_ba = torch.empty((B, Rmax), dtype=torch.int32, device=dev)
    d_nb = torch.empty((B, ldb), dtype=torch.int32, device=dev)
    head = (d_final.data_ptr(), d_dims.data_ptr(), B, Rmax, ldb, P, d_rc.data_ptr(),
            d_np.data_ptr(), d_func.data_ptr())
    tail = (d_x.data_ptr(), d_du.data_ptr(), d_obj.data_ptr(), d_ba.data_ptr(), d_nb.data_ptr(),
            stream.cuda_stream)
    if start is None:
        _lib.check(L.smx_batch_solution(*head, *tail), "smx_batch_solution")
    else:
        _lib.check(L.smx_batch_solution_from(*head, start[0].data_ptr(), start[1].data_ptr(),
                                             int(start[2]), *tail), "smx_batch_solution_from")
    return d_x, d_du, d_obj, d_ba, d_nb


def _device_ranging(L, stream, d_final, d_dims, d_ba, d_nb):
    """Enqueue smx_batch_ranging on fresh outputs; returns (rhs_lo, rhs_hi, cost_lo, cost_hi)."""
    B, Rmax, ldb = d_final.shape
    dev = d_final.device
    d_rl, d_rh = (torch.empty((B, Rmax), dtype=torch.float64, device=dev) for _ in "lh")
    d_cl, d_ch = (torch.empty((B, ldb), dtype=torch.float64, device=dev) for _ in "lh")
    _lib.check(L.smx_batch_ranging(
        d_final.data_ptr(), d_dims.data_ptr(), B, Rmax, ldb, d_ba.data_ptr(), d_nb.data_ptr(),
        d_rl.data_ptr(), d_rh.data_ptr(), d_cl.data_ptr(), d_ch.data_ptr(), stream.cuda_stream),
        "smx_batch_ranging")
    return d_rl, d_rh, d_cl, d_ch


def _cut(d, lead):
    """[count][width] on the device -> ``lead`` + [width - 1] on the host: the kernels write rows
    of Rmax / ldb entries whose last stands for the f-row / the '-b' column and holds nothing."""
    return d[:, :d.shape[1] - 1].contiguous().cpu().numpy().reshape(*lead, d.shape[1] - 1)


def _solution_arrays(sol, lead):
    """The host arrays of a ``_device_solution`` result, reshaped to ``lead`` + [...]."""
    d_x, d_du, d_obj, d_ba, d_nb = sol
    return {"x": _cut(d_x, lead), "duals": _cut(d_du, lead),
            "objective": d_obj.cpu().numpy().reshape(*lead),
            "basis": _cut(d_ba, lead), "nonbasis": _cut(d_nb, lead)}


def _ranging_arrays(rng, lead):
    return dict(zip(("rhs_lo", "rhs_hi", "cost_lo", "cost_hi"), (_cut(d, lead) for d in rng)))


def _enqueue_base(L, stream, tier, d_tabs, d_dims, P, history=False, solution=True,
                  ranging=False, rule=_lib.RULE_REFERENCE):
    """Enqueue a launch's solve on ``tier`` and, as asked, its solution and its ranges; returns
    (the ``_device_solve`` tensors, the original objective rows, the ``_device_solution`` tensors,
    the ``_device_ranging`` tensors), None for what was not asked.  Nothing comes back yet:
    ``_base_arrays`` does that."""
    run = _device_solve(L, stream, tier, d_tabs, d_dims, P, history, rule)
    d_func = sol = rng = None
    if solution:
        # the original objective rows (row n_k of problem k), gathered on the device
        d_func = d_tabs[torch.arange(len(d_tabs), device=d_tabs.device),
                        d_dims[:, 0].long()].contiguous()
        sol = _device_solution(L, stream, run[0], d_dims, P, run[1], run[4], d_func)
    if ranging:
        rng = _device_ranging(L, stream, run[0], d_dims, sol[3], sol[4])
    return run, d_func, sol, rng


def _base_arrays(run, sol, rng, tables=False):
    """The result dict of ``solve_batch_arrays`` from what ``_enqueue_base`` enqueued."""
    d_out, d_rc, d_xv, d_st, d_np, d_snaps = run
    res = {"final": d_out.cpu().numpy()} if tables else {}
    res.update({"rc": d_rc.cpu().numpy(), "xv": d_xv.cpu().numpy(),
                "status": d_st.cpu().numpy(), "npivots": d_np.cpu().numpy()})
    if sol is not None:
        res.update(_solution_arrays(sol, (len(d_out),)))
    if rng is not None:
        res.update(_ranging_arrays(rng, (len(d_out),)))
    if d_snaps is not None:
        steps = torch.arange(d_snaps.shape[1], device=d_np.device)[None, :] < d_np[:, None]
        res["snaps"] = d_snaps[steps].cpu().numpy()
        res["snap_off"] = np.concatenate([[0], np.cumsum(res["npivots"], dtype=np.int64)])
    return res


def solve_batch_arrays(tabs: np.ndarray, dims: np.ndarray, max_pivots: int = 256,
                       history: bool = False, device=None, kernel: str = "auto",
                       solution: bool = False, tables: bool = True,
                       ranging: bool = False, rule: str = "reference") -> dict:
    """Array-level batch solve (no Python objects per problem).

    ``tabs``: float64 [B][Rmax][ldb], problem k in rows 0..n_k (f-row = row n_k), columns
    0..m_k; ``dims``: int32 [B][3] = (n, m, len(function)) with every problem inside the kernel's
    envelope (see ``route``).  ``kernel``: ``"auto"`` runs the launch on the wave kernel when
    Rmax <= 64 and ldb <= 64 and on the workgroup kernel past that, up to what one CU's LDS
    holds; ``"wave"`` / ``"workgroup"`` force one (``choose_kernel``).  ``"global"`` runs the
    launch on the global-memory kernel at any shape inside ``smx_batch_gm_fits`` (to 724 x 724);
    ``"auto"`` still refuses a shape past the LDS edge, so this API reaches that tier only by
    name.  A shape that fits none raises ValueError.
    Returns numpy arrays: ``final`` (same layout as tabs),
    ``status`` (SMX_* codes; SMX_PIVOT = max_pivots reached), ``npivots``, ``rc`` [B][P][2],
    ``xv`` [B][P][2] (x1, x2 after each pivot) and, with ``history``, ``snaps``
    [sum(npivots)][Rmax][ldb] -- problem k's tables after each of its pivots are
    ``snaps[snap_off[k]:snap_off[k + 1]]`` (compacted on the device before the copy back).

    ``solution=True`` adds what ``k_batch_solution`` makes of every final table and pivot log on
    the device (labels as int32 codes: k in 0..m-1 is 'x{k+1}', m + i is 'y{i+1}'): ``x``
    [B][ldb - 1] (+0.0 past m_k), ``duals`` [B][Rmax - 1] (+0.0 past n_k), ``objective`` [B],
    ``basis`` [B][Rmax - 1] and ``nonbasis`` [B][ldb - 1] (-1 past n_k / m_k); see ``Solution``.
    ``tables=False`` (only with ``solution=True`` and without ``history``) leaves the final tables
    on the device: the result has no ``final``.

    ``ranging=True`` (only with ``solution=True``, whose labels it consumes; with or without
    ``tables``) adds what ``k_batch_ranging`` makes of every final table and those labels on the
    device: ``rhs_lo``, ``rhs_hi`` [B][Rmax - 1] and ``cost_lo``, ``cost_hi`` [B][ldb - 1] (+0.0
    past n_k / m_k); see ``Ranging``.

    ``rule``: ``"reference"`` (the default: the reference's pick_element) or ``"dual"``
    (SMX_RULE_DUAL of include/smx.h: a step from a table with a negative constant and no negative
    cost is a dual-simplex step, every other step the reference's).  Any other value raises
    ValueError before the device is asked for.  The result's keys, shapes and dtypes do not depend
    on it.
    """
    code = _lib.rule_code(rule)
    if not tables and not solution:
        raise ValueError("tables=False needs solution=True: nothing else would report the answer")
    if ranging and not solution:
        raise ValueError("ranging=True needs solution=True: the ranges are read off its labels")
    if not tables and history:
        raise ValueError("history=True needs the tables: tables=False cannot go with it")
    _need_device()
    tabs, dims, shape = _launch_arrays(tabs, dims)
    which = _launch_tier(dims, shape, kernel)
    if solution and solution_lds_bytes(*shape[1:]) < 0:
        raise ValueError(ENVELOPE_ERROR)
    if ranging and not ranging_fits(*shape[1:]):
        raise ValueError(ENVELOPE_ERROR)
    dev = torch.device(device if device is not None else "cuda")
    with torch.cuda.device(dev):
        d_tabs = torch.from_numpy(tabs).to(dev)
        d_dims = torch.from_numpy(dims).to(dev)
        run, _, sol, rng = _enqueue_base(_lib.load(), torch.cuda.current_stream(dev), which,
                                         d_tabs, d_dims, int(max_pivots), history, solution,
                                         ranging, code)
        return _base_arrays(run, sol, rng, tables)


def pack(problems):
    """(constraints, function) lists -> (tabs, dims) for solve_batch_arrays."""
    B = len(problems)
    dims = np.zeros((B, 3), dtype=np.int32)
    for q, (c, f) in enumerate(problems):
        dims[q] = (len(c), len(c[0]) - 1, len(f))
    Rmax = int(dims[:, 0].max()) + 1
    ldb = int(dims[:, 1].max()) + 1
    tabs = np.zeros((B, Rmax, ldb), dtype=np.float64)
    for q, (c, f) in enumerate(problems):
        n, m = len(c), len(c[0]) - 1
        tabs[q, :n, :m + 1] = c
        tabs[q, n, :min(len(f), m + 1)] = f[:m + 1]
    return tabs, dims


def _split_launches(shapes, max_pivots, history, cost, table_budget=None):
    """The launch splitter of ``wg_launches`` and ``gm_launches``.  ``cost(R, C)`` is what a
    launch of R x C blocks costs per problem, negative where the kernel does not take the shape.
    Sort the problems by their own cost; a launch takes the next problem while its padded
    rows x columns still fit the kernel and cost at most twice its smallest (first) member.  A
    launch also ends where its tables (B * Rmax * ldb * 8 bytes) would pass ``table_budget`` or,
    with ``history``, where its snapshot buffer would pass ``SNAP_BUDGET``; a single LP is never
    split."""
    order = sorted(range(len(shapes)), key=lambda q: cost(shapes[q][0] + 1, shapes[q][1] + 1))
    launches = []
    cur, R, C, floor = [], 0, 0, 0
    for q in order:
        n, m = shapes[q]
        R2, C2 = max(R, n + 1), max(C, m + 1)
        padded = cost(R2, C2)
        tab = (len(cur) + 1) * R2 * C2 * 8
        snap = tab * max(int(max_pivots), 1) if history else 0
        if cur and (not 0 <= padded <= 2 * floor or snap > SNAP_BUDGET
                    or (table_budget is not None and tab > table_budget)):
            launches.append(cur)
            cur, R2, C2 = [], n + 1, m + 1
            padded = cost(R2, C2)
        if not cur:
            floor = padded
        cur.append(q)
        R, C = R2, C2
    if cur:
        launches.append(cur)
    return launches


def wg_launches(shapes, max_pivots: int, history: bool):
    """Split workgroup-kernel problems into launches; ``shapes[q]`` = (n, m) of problem q, the
    result is a list of index lists.

    A launch pads every member to its largest rows x columns, and that padded block is what each
    workgroup holds in LDS, so one big member would cost all the others occupancy.  The rule is
    ``_split_launches`` with the LDS footprint (``wg_lds_bytes``) as the cost."""
    return _split_launches(shapes, max_pivots, history, wg_lds_bytes)


def gm_launches(shapes, max_pivots: int, history: bool):
    """Split global-memory-kernel problems into launches; ``shapes[q]`` = (n, m) of problem q,
    the result is a list of index lists.

    ``_split_launches`` with the element count (n + 1) * (m + 1) inside ``gm_fits`` as the cost
    and ``GM_TABLE_BUDGET`` on a launch's tables."""
    return _split_launches(shapes, max_pivots, history,
                           lambda R, C: R * C if gm_fits(R, C) else -1, GM_TABLE_BUDGET)


def _routes(problems, kernel):
    """``route`` of every problem, then what ``kernel`` makes of it (``solve_batch``)."""
    routes = [route(c, f) for c, f in problems]
    if kernel == "wave" and "workgroup" in routes:
        raise ValueError(ENVELOPE_ERROR)
    if kernel == "workgroup":
        routes = ["workgroup" if r == "wave" else r for r in routes]
    if kernel == "global":
        routes = [r if r == "single" else "global" for r in routes]
    elif kernel != "auto" or routes.count("global") < GM_MIN_BATCH:
        routes = ["single" if r == "global" else r for r in routes]
    return routes


def _launches(problems, routes, max_pivots, history):
    """[(kernel, problem indices)]: the wave problems in one launch, the workgroup and global
    problems in the launches of ``wg_launches`` / ``gm_launches``."""
    launches = []
    idx = [k for k, r in enumerate(routes) if r == "wave"]
    if idx:
        launches.append(("wave", idx))
    for which, split in (("workgroup", wg_launches), ("global", gm_launches)):
        idx = [k for k, r in enumerate(routes) if r == which]
        if idx:
            shapes = [(len(problems[k][0]), len(problems[k][0][0]) - 1) for k in idx]
            launches += [(which, [idx[q] for q in part])
                         for part in split(shapes, max_pivots, history)]
    return launches


def _status_name(status, np_, P):
    if status == _lib.OPTIMUM:
        return "optimum"
    if status in MESSAGES:
        return "error"
    if status == _lib.PIVOT and np_ >= P:
        return "cap"
    raise RuntimeError(f"unexpected batch status {status}")


def _solution_at(arrays, index, n, m):
    """The ``Solution`` of the LP at ``index`` (q, or (q, s) of a warm result) of the arrays of
    ``solve_batch_arrays(solution=True)`` and its kin; n and m are that LP's own."""
    return Solution(arrays["x"][index][:m].copy(), arrays["duals"][index][:n].copy(),
                    float(arrays["objective"][index]), arrays["basis"][index][:n].copy(),
                    arrays["nonbasis"][index][:m].copy(), int(arrays["npivots"][index]))


def _fallback(cons, func, max_pivots, history, rule="reference"):
    try:
        sm = SimplexMethod(cons, func)
        if history:
            return sm.get_solution(max_pivots=max_pivots, rule=rule), sm.status
        return sm.solve(record_history=False, max_pivots=max_pivots, rule=rule), sm.status
    except IndexError as exc:        # where the reference itself raises (simplex.py:49, 95, 159)
        return exc, "exception"


def _fallback_answer(cons, func, max_pivots, answer, rule="reference"):
    """One problem through ``SimplexMethod``; ``answer`` is the method that reads the result off
    the solved object (``SimplexMethod.solution`` / ``.ranging``)."""
    try:
        sm = SimplexMethod(cons, func)
        sm.solve(record_history=False, max_pivots=max_pivots, rule=rule)
        return answer(sm), sm.status
    except IndexError as exc:        # where the reference itself raises (simplex.py:49, 95, 159)
        return exc, "exception"


def _drive(problems, kernel, max_pivots, history, single, launch):
    """The scaffold of every object-level call: refuse a ``kernel`` that is no name and a machine
    without a device, route the problems (``_routes``), have ``single(k, constraints, function)``
    answer those routed ``"single"`` and ``launch(tier, idx, tabs, dims)`` every launch of the
    rest (``_launches``, ``pack``; problem ``idx[q]`` is member q).  Both store their answers
    themselves, by problem index."""
    _kernel_name(kernel)
    _need_device()
    routes = _routes(problems, kernel)
    for k, (c, f) in enumerate(problems):
        if routes[k] == "single":
            single(k, c, f)
    for which, idx in _launches(problems, routes, max_pivots, history):
        tabs, dims = pack([problems[k] for k in idx])
        launch(which, idx, tabs, dims)


def solve_batch(problems, max_pivots: int = 256, history: bool = True, device=None,
                kernel: str = "auto", rule: str = "reference"):
    """Solve every ``(constraints, function)``; returns ``(results, statuses)``.

    ``results[k]`` is the ``get_solution()`` list of problem k (``history=False``: only the
    initial and the final ``Info``, like ``SimplexMethod.solve(record_history=False)``), or the
    ``IndexError`` the reference would raise.  ``statuses[k]`` is ``"optimum"``, ``"error"``,
    ``"cap"`` (``max_pivots`` reached) or ``"exception"``.

    Each problem goes where ``route`` says: the wave problems in one launch, the workgroup
    problems in the launches of ``wg_launches``, the global problems in the launches of
    ``gm_launches`` when the call holds at least ``GM_MIN_BATCH`` of them, the rest through
    ``SimplexMethod`` one by one.
    ``kernel="workgroup"`` sends the wave problems through the workgroup kernel too;
    ``kernel="wave"`` raises ValueError if a problem needs the workgroup kernel; both leave the
    global problems to ``SimplexMethod``.  ``kernel="global"`` sends the wave and workgroup
    problems through the global-memory kernel too, whatever their number.
    ``rule`` is the selection rule of every solve, as in ``solve_batch_arrays`` (the problems sent
    through ``SimplexMethod`` included); an unknown one raises ValueError first."""
    _lib.rule_code(rule)
    problems = list(problems)
    results = [None] * len(problems)
    statuses = [None] * len(problems)
    P = int(max_pivots)

    def single(k, c, f):
        results[k], statuses[k] = _fallback(c, f, max_pivots, history, rule)

    def launch(which, idx, tabs, dims):
        out = solve_batch_arrays(tabs, dims, max_pivots, history, device, kernel=which, rule=rule)
        # Hundreds of thousands of fresh, acyclic lists: pause the cyclic collector while they
        # are built, or its generational passes rescan the growing result set (5x slower at 20k
        # LPs).
        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            for q, k in enumerate(idx):
                results[k], statuses[k] = _assemble(
                    problems[k], dims[q], out["final"][q], out["rc"][q], out["xv"][q],
                    out["snaps"][out["snap_off"][q]:out["snap_off"][q + 1]] if history else None,
                    int(out["status"][q]), int(out["npivots"][q]), P)
        finally:
            if gc_was_on:
                gc.enable()

    _drive(problems, kernel, max_pivots, history, single, launch)
    return results, statuses


def _solve_batch_answers(problems, max_pivots, device, kernel, answer, ranging, at,
                         rule="reference"):
    """``solve_batch_solutions`` and ``solve_batch_ranges``: ``answer`` reads a fallback's result
    off its ``SimplexMethod``, ``at(arrays, q, n, m)`` a launch member's off the arrays."""
    _lib.rule_code(rule)
    problems = list(problems)
    results = [None] * len(problems)
    statuses = [None] * len(problems)
    P = int(max_pivots)

    def single(k, c, f):
        results[k], statuses[k] = _fallback_answer(c, f, max_pivots, answer, rule)

    def launch(which, idx, tabs, dims):
        out = solve_batch_arrays(tabs, dims, max_pivots, False, device, kernel=which,
                                 solution=True, tables=False, ranging=ranging, rule=rule)
        for q, k in enumerate(idx):
            results[k] = at(out, q, int(dims[q, 0]), int(dims[q, 1]))
            statuses[k] = _status_name(int(out["status"][q]), int(out["npivots"][q]), P)

    _drive(problems, kernel, max_pivots, False, single, launch)
    return results, statuses


def solve_batch_solutions(problems, max_pivots: int = 256, device=None, kernel: str = "auto",
                          rule: str = "reference"):
    """Solve every ``(constraints, function)`` for its whole answer; returns
    ``(solutions, statuses)``.

    ``solutions[k]`` is the ``Solution`` of problem k -- ``x`` [m], ``duals`` [n], ``objective``,
    ``basis`` [n], ``nonbasis`` [m] as numpy arrays and scalars, ``pivots`` -- equal to
    ``SimplexMethod(...).solution()`` after ``solve(record_history=False)``, or the ``IndexError``
    the reference would raise; ``statuses[k]`` as in ``solve_batch``.  The values stand whatever
    the status.  Routing and launch splitting are ``solve_batch``'s; of a launch only the
    solutions come back from the device (``solve_batch_arrays(solution=True, tables=False)``),
    and no ``Info`` objects are built.  ``rule`` as in ``solve_batch``."""
    return _solve_batch_answers(problems, max_pivots, device, kernel, SimplexMethod.solution,
                                False, _solution_at, rule)


def _ranging_at(arrays, q, n, m):
    return Ranging(arrays["rhs_lo"][q, :n].copy(), arrays["rhs_hi"][q, :n].copy(),
                   arrays["cost_lo"][q, :m].copy(), arrays["cost_hi"][q, :m].copy())


def solve_batch_ranges(problems, max_pivots: int = 256, device=None, kernel: str = "auto",
                       rule: str = "reference"):
    """Solve every ``(constraints, function)`` for the ranges of its final basis; returns
    ``(ranges, statuses)``.

    ``ranges[k]`` is the ``Ranging`` of problem k -- ``rhs_lo``, ``rhs_hi`` [n] and ``cost_lo``,
    ``cost_hi`` [m] as numpy arrays -- equal to ``SimplexMethod(...).ranging()`` after
    ``solve(record_history=False)``, or the ``IndexError`` the reference would raise;
    ``statuses[k]`` as in ``solve_batch``.  The values stand whatever the status.  Routing and
    launch splitting are ``solve_batch``'s; of a launch only the solutions and the ranges come
    back from the device (``solve_batch_arrays(solution=True, ranging=True, tables=False)``).
    ``rule`` as in ``solve_batch``."""
    return _solve_batch_answers(problems, max_pivots, device, kernel, SimplexMethod.ranging,
                                True, _ranging_at, rule)


def _warm_chain(L, dev, tabs, dims, tier, P, S, make, rows, warm_tier, Pw, ranging, log,
                warm_rule=_lib.RULE_REFERENCE, cols=None):
    """The chain of every warm call, on one stream and with no host round trip between the steps:
    the base launch of ``tabs`` / ``dims`` on ``tier`` (``_enqueue_base``), then for every slice of
    the S sets ``make(stream, s0, c, final, d_dims, func, basis, nonbasis)``, which enqueues the
    kernel that writes the B * c warm tables of sets s0..s0 + c - 1 (``rows`` rows and ``cols``
    columns each; ``cols`` None: as many columns as the base tables) from the base launch's
    device tensors and returns (tables, their dims, their function rows, the ``start`` of
    ``_device_solution``); the warm solve on ``warm_tier`` capped at ``Pw`` under
    the selection rule ``warm_rule`` (the base launch keeps the reference rule), its solution from
    ``start`` and, with ``ranging``, its ranges.  A slice holds as many sets as keep
    its tables under ``GM_TABLE_BUDGET``.  Only when everything is enqueued does anything come
    back: ``base`` (``_base_arrays``) and per set, shaped [B][S]..., ``status``, ``npivots``, with
    ``log`` the warm pivot log ``rc``, the solution arrays and with ``ranging`` the range arrays.
    S == 0 runs one slice of no sets, on which every library call returns at once, so that its
    result has the shapes of any other."""
    B, _, ldb = tabs.shape
    width = ldb if cols is None else cols
    per = max(1, min(S, GM_TABLE_BUDGET // max(1, B * rows * width * 8)))
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        d_tabs = torch.from_numpy(tabs).to(dev)
        d_dims = torch.from_numpy(dims).to(dev)
        run, d_func, sol, rng = _enqueue_base(L, stream, tier, d_tabs, d_dims, P, ranging=ranging)
        slices = []
        for s0 in range(0, S, per) or (0,):                  # S == 0: one slice, of no sets
            c = min(S, s0 + per) - s0
            d_wtabs, d_wdims, d_wfunc, start = make(stream, s0, c, run[0], d_dims, d_func,
                                                    sol[3], sol[4])
            d_wout, d_wrc, _, d_wst, d_wnp, _ = _device_solve(L, stream, warm_tier, d_wtabs,
                                                              d_wdims, Pw, rule=warm_rule)
            wsol = _device_solution(L, stream, d_wout, d_wdims, Pw, d_wrc, d_wnp, d_wfunc, start)
            wrng = _device_ranging(L, stream, d_wout, d_wdims, wsol[3], wsol[4]) if ranging else ()
            slices.append((c, d_wst, d_wnp, d_wrc if log else None, wsol, wrng))
            del d_wtabs, d_wout, d_wrc               # a slice's tables do not outlive it
        # everything is enqueued: only now does anything come back
        res = {"base": _base_arrays(run, sol, rng)}
        parts = []
        for c, d_wst, d_wnp, d_wrc, wsol, wrng in slices:
            part = {"status": d_wst.cpu().numpy().reshape(B, c),
                    "npivots": d_wnp.cpu().numpy().reshape(B, c)}
            if log:
                part["rc"] = d_wrc.cpu().numpy().reshape(B, c, max(Pw, 1), 2)
            part.update(_solution_arrays(wsol, (B, c)))
            if ranging:
                part.update(_ranging_arrays(wrng, (B, c)))
            parts.append(part)
    for key in parts[0]:
        res[key] = np.concatenate([p[key] for p in parts], axis=1)
    return res


def solve_batch_scenarios_arrays(tabs: np.ndarray, dims: np.ndarray, drhs: np.ndarray,
                                 dcost: np.ndarray, max_pivots: int = 256, warm_pivots=None,
                                 device=None, kernel: str = "auto", ranging: bool = False,
                                 warm_rule: str = "reference") -> dict:
    """Array-level what-if solve: every LP of ``tabs`` / ``dims`` (as in ``solve_batch_arrays``)
    and S scenarios of each.  ``drhs``: float64 [B][S][Rmax - 1], ``drhs[k, s, i]`` is added to
    the constant of constraint i of problem k; ``dcost``: float64 [B][S][ldb - 1], added to its
    ``function``; entries past n_k / m_k are not read and a delta equal to zero is skipped.

    One stream, no host round trip between the steps: the base solve, ``smx_batch_solution``
    (``ranging``: ``smx_batch_ranging``), then ``smx_batch_scenario`` (the scenario tables under
    every LP's final labels, include/smx.h), the warm solve of all B * S tables on the same kernel
    capped at ``warm_pivots`` (default: ``max_pivots``), ``smx_batch_solution_from`` (the labels
    carry on from the base LP's) and, with ``ranging``, ``smx_batch_ranging`` on the warm runs'
    final tables.  The scenario tables are made in slices of S that keep them under
    ``GM_TABLE_BUDGET``.

    Returns ``base``: exactly the dict of ``solve_batch_arrays(solution=True, tables=False,
    ranging=ranging)``; and per scenario, shaped [B][S]...: ``status``, ``npivots`` (the warm
    pivots only), ``x``, ``duals``, ``objective`` (on the scenario's own costs), ``basis``,
    ``nonbasis`` and with ``ranging`` the four range arrays.

    ``warm_rule`` is the selection rule of the WARM solve only (``"reference"`` or ``"dual"``; any
    other value raises ValueError before the device is asked for); the base solve keeps the
    reference rule, so ``base`` does not depend on it.  Under the default rule, which is no dual
    simplex, a warm run need not terminate where a cold solve of the perturbed problem would.
    Under ``"dual"`` (SMX_RULE_DUAL, include/smx.h) a scenario that moves constants only, after a
    base run that ended at an optimum, starts dual feasible and terminates, up to degenerate
    cycling; a scenario that also moves costs into a negative f-row entry takes the reference's
    steps.  Either way read ``status``; SMX_PIVOT there means ``warm_pivots`` was reached."""
    _kernel_name(kernel)
    wcode = _lib.rule_code(warm_rule)
    drhs = np.ascontiguousarray(drhs, dtype=np.float64)
    dcost = np.ascontiguousarray(dcost, dtype=np.float64)
    tabs, dims, (B, Rmax, ldb) = _launch_arrays(tabs, dims)
    if drhs.ndim != 3 or drhs.shape[0] != B or drhs.shape[2] != Rmax - 1:
        raise ValueError("drhs must be float64 [B][S][Rmax - 1]")
    S = drhs.shape[1]
    if dcost.shape != (B, S, ldb - 1):
        raise ValueError("dcost must be float64 [B][S][ldb - 1]")
    _need_device()
    which = _launch_tier(dims, (B, Rmax, ldb), kernel)
    if solution_lds_bytes(Rmax, ldb) < 0 or not scenario_fits(Rmax, ldb):
        raise ValueError(ENVELOPE_ERROR)
    if ranging and not ranging_fits(Rmax, ldb):
        raise ValueError(ENVELOPE_ERROR)
    P = int(max_pivots)
    Pw = P if warm_pivots is None else int(warm_pivots)
    L = _lib.load()
    # the deltas in the kernel's layout: rows of Rmax / ldb, the last entry unused
    h_dr = np.zeros((B, S, Rmax), dtype=np.float64)
    h_dr[:, :, :Rmax - 1] = drhs
    h_dc = np.zeros((B, S, ldb), dtype=np.float64)
    h_dc[:, :, :ldb - 1] = dcost
    dev = torch.device(device if device is not None else "cuda")
    with torch.cuda.device(dev):
        d_dr = torch.from_numpy(h_dr).to(dev)
        d_dc = torch.from_numpy(h_dc).to(dev)

    def make(stream, s0, c, d_final, d_dims, d_func, d_basis, d_nonbasis):
        Q = B * c
        d_ts = torch.empty((Q, Rmax, ldb), dtype=torch.float64, device=dev)
        d_fs = torch.empty((Q, ldb), dtype=torch.float64, device=dev)
        d_ds = torch.empty((Q, 3), dtype=torch.int32, device=dev)
        d_drs = d_dr[:, s0:s0 + c].contiguous()              # named: alive until the launch
        d_dcs = d_dc[:, s0:s0 + c].contiguous()
        _lib.check(L.smx_batch_scenario(
            d_final.data_ptr(), d_dims.data_ptr(), B, c, Rmax, ldb, d_basis.data_ptr(),
            d_nonbasis.data_ptr(), d_func.data_ptr(), d_drs.data_ptr(), d_dcs.data_ptr(),
            d_ts.data_ptr(), d_fs.data_ptr(), d_ds.data_ptr(), stream.cuda_stream),
            "smx_batch_scenario")
        # the labels carry on from the base LP's: table q starts from those of LP q / c (a slice
        # of no sets still names a legal group)
        return d_ts, d_ds, d_fs, (d_basis, d_nonbasis, max(c, 1))

    return _warm_chain(L, dev, tabs, dims, which, P, S, make, Rmax, which, Pw, ranging, False,
                       wcode)


def _perturbed(cons, func, drhs, dcost):
    """The ORIGINAL problem with a scenario's deltas added (a delta equal to zero skipped)."""
    cons = [list(r) for r in cons]
    func = list(func)
    if drhs is not None:
        for i, d in enumerate(drhs):
            if d != 0:
                cons[i][-1] = cons[i][-1] + float(d)
    if dcost is not None:
        for k, d in enumerate(dcost):
            if d != 0:
                func[k] = func[k] + float(d)
    return cons, func


def _fallback_warm(cons, func, sets, max_pivots, warm_pivots, successor, warm_rule="reference"):
    """One problem and its sets through ``SimplexMethod``; ``successor(sm, set)`` is the warm
    object of a set (``what_if`` / ``add_constraints``), solved under ``warm_rule``."""
    try:
        sm = SimplexMethod(cons, func)
        sm.solve(record_history=False, max_pivots=max_pivots)
        base = sm.solution()
        out = []
        for entry in sets:
            warm = successor(sm, entry)
            warm.solve(record_history=False, max_pivots=warm_pivots, rule=warm_rule)
            out.append(Scenario(warm.solution(), warm.status, True))
        return base, out
    except IndexError as exc:        # where the reference itself raises (simplex.py:49, 95, 159)
        return exc, [Scenario(exc, "exception", True) for _ in sets]


def _warm_answers(out, q, n, m, added, Pw, wide=False):
    """(Solution, [Scenario]) of member q of a warm launch; set s holds n + added[s] rows
    (``wide``: m + added[s] variables)."""
    return (_solution_at(out["base"], q, n, m),
            [Scenario(_solution_at(out, (q, s), n if wide else n + a, m + a if wide else m),
                      _status_name(int(out["status"][q, s]), int(out["npivots"][q, s]), Pw), True)
             for s, a in enumerate(added)])


def _cold_tail(results, cold_problem, max_pivots, device, kernel):
    """``cold_fallback``: every set whose warm run did not end at an optimum is solved cold, as
    the problem ``cold_problem(k, s)``, through ``solve_batch_solutions``."""
    todo = [(k, s) for k, (_, answers) in enumerate(results) for s, sc in enumerate(answers)
            if sc.status not in ("optimum", "exception")]
    if todo:
        sols, sts = solve_batch_solutions([cold_problem(k, s) for k, s in todo], max_pivots,
                                          device, kernel)
        for (k, s), sol, st in zip(todo, sols, sts):
            results[k][1][s] = Scenario(sol, st, False)


def solve_batch_scenarios(problems, scenarios, max_pivots: int = 256, warm_pivots=None,
                          cold_fallback: bool = True, device=None, kernel: str = "auto",
                          warm_rule: str = "reference"):
    """Solve every ``(constraints, function)`` and its what-if scenarios; ``scenarios[k]`` is a
    list of ``(drhs, dcost)`` for problem k (``drhs`` [n] added to the constraints' constants,
    ``dcost`` [m] to ``function``; either may be ``None``).  Returns per problem ``(Solution,
    [Scenario])``: the base answer as ``solve_batch_solutions`` gives it and one ``Scenario`` per
    entry of ``scenarios[k]``, in order.

    Routing and launch grouping are ``solve_batch_solutions``'s; inside a launch the scenario
    counts are padded with all-zero scenarios and dropped again
    (``solve_batch_scenarios_arrays``).  Problems routed ``"single"`` go through
    ``SimplexMethod.what_if``.  A warm run is capped at ``warm_pivots`` (default ``max_pivots``)
    and under the default rule need not terminate; with ``cold_fallback`` every scenario whose
    warm run did not end at ``"optimum"`` is solved cold from the perturbed original through
    ``solve_batch_solutions`` with the full ``max_pivots`` and marked ``warm=False``.
    ``warm_rule`` (``"reference"`` / ``"dual"``, as in ``solve_batch_scenarios_arrays``) is the rule
    of the warm solves only -- the base solves and the cold re-solves keep the reference rule."""
    problems = list(problems)
    scenarios = [list(s) for s in scenarios]
    _kernel_name(kernel)                                     # refused before the scenarios are
    _lib.rule_code(warm_rule)
    if len(scenarios) != len(problems):
        raise ValueError("scenarios must hold one list of scenarios per problem")
    P = int(max_pivots)
    Pw = P if warm_pivots is None else int(warm_pivots)
    results = [None] * len(problems)

    def single(k, c, f):
        results[k] = _fallback_warm(c, f, scenarios[k], P, Pw, lambda sm, sc: sm.what_if(*sc),
                                    warm_rule)

    def launch(which, idx, tabs, dims):
        _, Rmax, ldb = tabs.shape
        S = max(len(scenarios[k]) for k in idx)
        drhs = np.zeros((len(idx), S, Rmax - 1), dtype=np.float64)
        dcost = np.zeros((len(idx), S, ldb - 1), dtype=np.float64)
        for q, k in enumerate(idx):
            n, m = int(dims[q, 0]), int(dims[q, 1])
            for s, (dr, dc) in enumerate(scenarios[k]):
                if dr is not None:
                    drhs[q, s, :n] = np.asarray(dr, dtype=np.float64).reshape(n)
                if dc is not None:
                    dcost[q, s, :m] = np.asarray(dc, dtype=np.float64).reshape(m)
        out = solve_batch_scenarios_arrays(tabs, dims, drhs, dcost, P, Pw, device, kernel=which,
                                           warm_rule=warm_rule)
        for q, k in enumerate(idx):
            results[k] = _warm_answers(out, q, int(dims[q, 0]), int(dims[q, 1]),
                                       [0] * len(scenarios[k]), Pw)

    _drive(problems, kernel, max_pivots, False, single, launch)
    if cold_fallback:
        _cold_tail(results, lambda k, s: _perturbed(*problems[k], *scenarios[k][s]), max_pivots,
                   device, kernel)
    return results


_TIERS = ("wave", "workgroup", "global")


def warm_kernel(base: str, Rmax_out: int, ldb: int) -> str:
    """The kernel the enlarged tables of a cut launch run on: the first tier at or above the base
    run's (``"wave"`` < ``"workgroup"`` < ``"global"``) that takes Rmax_out x ldb blocks.  Raises
    ValueError when none does."""
    for which in _TIERS[_TIERS.index(base):]:
        try:
            return choose_kernel(Rmax_out, ldb, which)
        except ValueError:
            continue
    raise ValueError(ENVELOPE_ERROR)


def _enqueue_cuts(L, stream, d_final, d_dims, d_func, d_basis, d_nonbasis, d_cs, d_ns):
    """Enqueue smx_batch_cuts for the slice ``d_cs`` [B][c][K][ldb] / ``d_ns`` [B][c] on fresh
    outputs; returns what ``_warm_chain`` asks of its ``make``."""
    (B, Rmax, ldb), c, K, dev = d_final.shape, d_ns.shape[1], d_cs.shape[2], d_final.device
    d_tc = torch.empty((B * c, Rmax + K, ldb), dtype=torch.float64, device=dev)
    d_dc = torch.empty((B * c, 3), dtype=torch.int32, device=dev)
    d_bc = torch.empty((B * c, Rmax + K), dtype=torch.int32, device=dev)
    _lib.check(L.smx_batch_cuts(
        d_final.data_ptr(), d_dims.data_ptr(), B, c, Rmax, ldb, d_basis.data_ptr(),
        d_nonbasis.data_ptr(), d_cs.data_ptr() if K else None, d_ns.data_ptr(), K, Rmax + K,
        d_tc.data_ptr(), d_dc.data_ptr(), d_bc.data_ptr(), stream.cuda_stream),
        "smx_batch_cuts")
    # every table's own start labels (group 1): its LP's column labels and function row
    return (d_tc, d_dc, d_func.repeat_interleave(c, dim=0),
            (d_bc, d_nonbasis.repeat_interleave(c, dim=0), 1))


def _enqueue_cols(L, stream, d_final, d_dims, d_func, d_basis, d_nonbasis, d_cs, d_ns):
    """Enqueue smx_batch_cols for the slice ``d_cs`` [B][c][K][Rmax] / ``d_ns`` [B][c] on fresh
    outputs; returns what ``_warm_chain`` asks of its ``make``."""
    (B, Rmax, ldb), c, K, dev = d_final.shape, d_ns.shape[1], d_cs.shape[2], d_final.device
    d_tv = torch.empty((B * c, Rmax, ldb + K), dtype=torch.float64, device=dev)
    d_fv = torch.empty((B * c, ldb + K), dtype=torch.float64, device=dev)
    d_dv = torch.empty((B * c, 3), dtype=torch.int32, device=dev)
    d_bv = torch.empty((B * c, Rmax), dtype=torch.int32, device=dev)
    d_nv = torch.empty((B * c, ldb + K), dtype=torch.int32, device=dev)
    _lib.check(L.smx_batch_cols(
        d_final.data_ptr(), d_dims.data_ptr(), B, c, Rmax, ldb, d_basis.data_ptr(),
        d_nonbasis.data_ptr(), d_func.data_ptr(), d_cs.data_ptr() if K else None,
        d_ns.data_ptr(), K, ldb + K, d_tv.data_ptr(), d_fv.data_ptr(), d_dv.data_ptr(),
        d_bv.data_ptr(), d_nv.data_ptr(), stream.cuda_stream), "smx_batch_cols")
    # every table's own start labels (group 1), in the widened LP's coding
    return d_tv, d_dv, d_fv, (d_bv, d_nv, 1)


def _grown_arrays(wide, tabs, dims, sets, counts, max_pivots, warm_pivots, device, kernel,
                  ranging, log, warm_rule):
    """``solve_batch_cuts_arrays`` (``wide`` False: K rows of ldb entries are added to every
    table) and ``solve_batch_columns_arrays`` (``wide`` True: K columns of Rmax entries), stated
    once: the checks in their order, the upload and the ``_warm_chain`` whose ``make`` enqueues the
    feature's kernel (``_enqueue_cuts`` / ``_enqueue_cols``) on a slice of the sets."""
    name, last, fits, enqueue = (("cols", "Rmax", cols_fits, _enqueue_cols) if wide else
                                 ("cuts", "ldb", cuts_fits, _enqueue_cuts))
    _kernel_name(kernel)
    wcode = _lib.rule_code(warm_rule)
    sets = np.ascontiguousarray(sets, dtype=np.float64)
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    tabs, dims, (B, Rmax, ldb) = _launch_arrays(tabs, dims)
    if sets.ndim != 4 or sets.shape[0] != B or sets.shape[3] != (Rmax if wide else ldb):
        raise ValueError(f"{name} must be float64 [B][S][K][{last}]")
    S, K = sets.shape[1], sets.shape[2]
    if counts.shape != (B, S):
        raise ValueError(f"n{name} must be int32 [B][S]")
    if ((counts < 0) | (counts > K)).any():
        raise ValueError(f"n{name} must lie in 0..K")
    if wide and B and S and ((dims[:, 2] < dims[:, 1]) & (counts > 0).any(axis=1)).any():
        raise ValueError("a problem whose function is shorter than m takes no new variables")
    _need_device()
    rows, width = (Rmax, ldb + K) if wide else (Rmax + K, ldb)
    which = _launch_tier(dims, (B, Rmax, ldb), kernel)
    warm = warm_kernel(which, rows, width) if B else "wave"
    if solution_lds_bytes(rows, width) < 0 or not fits(rows, width):
        raise ValueError(ENVELOPE_ERROR)
    if ranging and not ranging_fits(rows, width):
        raise ValueError(ENVELOPE_ERROR)
    P = int(max_pivots)
    Pw = P if warm_pivots is None else int(warm_pivots)
    L = _lib.load()
    dev = torch.device(device if device is not None else "cuda")
    with torch.cuda.device(dev):
        d_sets = torch.from_numpy(sets).to(dev)
        d_counts = torch.from_numpy(counts).to(dev)

    def make(stream, s0, c, *base):
        return enqueue(L, stream, *base, d_sets[:, s0:s0 + c].contiguous(),
                       d_counts[:, s0:s0 + c].contiguous())

    return _warm_chain(L, dev, tabs, dims, which, P, S, make, rows, warm, Pw, ranging, log,
                       wcode, cols=width if wide else None)


def solve_batch_cuts_arrays(tabs: np.ndarray, dims: np.ndarray, cuts: np.ndarray,
                            ncuts: np.ndarray, max_pivots: int = 256, warm_pivots=None,
                            device=None, kernel: str = "auto", ranging: bool = False,
                            log: bool = False, warm_rule: str = "reference") -> dict:
    """Array-level solve with new constraints: every LP of ``tabs`` / ``dims`` (as in
    ``solve_batch_arrays``) and S cut sets of each.  ``cuts``: float64 [B][S][K][ldb], row
    ``cuts[k, s, c]`` is a constraint of problem k in the format of its own rows (entry m_k the
    constant; entries past it are not read); ``ncuts``: int32 [B][S], how many of the K rows set
    s of problem k holds (0..K, else ValueError).

    One stream, no host round trip between the steps: the base solve, ``smx_batch_solution``
    (``ranging``: ``smx_batch_ranging``), then ``smx_batch_cuts`` (the extended tables of Rmax + K
    rows under every LP's final labels, include/smx.h), the warm solve of all B * S tables capped
    at ``warm_pivots`` (default: ``max_pivots``), ``smx_batch_solution_from`` (group 1: every
    table starts from its own extended labels) and, with ``ranging``, ``smx_batch_ranging`` on
    the warm runs' final tables.  The warm solve's kernel is chosen again for (Rmax + K, ldb)
    (``warm_kernel``): a launch may leave the wavefront tier for the workgroup tier or the LDS
    edge for the global-memory tier; a shape that leaves every tier raises ValueError.  The
    extended tables are made in slices of S that keep them under ``GM_TABLE_BUDGET``.

    Returns ``base`` exactly as ``solve_batch_scenarios_arrays`` does; and per cut set, shaped
    [B][S]...: ``status``, ``npivots`` (the warm pivots only; with ``log`` also their log ``rc``
    [warm_pivots][2], B * S * warm_pivots * 8 bytes to copy back), ``x`` [ldb - 1], ``duals``
    [Rmax + K - 1] (the new constraints' included, at n_k..n_k + ncuts - 1), ``objective``,
    ``basis`` [Rmax + K - 1], ``nonbasis`` [ldb - 1] and with ``ranging`` the four range arrays.
    A new constraint's label code is m_k + n_k + c.

    ``warm_rule`` is the selection rule of the WARM solve only (``"reference"`` or ``"dual"``; any
    other value raises ValueError before the device is asked for); ``base`` does not depend on it.
    Under the default rule, which is no dual simplex, a warm run need not terminate where a cold
    solve of the enlarged problem would.  An extended table keeps its base run's f-row, so after a
    base run that ended at an optimum it is dual feasible and under ``"dual"`` (SMX_RULE_DUAL,
    include/smx.h) the warm run terminates, up to degenerate cycling.  Either way read ``status``;
    SMX_PIVOT there means ``warm_pivots`` was reached."""
    return _grown_arrays(False, tabs, dims, cuts, ncuts, max_pivots, warm_pivots, device, kernel,
                         ranging, log, warm_rule)


def _enlarged(cons, func, rows):
    """The ORIGINAL problem with a cut set's rows appended."""
    return [list(r) for r in cons] + [[float(v) for v in r] for r in rows], list(func)


def _solve_batch_grown(wide, problems, sets, max_pivots, warm_pivots, cold_fallback, device, kernel,
                       warm_rule):
    """``solve_batch_cuts`` (``wide`` False) and ``solve_batch_columns`` (``wide`` True) once their
    ``sets`` are checked: a launch pads its members' sets into [len(idx)][S][K][ldb or Rmax] plus
    counts and goes through the array level, unless its grown tables leave every tier
    (``warm_kernel``): then, like the problems routed ``"single"``, its members go one by one."""
    arrays, successor, grown = (
        (solve_batch_columns_arrays, SimplexMethod.add_variables, _widened) if wide else
        (solve_batch_cuts_arrays, SimplexMethod.add_constraints, _enlarged))
    P = int(max_pivots)
    Pw = P if warm_pivots is None else int(warm_pivots)
    results = [None] * len(problems)

    def single(k, c, f):
        results[k] = _fallback_warm(c, f, sets[k], P, Pw, successor, warm_rule)

    def launch(which, idx, tabs, dims):
        _, Rmax, ldb = tabs.shape
        S = max(len(sets[k]) for k in idx)
        K = max((len(new) for k in idx for new in sets[k]), default=0)
        try:
            warm_kernel(which, *((Rmax, ldb + K) if wide else (Rmax + K, ldb)))
        except ValueError:
            for k in idx:
                single(k, *problems[k])
            return
        g = np.zeros((len(idx), S, K, Rmax if wide else ldb), dtype=np.float64)
        nc = np.zeros((len(idx), S), dtype=np.int32)
        for q, k in enumerate(idx):
            used = int(dims[q, 0 if wide else 1]) + 1
            for s, new in enumerate(sets[k]):
                nc[q, s] = len(new)
                if new:
                    g[q, s, :len(new), :used] = np.asarray(new, dtype=np.float64)
        out = arrays(tabs, dims, g, nc, P, Pw, device, kernel=which, warm_rule=warm_rule)
        for q, k in enumerate(idx):
            results[k] = _warm_answers(out, q, int(dims[q, 0]), int(dims[q, 1]),
                                       [len(new) for new in sets[k]], Pw, wide)

    _drive(problems, kernel, max_pivots, False, single, launch)
    if cold_fallback:
        _cold_tail(results, lambda k, s: grown(*problems[k], sets[k][s]), max_pivots, device,
                   kernel)
    return results


def solve_batch_cuts(problems, cuts, max_pivots: int = 256, warm_pivots=None,
                     cold_fallback: bool = True, device=None, kernel: str = "auto",
                     warm_rule: str = "reference"):
    """Solve every ``(constraints, function)`` and, for each of its cut sets, the problem with
    that set's constraints added; ``cuts[k]`` is a list of cut sets of problem k, each a list of
    rows in the constraints' own format ([m coefficients, constant]; an empty set adds nothing).
    Returns per problem ``(Solution, [Scenario])``: the base answer as ``solve_batch_solutions``
    gives it and one ``Scenario`` per cut set, in order, whose ``Solution`` has n + K' duals and
    row labels (a new constraint's code is m + n + c).

    Routing and launch grouping are ``solve_batch_solutions``'s; inside a launch the set counts
    and sizes are padded with empty sets and dropped again (``solve_batch_cuts_arrays``).
    Problems routed ``"single"``, and those of a launch whose enlarged tables leave every batch
    kernel's envelope, go through ``SimplexMethod.add_constraints``.  A warm run is capped at
    ``warm_pivots`` (default ``max_pivots``) and under the default rule need not terminate; with
    ``cold_fallback`` every set whose warm run did not end at ``"optimum"`` is solved cold from
    the enlarged original through ``solve_batch_solutions`` with the full ``max_pivots`` and
    marked ``warm=False``.  ``warm_rule`` (``"reference"`` / ``"dual"``, as in
    ``solve_batch_cuts_arrays``) is the rule of the warm solves only -- the base solves and the
    cold re-solves keep the reference rule."""
    problems = list(problems)
    cuts = [[[list(r) for r in rows] for rows in sets] for sets in cuts]
    _kernel_name(kernel)                                     # refused before the cuts are
    _lib.rule_code(warm_rule)
    if len(cuts) != len(problems):
        raise ValueError("cuts must hold one list of cut sets per problem")
    for (c, _), sets in zip(problems, cuts):
        if any(len(r) != len(c[0]) for rows in sets for r in rows):
            raise ValueError("a cut must have the length of its problem's constraints")
    return _solve_batch_grown(False, problems, cuts, max_pivots, warm_pivots, cold_fallback, device,
                              kernel, warm_rule)


def solve_batch_columns_arrays(tabs: np.ndarray, dims: np.ndarray, cols: np.ndarray,
                               ncols: np.ndarray, max_pivots: int = 256, warm_pivots=None,
                               device=None, kernel: str = "auto", ranging: bool = False,
                               log: bool = False, warm_rule: str = "reference") -> dict:
    """Array-level solve with new variables: every LP of ``tabs`` / ``dims`` (as in
    ``solve_batch_arrays``) and S column sets of each.  ``cols``: float64 [B][S][K][Rmax], column
    ``cols[k, s, c]`` holds the new variable's coefficient in every constraint of problem k
    (entries 0..n_k - 1) and its entry in ``function`` (entry n_k; entries past it are not read);
    ``ncols``: int32 [B][S], how many of the K columns set s of problem k holds (0..K, else
    ValueError).  A problem whose ``function`` is shorter than m_k takes no columns (ValueError).

    One stream, no host round trip between the steps: the base solve, ``smx_batch_solution``
    (``ranging``: ``smx_batch_ranging``), then ``smx_batch_cols`` (the widened tables of ldb + K
    columns under every LP's final labels, recoded; include/smx.h), the warm solve of all B * S
    tables capped at ``warm_pivots`` (default: ``max_pivots``), ``smx_batch_solution_from`` (group
    1: every table starts from its own recoded labels) and, with ``ranging``,
    ``smx_batch_ranging`` on the warm runs' final tables.  The warm solve's kernel is chosen again
    for (Rmax, ldb + K) (``warm_kernel``): a launch may leave the wavefront tier for the workgroup
    tier or the LDS edge for the global-memory tier; a shape that leaves every tier raises
    ValueError before anything is enqueued.  The widened tables are made in slices of S that keep
    them under ``GM_TABLE_BUDGET``.

    Returns ``base`` exactly as ``solve_batch_scenarios_arrays`` does; and per column set, shaped
    [B][S]...: ``status``, ``npivots`` (the warm pivots only; with ``log`` also their log ``rc``
    [warm_pivots][2]), ``x`` [ldb + K - 1] (the new variables' included, at m_k..m_k + ncols - 1),
    ``duals`` [Rmax - 1], ``objective`` (on the widened ``function``), ``basis`` [Rmax - 1],
    ``nonbasis`` [ldb + K - 1] and with ``ranging`` the four range arrays.  The labels are in the
    widened LP's coding: a new variable's code is m_k + c, slack i's is m_k + ncols + i.

    ``warm_rule`` is the selection rule of the WARM solve only (``"reference"`` or ``"dual"``; any
    other value raises ValueError before the device is asked for); ``base`` does not depend on it.
    A new variable leaves every constant as it was, so after a base run that ended at an optimum
    the widened table is primal feasible and the default rule carries on as an ordinary primal
    simplex.  Read ``status`` all the same; SMX_PIVOT there means ``warm_pivots`` was reached."""
    return _grown_arrays(True, tabs, dims, cols, ncols, max_pivots, warm_pivots, device, kernel,
                         ranging, log, warm_rule)


def _widened(cons, func, columns):
    """The ORIGINAL problem with a column set's variables inserted: the coefficients before every
    constraint's constant, the costs into ``function`` at position m."""
    m = len(cons[0]) - 1
    cons = [list(r[:m]) + [float(a[i]) for a in columns] + list(r[m:]) for i, r in enumerate(cons)]
    func = list(func[:m]) + [float(a[-1]) for a in columns] + list(func[m:])
    return cons, func


def solve_batch_columns(problems, columns, max_pivots: int = 256, warm_pivots=None,
                        cold_fallback: bool = True, device=None, kernel: str = "auto",
                        warm_rule: str = "reference"):
    """Solve every ``(constraints, function)`` and, for each of its column sets, the problem with
    that set's variables added; ``columns[k]`` is a list of column sets of problem k, each a list
    of new variables ([n coefficients, cost]: the variable's coefficient in every constraint, then
    its entry in ``function``; an empty set adds nothing).  Returns per problem ``(Solution,
    [Scenario])``: the base answer as ``solve_batch_solutions`` gives it and one ``Scenario`` per
    column set, in order, whose ``Solution`` has m + K' entries of ``x`` and column labels in the
    widened LP's coding (a new variable's code is m + c, slack i's is m + K' + i).

    Routing and launch grouping are ``solve_batch_solutions``'s; inside a launch the set counts
    and sizes are padded with empty sets and dropped again (``solve_batch_columns_arrays``).
    Problems routed ``"single"``, and those of a launch whose widened tables leave every batch
    kernel's envelope, go through ``SimplexMethod.add_variables``.  A warm run is capped at
    ``warm_pivots`` (default ``max_pivots``); with ``cold_fallback`` every set whose warm run did
    not end at ``"optimum"`` is solved cold from the widened original through
    ``solve_batch_solutions`` with the full ``max_pivots`` and marked ``warm=False``.
    ``warm_rule`` (``"reference"`` / ``"dual"``, as in ``solve_batch_columns_arrays``) is the rule
    of the warm solves only -- the base solves and the cold re-solves keep the reference rule."""
    problems = list(problems)
    columns = [[[list(a) for a in cols] for cols in sets] for sets in columns]
    _kernel_name(kernel)                                     # refused before the columns are
    _lib.rule_code(warm_rule)
    if len(columns) != len(problems):
        raise ValueError("columns must hold one list of column sets per problem")
    for (c, _), sets in zip(problems, columns):
        if any(len(a) != len(c) + 1 for cols in sets for a in cols):
            raise ValueError("a new variable must hold one coefficient per constraint and a cost")
    return _solve_batch_grown(True, problems, columns, max_pivots, warm_pivots, cold_fallback,
                              device, kernel, warm_rule)


def branch_fits(Rmax_out: int, ldb: int) -> bool:
    """Whether blocks of Rmax_out x ldb are inside the branch kernels' envelope (``cuts_fits``)."""
    return bool(_envelope("smx_batch_branch_fits", Rmax_out, ldb, False))


def _device_pick(L, stream, node, d_ints, d_lp, tol):
    """Enqueue smx_batch_branch_pick on the nodes ``node`` = (final, dims, basis, nonbasis, func)
    on fresh outputs; returns the device tensors (bvar, brow, bval, bneg, bmin)."""
    d_final, d_dims, d_basis = node[0], node[1], node[2]
    Q, Rmax, ldb = d_final.shape
    dev = d_final.device
    d_bvar = torch.empty(Q, dtype=torch.int32, device=dev)
    d_brow = torch.empty(Q, dtype=torch.int32, device=dev)
    d_bval, d_bneg, d_bmin = (torch.empty(Q, dtype=torch.float64, device=dev) for _ in "vnm")
    _lib.check(L.smx_batch_branch_pick(
        d_final.data_ptr(), d_dims.data_ptr(), Q, Rmax, ldb, d_basis.data_ptr(),
        d_ints.data_ptr(), d_ints.shape[0], d_lp.data_ptr(), float(tol), d_bvar.data_ptr(),
        d_brow.data_ptr(), d_bval.data_ptr(), d_bneg.data_ptr(), d_bmin.data_ptr(),
        stream.cuda_stream), "smx_batch_branch_pick")
    return d_bvar, d_brow, d_bval, d_bneg, d_bmin


def _device_branch(L, stream, node, d_src, d_brow, Rout, snap):
    """Enqueue smx_batch_branch for the parents ``d_src`` of the nodes ``node`` on fresh outputs
    of ``Rout`` rows; returns the children as (tabs, dims, basis, nonbasis, func)."""
    d_final, d_dims, d_basis, d_nonbasis, d_func = node
    Q, Rmax, ldb = d_final.shape
    Qc, dev = len(d_src), d_final.device
    d_tc = torch.empty((2 * Qc, Rout, ldb), dtype=torch.float64, device=dev)
    d_dc = torch.empty((2 * Qc, 3), dtype=torch.int32, device=dev)
    d_bc = torch.empty((2 * Qc, Rout), dtype=torch.int32, device=dev)
    d_nc = torch.empty((2 * Qc, ldb), dtype=torch.int32, device=dev)
    d_fc = torch.empty((2 * Qc, ldb), dtype=torch.float64, device=dev)
    _lib.check(L.smx_batch_branch(
        d_final.data_ptr(), d_dims.data_ptr(), Q, Rmax, ldb, d_basis.data_ptr(),
        d_nonbasis.data_ptr(), d_func.data_ptr(), d_src.data_ptr(), d_brow.data_ptr(), Qc, Rout,
        float(snap), d_tc.data_ptr(), d_dc.data_ptr(), d_bc.data_ptr(), d_nc.data_ptr(), d_fc.data_ptr(),
        stream.cuda_stream), "smx_batch_branch")
    return d_tc, d_dc, d_bc, d_nc, d_fc


def solve_batch_integer_arrays(tabs: np.ndarray, dims: np.ndarray, integers=None,
                               max_pivots: int = 256, warm_pivots=None, max_depth: int = 16,
                               max_nodes=None, int_tol: float = 1e-6, rule: str = "reference",
                               kernel: str = "auto", device=None) -> dict:
    """Array-level integer solve: every LP of ``tabs`` / ``dims`` (as in ``solve_batch_arrays``)
    with the variables marked in ``integers`` (None: all; else [B][ldb - 1], non-zero: x{k+1} of
    problem k must be whole) held to whole numbers, by branch and bound on the device.  The
    method minimises ``function . x``.

    The root solve is ``solve_batch_arrays``'s chain under ``rule``; only roots at SMX_OPTIMUM
    enter the tree.  Then level by level, the tables never leaving the device: the pick on the
    frontier (``smx_batch_branch_pick``); ``status``, ``objective`` and the pick's per-node
    scalars come back (small arrays only) and the host updates every problem's incumbent (an integral node, the
    lowest objective), prunes (a node whose objective is not below its problem's incumbent) and
    lists the nodes to expand; ``smx_batch_branch`` writes both children of each into fresh
    buffers (the parents' are released once the children are solved: two frontiers are alive);
    one warm solve of all children under SMX_RULE_DUAL capped at ``warm_pivots`` (default:
    ``max_pivots``) on the kernel chosen once by ``warm_kernel(base, Rmax + max_depth, ldb)``;
    ``smx_batch_solution_from(group=1)`` with the children's own labels.  From level 1 on every
    block has Rmax + max_depth rows.  A child at SMX_INCORRECT on a row that misses by more than
    ``int_tol`` is empty and dropped (``branch.Tree.children``: the pick also reports how far a
    node's constants are below zero, since the kernels compare with zero exactly; a constant that
    misses zero from below by less is written to the children as zero).  A node that
    can be neither closed nor expanded -- a warm run at its cap or at SMX_NOT_CONVERGE, a node at
    ``max_depth``, what a frontier past ``max_nodes`` children (default: what keeps two frontiers
    under ``GM_TABLE_BUDGET``; the lowest objectives are kept, ties by node index) leaves out --
    counts a valid lower bound into its problem's ``bound`` and makes its status ``"limit"``:
    ``"optimal"`` is reported only when every node of the problem was closed.  A shape whose
    blocks of Rmax + max_depth rows leave every tier raises ValueError before anything is
    enqueued.  ``int_tol``: how far from a whole number a marked variable may stand and count as
    whole; 1e-6 is a convention of LP-based integer solvers, not a measured number.

    Returns per problem: ``status`` (list of "optimal", "infeasible", "limit" or the root's own
    "error" / "cap"), ``x`` [B][ldb - 1] (the marked variables rounded to the nearest whole number;
    NaN without an answer), ``x_raw``, ``objective`` [B] (on the rounded ``x``, by
    ``smx_batch_solution``'s ordered sum; +inf without an answer), ``bound`` [B], ``nodes``,
    ``warm_pivots`` and ``depth`` [B], ``found`` [B] (whether ``x`` holds an answer) and
    ``root_status`` (SMX_* codes)."""
    from . import branch
    _kernel_name(kernel)
    code = _lib.rule_code(rule)
    tabs, dims, (B, Rmax, ldb) = _launch_arrays(tabs, dims)
    if integers is None:
        integers = np.ones((B, ldb - 1), dtype=np.int32)
    integers = np.asarray(integers)
    if integers.shape != (B, ldb - 1):
        raise ValueError("integers must be [B][ldb - 1]")
    depth = int(max_depth)
    if depth < 0:
        raise ValueError("max_depth must not be negative")
    _need_device()
    Rout = Rmax + depth
    which = _launch_tier(dims, (B, Rmax, ldb), kernel)
    warm = warm_kernel(which, Rout, ldb) if B else "wave"
    if solution_lds_bytes(Rout, ldb) < 0 or not branch_fits(Rout, ldb):
        raise ValueError(ENVELOPE_ERROR)
    P = int(max_pivots)
    Pw = P if warm_pivots is None else int(warm_pivots)
    if max_nodes is None:
        max_nodes = branch.default_max_nodes(Rout, ldb, GM_TABLE_BUDGET)
    h_ints = np.zeros((B, ldb), dtype=np.int32)
    h_ints[:, :ldb - 1] = integers != 0
    tree = branch.Tree(B, depth, max_nodes, int_tol)
    L = _lib.load()
    dev = torch.device(device if device is not None else "cuda")
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        d_tabs = torch.from_numpy(tabs).to(dev)
        d_dims = torch.from_numpy(dims).to(dev)
        d_ints = torch.from_numpy(h_ints).to(dev)
        run, d_func, sol, _ = _enqueue_base(L, stream, which, d_tabs, d_dims, P, rule=code)
        root_status = run[3].cpu().numpy()
        root_np = run[4].cpu().numpy()
        live = tree.start([_status_name(int(s), int(p), P) for s, p in zip(root_status, root_np)])
        h_obj = sol[2].cpu().numpy()
        frontier = [(k, k, float(h_obj[k])) for k in live]
        node, d_x = (run[0], d_dims, sol[3], sol[4], d_func), sol[0]
        h_lp = np.arange(B, dtype=np.int32)
        level = 0
        picks = _device_pick(L, stream, node, d_ints, torch.from_numpy(h_lp).to(dev), int_tol)
        while frontier:
            d_brow = picks[1]
            parents = tree.close(
                level, frontier, picks[0].cpu().numpy(),
                lambda qs: d_x[torch.as_tensor(qs, dtype=torch.long, device=dev)].cpu().numpy())
            if not parents:
                break
            level += 1
            h_src = np.array([q for q, _, _ in parents], dtype=np.int32)
            d_src = torch.from_numpy(h_src).to(dev)
            kids = _device_branch(L, stream, node, d_src, d_brow, Rout, int_tol)
            d_out, d_rc, _, d_st, d_np, _ = _device_solve(L, stream, warm, kids[0], kids[1], Pw,
                                                          rule=_lib.RULE_DUAL)
            wsol = _device_solution(L, stream, d_out, kids[1], Pw, d_rc, d_np, kids[4],
                                    (kids[2], kids[3], 1))
            h_lp = np.repeat(h_lp[h_src], 2)
            node, d_x = (d_out, kids[1], wsol[3], wsol[4], kids[4]), wsol[0]
            picks = _device_pick(L, stream, node, d_ints, torch.from_numpy(h_lp).to(dev), int_tol)
            frontier = tree.children(level, parents, d_st.cpu().numpy(), d_np.cpu().numpy(),
                                     wsol[2].cpu().numpy(), picks[3].cpu().numpy(),
                                     picks[4].cpu().numpy())
            del kids, d_rc                                   # the parents' buffers go with `node`
    res = {"status": [], "x": np.full((B, ldb - 1), np.nan), "x_raw": np.full((B, ldb - 1), np.nan),
           "objective": np.full(B, np.inf), "bound": np.zeros(B),
           "nodes": np.zeros(B, dtype=np.int64), "warm_pivots": np.zeros(B, dtype=np.int64),
           "depth": np.zeros(B, dtype=np.int64), "root_status": root_status,
           "found": np.zeros(B, dtype=bool)}
    for k in range(B):
        n, m = int(dims[k, 0]), int(dims[k, 1])
        ans = tree.answer(k, tabs[k, n, :m], h_ints[k, :m])
        res["status"].append(ans.status)
        if ans.x is not None:
            res["found"][k] = True
            res["x"][k, :m], res["x_raw"][k, :m] = ans.x, ans.x_raw
            res["x"][k, m:] = res["x_raw"][k, m:] = 0.0
        res["objective"][k], res["bound"][k] = ans.objective, ans.bound
        res["nodes"][k], res["warm_pivots"][k], res["depth"][k] = (ans.nodes, ans.warm_pivots,
                                                                   ans.depth)
    return res


def solve_batch_integer(problems, integers=None, max_pivots: int = 256, warm_pivots=None,
                        max_depth: int = 16, max_nodes=None, int_tol: float = 1e-6,
                        rule: str = "reference", kernel: str = "auto", device=None):
    """Solve every ``(constraints, function)`` with the variables marked in ``integers[k]`` (None,
    for the call or for a problem: all of them; else m truth values) held to whole numbers;
    returns one ``IntegerSolution`` (branch.py) per problem, or the ``IndexError`` the reference
    would raise.  The method minimises ``function . x``.

    Routing and launch grouping are ``solve_batch_cuts``'s.  Problems routed ``"single"``, and
    those of a launch whose blocks of Rmax + max_depth rows leave every batch kernel's envelope, go
    through ``SimplexMethod.solve_integer`` one by one; every other launch runs its trees on the
    device (``solve_batch_integer_arrays``), where ``max_nodes`` caps a launch's frontier.  Both
    walk the same tree by the same rules (``branch.Tree``)."""
    from .branch import IntegerSolution, mask_of
    problems = list(problems)
    _kernel_name(kernel)
    _lib.rule_code(rule)
    if integers is None:
        integers = [None] * len(problems)
    integers = list(integers)
    if len(integers) != len(problems):
        raise ValueError("integers must hold one entry per problem")
    P = int(max_pivots)
    Pw = P if warm_pivots is None else int(warm_pivots)
    results = [None] * len(problems)

    def single(k, c, f):
        try:
            results[k] = SimplexMethod(c, f).solve_integer(integers[k], P, Pw, max_depth,
                                                           max_nodes, int_tol, rule)
        except IndexError as exc:    # where the reference itself raises (simplex.py:49, 95, 159)
            results[k] = exc

    def launch(which, idx, tabs, dims):
        _, Rmax, ldb = tabs.shape
        try:
            warm_kernel(which, Rmax + int(max_depth), ldb)
        except ValueError:
            for k in idx:
                single(k, *problems[k])
            return
        mask = np.zeros((len(idx), ldb - 1), dtype=np.int32)
        for q, k in enumerate(idx):
            mask[q, :int(dims[q, 1])] = mask_of(integers[k], int(dims[q, 1]))
        out = solve_batch_integer_arrays(tabs, dims, mask, P, Pw, max_depth, max_nodes, int_tol,
                                         rule, which, device)
        for q, k in enumerate(idx):
            m = int(dims[q, 1])
            has = bool(out["found"][q])
            results[k] = IntegerSolution(
                out["status"][q], out["x"][q, :m].copy() if has else None,
                out["x_raw"][q, :m].copy() if has else None, float(out["objective"][q]),
                float(out["bound"][q]), int(out["nodes"][q]), int(out["warm_pivots"][q]),
                int(out["depth"][q]))

    _drive(problems, kernel, max_pivots, False, single, launch)
    return results


def _table(T, n, flen, m):
    rows = T[:n, :m + 1].tolist()
    rows.append(T[n, :min(flen, m + 1)].tolist())
    return rows


def _tables(S, n, flen, m):
    """All snapshots of one LP as Python lists in one conversion (f-row cut to len(function))."""
    tabs = S[:, :n + 1, :m + 1].tolist()
    if flen < m + 1:
        for t in tabs:
            t[n] = t[n][:flen]
    return tabs


def _assemble(problem, dims, final, rc, xv, snaps, status, np_, P):
    """Build the get_solution list (simplex.py:179-199) from the device outputs."""
    cons, func = problem
    n, m, flen = (int(v) for v in dims)
    row, col = _labels(n, m)
    f0, f1 = func[0], func[1]                                # simplex.py:48-49
    # snapshot #0 keeps the caller's values and types (simplex.py:181); rows of numbers, so a
    # row-wise copy is the deep copy
    res = [Info.owning(row, col, [list(r) for r in cons] + [list(func)], None, None, 0, 0, 0)]
    rcl = rc[:np_].tolist()
    xvl = xv[:np_].tolist()
    tables = _tables(snaps[:np_], n, flen, m) if snaps is not None else None
    x1 = x2 = 0
    for s in range(np_):
        r, c = rcl[s]
        if tables is not None or s == 0:
            res[-1].i, res[-1].j = r, c                      # simplex.py:194-195
        row[c], col[r] = col[r], row[c]                      # simplex.py:152
        x1 = xvl[s][0] if 'x1' in col else 0                 # simplex.py:51-68
        x2 = xvl[s][1] if 'x2' in col else 0
        if tables is not None:
            res.append(Info.owning(row, col, tables[s], None, None, x1, x2, f0 * x1 + f1 * x2))
    if tables is None:  # like SimplexMethod.solve(record_history=False): initial + final
        res.append(Info.owning(row, col, _table(final, n, flen, m), None, None, x1, x2,
                               f0 * x1 + f1 * x2))
    name = _status_name(status, np_, P)
    if name == "error":
        res.append(Error(MESSAGES[status]))
    return res, name
