"""``SimplexMethod`` / ``Info`` / ``Error`` -- the reference's solver surface, backed by HBM.

Mirrors ``/root/reference/src/simplex.py`` (jqnfxa/Simplex-Method-Solver @ 2025-06-20):
same constructor, attributes, method names, return tuples, snapshot objects and error
strings, so ``main.py:13`` (``from simplex import SimplexMethod, Error``) and
``table_widget.py:7`` (``from simplex import Info``) work unchanged through the ``simplex.py``
drop-in next to this package.  The tableau lives on the MI355X; every selection and every
pivot is a HIP kernel (``ops.py`` -> ``libsmx.so``).  On a machine with no HIP device at all (a
desktop running the reference UI's 2-variable LPs) the same library's host engine runs the
loop instead (``host.py``, ``backend == "host"``, bit-identical decisions and arithmetic); a
machine with an MI355X never takes it unless asked (``device="cpu"``).

Additions (not in the reference, all opt-in): ``step()`` (one pick + pivot), ``solve()``
(``get_solution`` with an optional pivot cap, or the chained no-history fast path),
``solution()`` (every variable, the duals and the objective of the current table),
``ranging()`` (how far each constant and each cost can move before the basis changes),
``solve_integer()`` (branch and bound with marked variables held to whole numbers),
``pivots`` / ``pivot_log`` and ``status``.

Deliberate differences, all on inputs the reference UI never produces (main.py:309-312 always
passes rectangular float rows and ``len(function) == m``):
* ragged constraint rows raise ``ValueError`` (the device tableau is dense);
* integer inputs are held as fp64 on the device.  The reference keeps them as Python ints until
  its first pivot, whose int arithmetic gives some zero results the opposite sign from fp64
  (-0 is the int 0; an int product 0 * -3 is +0): the first pivot of a table with int entries
  is followed by ``smx_int_first_fix`` (csrc/smx_intfirst.hpp), which rewrites exactly those
  zeros, so the tables match the reference's bits (tests/golden/intzero.json).  That holds
  while every int is below 2^26 in magnitude (products and differences exact in fp64); larger
  ints get a ``RuntimeWarning``: the reference computes their products exactly, fp64 rounds.
"""
from __future__ import annotations

import copy
import gc
from collections import namedtuple

import numpy as np

from . import _lib
from .basis import BasisTracker
from .device import DeviceTableau

MESSAGES = {_lib.INCORRECT: "incorrect system",                  # simplex.py:89
            _lib.NOT_CONVERGE: "simplex method does not converge"}  # simplex.py:139


# The whole answer of one LP (``SimplexMethod.solution()``, ``batch.solve_batch_solutions``).
# Labels are int32 codes: k in 0..m-1 is 'x{k+1}', m + i is 'y{i+1}'.  ``x`` [m]: the "-b" entry of
# the row labelled x{k+1}, else +0.0; ``duals`` [n]: the f-row entry of the column labelled
# y{i+1} (in the tableau's sign), else +0.0; ``objective``: function[0]*x[0] + ... summed left to
# right; ``basis`` [n] / ``nonbasis`` [m]: the labels of the rows / columns; ``pivots``: how many
# pivots led here.
Solution = namedtuple("Solution", "x duals objective basis nonbasis pivots")

# How far the data of one LP can move before its final basis changes (``SimplexMethod.ranging()``,
# ``batch.solve_batch_ranges``): adding d to the constant t_i of constraint i keeps the basis for
# ``rhs_lo[i] <= d <= rhs_hi[i]``, adding d to ``function[k]`` for ``cost_lo[k] <= d <=
# cost_hi[k]``.  numpy float64 arrays of [n], [n], [m], [m]; the rules are stated once, in
# include/smx.h (smx_batch_ranging).  At an optimum every lo <= 0 <= hi.
Ranging = namedtuple("Ranging", "rhs_lo rhs_hi cost_lo cost_hi")


class Scenario:
    """One what-if answer of ``batch.solve_batch_scenarios``: ``solution`` (a ``Solution``; its
    objective is formed on the scenario's own costs, its ``pivots`` count the run that gave it),
    ``status`` ("optimum", "error", "cap" or "exception") and ``warm`` -- True when the answer is
    the warm run's from the base LP's final table, False when it is a cold solve of the perturbed
    original."""
    __slots__ = ("solution", "status", "warm")

    def __init__(self, solution, status, warm):
        self.solution = solution
        self.status = status
        self.warm = warm

    def __repr__(self):
        return f"Scenario(status={self.status!r}, warm={self.warm!r}, solution={self.solution!r})"


def _label_code(label: str, m: int) -> int:
    return int(label[1:]) - 1 + (m if label[0] == 'y' else 0)


class Error:
    """simplex.py:4-9."""

    def __init__(self, error_string):
        self.error_string = error_string

    def __str__(self):
        return self.error_string


class Info:
    """simplex.py:12-21: one step snapshot (labels and table copied)."""

    def __init__(self, row, column, table, i, j, x1, x2, optimum):
        self.row = row.copy()
        self.column = column.copy()
        self.table = copy.deepcopy(table)
        self.i = i
        self.j = j
        self.x1 = x1
        self.x2 = x2
        self.optimum = optimum

    @classmethod
    def owning(cls, row, column, table, i, j, x1, x2, optimum):
        """The same snapshot for a table the caller just built and hands over (fresh lists of
        Python floats from the device download): labels are copied, the table is not
        deep-copied again -- the observable object is identical."""
        self = cls.__new__(cls)
        self.row = row.copy()
        self.column = column.copy()
        self.table = table
        self.i = i
        self.j = j
        self.x1 = x1
        self.x2 = x2
        self.optimum = optimum
        return self


class LazyInfo(Info):
    """An ``Info`` whose ``table`` is materialised on first access from the device history
    (checkpoint + replay of the logged pivots with the bit-identical update kernel), so a
    get_solution history of a large tableau costs O(pivots) host memory, not O(pivots x R x C)."""

    def __init__(self, row, column, history, step, i, j, x1, x2, optimum, table=None):
        self.row = row.copy()
        self.column = column.copy()
        self._history = history
        self._step = step
        self._table = table
        self.i = i
        self.j = j
        self.x1 = x1
        self.x2 = x2
        self.optimum = optimum

    @property
    def table(self):
        if self._table is None:
            self._table = self._history.table(self._step)
        return self._table

    @table.setter
    def table(self, value):
        self._table = value


class History:
    """Device checkpoints of the tableau every ``every`` pivots (within ``budget_bytes``) plus
    the host copy of the pivot log; ``table(step)`` replays from the nearest checkpoint."""

    def __init__(self, solver, every=256, budget_bytes=8 << 30):
        import torch
        self.sm = solver
        self.dev = solver._dev
        self.every = max(1, int(every))
        self.budget = budget_bytes
        self.ckpt = {}
        self.base = solver.pivots          # pivot count at the start of this history
        self._torch = torch
        self._scratch = None
        self.checkpoint(self.base)

    def _bytes(self):
        return sum(t.numel() * 8 for t in self.ckpt.values())

    def checkpoint(self, step):
        dev = self.dev
        if step in self.ckpt or (step - self.base) % self.every and step != self.base:
            return
        one = (dev.rows + 1) * dev.ld * 8
        if self.ckpt and self._bytes() + one > self.budget:
            return
        with self._torch.cuda.stream(dev.stream):
            self.ckpt[step] = dev.cur().clone()

    def checkpoint_now(self):
        """Checkpoint the current device table regardless of spacing (budget permitting)."""
        dev = self.dev
        step = self.sm.pivots
        one = (dev.rows + 1) * dev.ld * 8
        if step in self.ckpt or (self.ckpt and self._bytes() + one > self.budget):
            return
        with self._torch.cuda.stream(dev.stream):
            self.ckpt[step] = dev.cur().clone()

    def table(self, step):
        dev, torch = self.dev, self._torch
        s0 = max(k for k in self.ckpt if k <= step)
        log = self.sm.pivot_log
        with torch.cuda.stream(dev.stream):
            if self._scratch is None:
                self._scratch = torch.empty((2, dev.rows + 1, dev.ld), dtype=torch.float64,
                                            device=dev.device)
            sc = self._scratch
            sc[0].copy_(self.ckpt[s0])
            from . import ops
            ih = self.sm._int_hist
            for t in range(s0, step):
                a = (t - s0) & 1
                r, c = log[t]
                ops.update_forced(sc[a], sc[a ^ 1], dev.shape, r, c)
                if t == 0 and ih is not None:   # the caller's ints: their first pivot's zeros
                    from .device import int_first_fix
                    int_first_fix(sc[a], sc[a ^ 1], dev.C, ih[0], ih[1], ih[2])
            T = sc[(step - s0) & 1][:, :dev.C].cpu().numpy()
        rows = T[:self.sm.n].tolist()
        rows.append(T[self.sm.n, :min(self.sm.flen, self.sm.m + 1)].tolist())
        return rows


def _dense_from_lists(constraints, function, m):
    n = len(constraints)
    T = np.zeros((n + 1, m + 1), dtype=np.float64)
    if n:
        T[:n, :] = np.asarray(constraints, dtype=np.float64)
    k = min(len(function), m + 1)
    if k:
        T[n, :k] = np.asarray(function[:k], dtype=np.float64)
    return T


INT_EXACT = 1 << 26   # |int| below this: the first pivot's int products are exact in fp64


def _int_entries(constraints, function, m, dense):
    """Which tableau entries the caller passed as ints (Python ``int`` / ``bool``, numpy integer
    scalars or integer rows): None when none, True when all of them, else a uint8 mask
    ``[n + 1][m + 1]``."""
    rows = list(constraints) + [function]
    n = len(constraints)
    kinds = []
    for row in rows:
        if isinstance(row, np.ndarray):
            kinds.append(1 if row.dtype.kind in "iub" else 0)
            continue
        ts = set(map(type, row))
        ints = {t for t in ts if issubclass(t, (int, np.integer))}
        kinds.append(0 if not ints else (1 if ints == ts else 2))
    if not any(kinds):
        return None
    if all(k == 1 for k in kinds):   # (f-row padding is never an operand: int or not alike)
        mask = True
        big = float(np.abs(dense[:n + 1, :m + 1]).max(initial=0.0)) >= INT_EXACT
    else:
        mask = np.zeros((n + 1, m + 1), dtype=np.uint8)
        for i, (row, k) in enumerate(zip(rows, kinds)):
            if k == 1:
                mask[i, :min(len(row), m + 1)] = 1
            elif k == 2:
                mask[i, :min(len(row), m + 1)] = [isinstance(x, (int, np.integer))
                                                  for x in row[:m + 1]]
        big = float(np.abs(np.where(mask != 0, dense[:n + 1, :m + 1], 0.0)).max(initial=0.0)) \
            >= INT_EXACT
    if big:
        import warnings
        warnings.warn("simplex_mi355x: integer inputs of magnitude >= 2^26: the reference forms "
                      "their first-pivot products in exact integer arithmetic, this engine in "
                      "fp64 (the results may differ in the last bits)", RuntimeWarning,
                      stacklevel=3)
    return mask


def _use_host(device) -> bool:
    """The host engine runs a tableau only on request (``device="cpu"``) or when this machine has
    no HIP device at all -- then with a one-time ``RuntimeWarning``, and ``SimplexMethod.backend``
    reads "host"; with an MI355X present every tableau lives in HBM."""
    if device is not None:
        return str(device) == "cpu"
    import torch
    if torch.cuda.is_available():
        return False
    global _warned_host
    if not _warned_host:
        _warned_host = True
        import warnings
        warnings.warn("simplex_mi355x: no HIP device is visible, so SimplexMethod runs on the host "
                      "engine (backend == 'host'); pass device='cpu' to choose it explicitly",
                      RuntimeWarning, stacklevel=3)
    return True


_warned_host = False


class SimplexMethod:
    """simplex.py:24-199 on an MI355X-resident tableau (or, on a machine without one, on the
    host engine of the same library: ``backend == "host"``)."""

    def __init__(self, constraints, function, device=None, devices=None, pivots=None,
                 exchange=None):
        # simplex.py:26-33 (IndexError on an empty constraint list, like the reference)
        self.n = len(constraints)
        self.m = len(constraints[0]) - 1
        self.invalid_index = 1 + max(self.n, self.m)
        self.function = function
        self.row = ['x' + str(_) for _ in range(1, self.m + 1)]
        self.column = ['y' + str(_) for _ in range(1, self.n + 1)]
        self.row.append('-b')
        self.column.append('f')
        if any(len(c) != self.m + 1 for c in constraints):
            raise ValueError("ragged constraint rows: the device tableau is dense "
                             f"(every row must have m + 1 = {self.m + 1} entries)")
        # simplex.py:36-39: the caller's rows (and function) by reference, until the first pivot
        self._initial = [constraint for constraint in constraints]
        self._initial.append(function)
        self.flen = len(function)
        dense = _dense_from_lists(constraints, function, self.m)
        if devices is not None:
            # row sharding behind the same surface: rank p's rows on devices[p] (multi.py)
            from .multi import MultiTableau
            self._dev = MultiTableau(dense, self.n, self.m, self.flen, devices, pivots=pivots,
                                     exchange=exchange)
        elif _use_host(device):
            from .host import HostTableau
            self._dev = HostTableau(dense, self.n, self.m, self.flen)
        else:
            self._dev = DeviceTableau(dense, self.n, self.m, self.flen, device=device)
        self._pristine = True
        # int entries of the caller's table (None / True / mask): pending until the first pivot,
        # then kept with its (r, c) for history replays (_int_first_fix)
        self._int0 = _int_entries(constraints, function, self.m, dense)
        self._int_hist = None
        self.pivot_log: list[tuple[int, int]] = []
        self.status = "ready"
        self.cycle = None          # (first step of a repeated basis, period) when detected
        self._tracker = None

    @classmethod
    def from_file(cls, path, device=None):
        """Load a problem file: the reference UI's ``.txt`` (main.py:402-495; objective =
        gradient[:-1], main.py:312) or a binary ``.smx`` tableau streamed straight into HBM."""
        from . import problem_io
        if path.endswith(".smx"):
            dev = problem_io.load_device(path, device=device)
            return cls._from_device(dev)
        return cls(*problem_io.solver_inputs_txt(path), device=device)

    @classmethod
    def _from_device(cls, dev):
        """A SimplexMethod around an already-resident tableau (no host lists of the table)."""
        self = cls.__new__(cls)
        self.n, self.m, self.flen = dev.rows, dev.m, dev.flen
        self.invalid_index = 1 + max(self.n, self.m)
        with __import__("torch").cuda.stream(dev.stream):
            self.function = dev.buf[0, self.n, :min(dev.flen, dev.C)].cpu().tolist()
        self.row = ['x' + str(_) for _ in range(1, self.m + 1)] + ['-b']
        self.column = ['y' + str(_) for _ in range(1, self.n + 1)] + ['f']
        self._initial = None
        self._dev = dev
        self._pristine = False
        self._int0 = self._int_hist = None
        self.pivot_log = []
        self.status = "ready"
        self.cycle = None
        self._tracker = None
        return self

    # ---------------------------------------------------------------- state views --------
    @property
    def table(self):
        """The current tableau as the reference's list of lists (f-row has len(function))."""
        if self._pristine:
            return self._initial
        T = self._dev.download()
        rows = T[:self.n].tolist()
        rows.append(T[self.n, :min(self.flen, self.m + 1)].tolist())
        return rows

    def _snapshot(self, x1, x2, optimum) -> Info:
        """Info of the current state (simplex.py:181, :197-198).  A downloaded table is a fresh
        list of fresh floats, so it is handed over instead of deep-copied a second time; the
        pristine table (the caller's own lists) is deep-copied like the reference does."""
        if self._pristine:
            return Info(self.row, self.column, self.table, None, None, x1, x2, optimum)
        return Info.owning(self.row, self.column, self.table, None, None, x1, x2, optimum)

    @table.setter
    def table(self, value):
        cons, func = value[:-1], value[-1]
        if any(len(c) != self.m + 1 for c in cons) or len(cons) != self.n:
            raise ValueError("table shape does not match this problem")
        self._initial = list(value)
        self.flen = len(func)
        dense = _dense_from_lists(cons, func, self.m)
        self._dev.upload(dense)
        self._pristine = True
        self._int0 = _int_entries(cons, func, self.m, dense)
        self._int_hist = None

    @property
    def backend(self) -> str:
        """"hip" (the tableau is in HBM, every pivot a HIP kernel), "sharded" (row blocks on
        several devices, ``devices=[...]``) or "host" (no HIP device)."""
        if getattr(self._dev, "is_host", False):
            return "host"
        return "sharded" if hasattr(self._dev, "ranks") else "hip"

    @property
    def pivots(self) -> int:
        return len(self.pivot_log)

    def print_table(self):
        """simplex.py:41-46."""
        table = self.table
        print("\t", end='')
        print("\t".join(self.row))
        for row in range(self.n + 1):
            print(self.column[row], end='\t')
            print("\t".join([str(round(val, 6)) for val in table[row]]))

    def f(self, x1, x2):
        """simplex.py:48-49 (on the ORIGINAL objective list)."""
        return self.function[0] * x1 + self.function[1] * x2

    def _last_of_rows(self, rows):
        if self._pristine:
            return [self._initial[i][-1] for i in rows]
        last = [(i, self.m if i < self.n else min(self.flen, self.m + 1) - 1) for i in rows]
        return self._dev.values(last)

    def find_optimum(self) -> (float, float):
        """simplex.py:51-68."""
        def index_of(s):
            for row in range(len(self.column)):
                if self.column[row] == s:
                    return row
            return self.invalid_index

        x1_i = index_of('x1')
        x2_i = index_of('x2')
        want = [i for i in (x1_i, x2_i) if i != self.invalid_index]
        vals = dict(zip(want, self._last_of_rows(want)))
        x1 = vals[x1_i] if x1_i != self.invalid_index else 0
        x2 = vals[x2_i] if x2_i != self.invalid_index else 0
        return x1, x2

    def _label_codes(self):
        """``column`` / ``row`` as the int32 codes (basis [n], nonbasis [m]) of ``Solution``."""
        m = self.m
        return (np.array([_label_code(s, m) for s in self.column[:self.n]], dtype=np.int32),
                np.array([_label_code(s, m) for s in self.row[:m]], dtype=np.int32))

    def _dense_table(self):
        """The current table as a dense float64 (n + 1) x (m + 1) array: the backend's
        ``download()``, or before the first pivot the caller's own lists, where a short f-row
        reads as +0.0."""
        n, m = self.n, self.m
        if not self._pristine:
            return np.ascontiguousarray(self._dev.download()[:n + 1, :m + 1], dtype=np.float64)
        T = np.zeros((n + 1, m + 1), dtype=np.float64)
        T[:n] = self._initial[:n]
        frow = self._initial[n][:m + 1]
        T[n, :len(frow)] = frow
        return T

    def _successor(self, table, n, function, row, column, invalid_index, m=None, flen=None):
        """A new object on this one's backend around ``table`` ((n + 1) x (m + 1), already under
        the labels ``row`` / ``column``): past its first pivot, with an empty pivot log.  ``m`` and
        ``flen`` default to this object's."""
        m = self.m if m is None else m
        flen = self.flen if flen is None else flen
        new = type(self).__new__(type(self))
        new.n, new.m, new.flen = n, m, flen
        new.invalid_index = invalid_index
        new.function = function
        new.row, new.column = row, column
        new._initial = None
        old = self._dev
        if self.backend == "host":
            new._dev = type(old)(table, n, m, flen)
        elif self.backend == "sharded":
            new._dev = type(old)(table, n, m, flen, old.devices, pivots=old.P,
                                 exchange=old.exchange)
        else:
            new._dev = type(old)(table, n, m, flen, device=old.device)
        new._pristine = False
        new._int0 = new._int_hist = None
        new.pivot_log = []
        new.status = "ready"
        new.cycle = None
        new._tracker = None
        return new

    def solution(self) -> Solution:
        """The current table's whole answer: ``find_optimum`` for every variable, the f-row
        entries under the slack labels and the objective on the ORIGINAL function, with the
        labels as int32 codes (``Solution``).  Values are read whatever ``status`` says; on the
        caller's own table (before the first pivot) every x and dual is +0.0."""
        n, m = self.n, self.m
        basis, nonbasis = self._label_codes()
        rows = [i for i in range(n) if basis[i] < m]
        cols = [j for j in range(m) if nonbasis[j] >= m]
        if self._pristine:        # the caller's own lists (labels may stand from an earlier run)
            T = self._initial
            vals = [T[i][m] for i in rows] + [T[n][j] if j < len(T[n]) else 0.0 for j in cols]
        else:
            vals = self._dev.values([(i, m) for i in rows] + [(n, j) for j in cols])
        x = np.zeros(m, dtype=np.float64)
        duals = np.zeros(n, dtype=np.float64)
        if vals:
            x[basis[rows]] = vals[:len(rows)]
            duals[nonbasis[cols] - m] = vals[len(rows):]
        xs = x.tolist()
        objective = self.function[0] * xs[0]                 # each product rounded on its own,
        for k in range(1, m):                                # summed strictly left to right
            objective = objective + self.function[k] * xs[k]
        return Solution(x, duals, float(objective), basis, nonbasis, self.pivots)

    def ranging(self) -> Ranging:
        """The current table's sensitivity ranges (``Ranging``): for which change of a
        constraint's constant or of a cost the basis stays as it stands.  The labels come from
        ``row`` / ``column``, the table from the backend's ``download()`` (the caller's own lists
        before the first pivot), the rules from ``smx_host_ranging`` -- on every backend.  Values
        are formed whatever ``status`` says; they mean something at an optimum."""
        n, m = self.n, self.m
        basis, nonbasis = self._label_codes()
        T = self._dense_table()
        out = [np.empty(k, dtype=np.float64) for k in (n, n, m, m)]
        err = _lib.load().smx_host_ranging(T.ctypes.data, T.shape[1], n, m, basis.ctypes.data,
                                           nonbasis.ctypes.data, *(a.ctypes.data for a in out))
        if err:
            raise RuntimeError(f"smx_host_ranging refused n={n}, m={m} ({err})")
        return Ranging(*out)

    def what_if(self, drhs=None, dcost=None) -> "SimplexMethod":
        """A new ``SimplexMethod`` on the scenario table of the current one: ``drhs[i]`` added
        to the constant of constraint i and ``dcost[k]`` to ``function[k]`` of the ORIGINAL
        problem, re-expressed under the labels this table stands under (``None``: no change; a
        delta equal to zero is skipped).  The labels come from ``row`` / ``column``, the table
        from the backend's ``download()`` (the caller's own lists before the first pivot), the
        rule from ``smx_host_scenario`` (include/smx.h) -- on every backend, so on a sharded or
        16384 x 16384 tableau this is correct, not fast.  The result lives on the same backend:
        its ``row`` / ``column`` carry the labels, its ``function`` is the scenario's cost vector,
        its pivot log starts empty, and ``solve()``, ``solution()`` and ``ranging()`` carry on
        from there.  Under the default rule, which is no dual simplex, such a warm run need not
        terminate.  After a solve that ended at ``"optimum"`` and with ``dcost`` unchanged the
        table is dual feasible, and ``solve(rule="dual")`` terminates from it, up to degenerate
        cycling (include/smx.h, SMX_RULE_DUAL).  Either way cap the run with ``max_pivots`` and
        read ``status``."""
        n, m = self.n, self.m
        basis, nonbasis = self._label_codes()
        dr = np.zeros(n, dtype=np.float64)
        dc = np.zeros(m, dtype=np.float64)
        if drhs is not None:
            dr[:] = np.asarray(drhs, dtype=np.float64).reshape(n)
        if dcost is not None:
            dc[:] = np.asarray(dcost, dtype=np.float64).reshape(m)
        T = self._dense_table()
        func = np.zeros(m, dtype=np.float64)
        k = min(len(self.function), m)
        func[:k] = np.asarray(self.function[:k], dtype=np.float64)
        S = np.empty((n + 1, m + 1), dtype=np.float64)
        func_s = np.empty(m, dtype=np.float64)
        err = _lib.load().smx_host_scenario(
            T.ctypes.data, T.shape[1], n, m, basis.ctypes.data, nonbasis.ctypes.data,
            func.ctypes.data, dr.ctypes.data, dc.ctypes.data, S.ctypes.data, S.shape[1],
            func_s.ctypes.data)
        if err:
            raise RuntimeError(f"smx_host_scenario refused n={n}, m={m} ({err})")
        return self._successor(S, n, func_s.tolist() + [float(v) for v in self.function[m:]],
                               list(self.row), list(self.column), self.invalid_index)

    def add_constraints(self, rows) -> "SimplexMethod":
        """A new ``SimplexMethod`` on the extended table of the current one: every row of
        ``rows`` ([m coefficients, constant], the format of a constraint of the ORIGINAL problem)
        becomes one more constraint row under the labels this table stands under, the f-row moves
        below them.  The labels come from ``row`` / ``column``, the table from the backend's
        ``download()`` (the caller's own lists before the first pivot), the rule from
        ``smx_host_cuts`` (include/smx.h) -- on every backend, so this is correct everywhere and
        fast nowhere special.  The result lives on the same backend: ``column`` is extended by
        'y{n+1}'.., ``row`` and ``function`` are unchanged, its pivot log starts empty, and
        ``solve()``, ``solution()`` and ``ranging()`` carry on from there.  Under the default
        rule, which is no dual simplex, such a warm run need not terminate.  After a solve that
        ended at ``"optimum"`` the extended table is dual feasible, and ``solve(rule="dual")``
        terminates from it, up to degenerate cycling (include/smx.h, SMX_RULE_DUAL).  Either way
        cap the run with ``max_pivots`` and read ``status``."""
        n, m = self.n, self.m
        rows = [list(r) for r in rows]
        if any(len(r) != m + 1 for r in rows):
            raise ValueError(f"a new constraint must hold {m} coefficients and a constant")
        K = len(rows)
        G = np.ascontiguousarray(rows, dtype=np.float64).reshape(K, m + 1)
        basis, nonbasis = self._label_codes()
        T = self._dense_table()
        E = np.empty((n + K + 1, m + 1), dtype=np.float64)
        basis_out = np.empty(n + K, dtype=np.int32)
        err = _lib.load().smx_host_cuts(
            T.ctypes.data, T.shape[1], n, m, basis.ctypes.data, nonbasis.ctypes.data,
            G.ctypes.data if K else None, K, E.ctypes.data, E.shape[1], basis_out.ctypes.data)
        if err:
            raise RuntimeError(f"smx_host_cuts refused n={n}, m={m}, K={K} ({err})")
        column = (list(self.column[:n]) + ['y' + str(n + c + 1) for c in range(K)]
                  + list(self.column[n:]))
        return self._successor(E, n + K, list(self.function), list(self.row), column,
                               1 + max(n + K, m))

    def add_variables(self, cols) -> "SimplexMethod":
        """A new ``SimplexMethod`` on the widened table of the current one: every entry of
        ``cols`` ([n coefficients, cost]: the new variable's coefficient in every constraint of
        the ORIGINAL problem, then its entry in ``function``) becomes one more column under the
        labels this table stands under, the '-b' column moves to their right.  The labels come
        from ``row`` / ``column``, the table from the backend's ``download()`` (the caller's own
        lists before the first pivot), the rule from ``smx_host_cols`` (include/smx.h) -- on every
        backend, so this is correct everywhere and fast nowhere special.  The result lives on the
        same backend and has ``m + K`` variables: ``row`` is extended by 'x{m+1}'.. before '-b',
        ``function`` holds the costs inserted at position m, a slack keeps its name (its code
        moves up by K), its pivot log starts empty, and ``solve()``, ``solution()`` and
        ``ranging()`` carry on from there.  A new variable leaves every constant as it was, so
        after a solve that ended at ``"optimum"`` the widened table is primal feasible and the
        default rule carries on as an ordinary primal simplex; cap the run with ``max_pivots``
        and read ``status`` all the same."""
        n, m = self.n, self.m
        cols = [list(a) for a in cols]
        if any(len(a) != n + 1 for a in cols):
            raise ValueError(f"a new variable must hold {n} coefficients and a cost")
        if self.flen < m:        # a short f-row: its padding entries would become live costs
            raise ValueError("a problem whose function is shorter than m takes no new variables")
        K = len(cols)
        A = np.ascontiguousarray(cols, dtype=np.float64).reshape(K, n + 1)
        basis, nonbasis = self._label_codes()
        T = self._dense_table()
        W = np.empty((n + 1, m + K + 1), dtype=np.float64)
        basis_out = np.empty(n, dtype=np.int32)
        nonbasis_out = np.empty(m + K, dtype=np.int32)
        err = _lib.load().smx_host_cols(
            T.ctypes.data, T.shape[1], n, m, basis.ctypes.data, nonbasis.ctypes.data,
            A.ctypes.data if K else None, K, W.ctypes.data, W.shape[1], basis_out.ctypes.data,
            nonbasis_out.ctypes.data)
        if err:
            raise RuntimeError(f"smx_host_cols refused n={n}, m={m}, K={K} ({err})")
        row = (list(self.row[:m]) + ['x' + str(m + c + 1) for c in range(K)]
               + list(self.row[m:]))
        function = (list(self.function[:m]) + [float(a[n]) for a in cols]
                    + list(self.function[m:]))
        return self._successor(W, n, function, row, list(self.column), 1 + max(n, m + K),
                               m=m + K, flen=self.flen + K)

    def _branch_pick(self, mask, tol):
        """(bvar, brow, bval, bneg, bmin) of the current table under the mask ``mask`` [m] (int32):
        ``smx_host_branch_pick`` (include/smx.h) on the backend's ``download()``."""
        import ctypes
        basis, _ = self._label_codes()
        T = self._dense_table()
        bvar, brow = ctypes.c_int32(), ctypes.c_int32()
        bval, bneg, bmin = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        err = _lib.load().smx_host_branch_pick(
            T.ctypes.data, T.shape[1], self.n, self.m, basis.ctypes.data, mask.ctypes.data,
            float(tol), ctypes.byref(bvar), ctypes.byref(brow), ctypes.byref(bval),
            ctypes.byref(bneg), ctypes.byref(bmin))
        if err:
            raise RuntimeError(f"smx_host_branch_pick refused n={self.n}, m={self.m} ({err})")
        return bvar.value, brow.value, bval.value, bneg.value, bmin.value

    def _branch(self, p, snap=0.0):
        """The down and the up child of the current table branched on row ``p``
        (``smx_host_branch``, include/smx.h; ``snap`` is its tolerance), each a new object on this one's backend with one
        more constraint row 'y{n+1}', as ``add_constraints`` would leave it."""
        n, m = self.n, self.m
        basis, nonbasis = self._label_codes()
        T = self._dense_table()
        E = [np.empty((n + 2, m + 1), dtype=np.float64) for _ in range(2)]
        basis_out = np.empty(n + 1, dtype=np.int32)
        err = _lib.load().smx_host_branch(
            T.ctypes.data, T.shape[1], n, m, basis.ctypes.data, nonbasis.ctypes.data, int(p),
            float(snap), E[0].ctypes.data, E[1].ctypes.data, m + 1, basis_out.ctypes.data)
        if err:
            raise RuntimeError(f"smx_host_branch refused n={n}, m={m}, row {p} ({err})")
        column = list(self.column[:n]) + ['y' + str(n + 1)] + list(self.column[n:])
        return [self._successor(e, n + 1, list(self.function), list(self.row), list(column),
                                1 + max(n + 1, m)) for e in E]

    def solve_integer(self, integers=None, max_pivots=None, warm_pivots=None, max_depth=16,
                      max_nodes=None, int_tol=1e-6, rule="reference"):
        """Solve the problem with the variables marked in ``integers`` (None: all of them; else m
        truth values) held to whole numbers, by branch and bound; returns an
        ``IntegerSolution`` (branch.py).  The method minimises ``function . x``.

        The root is ``solve(record_history=False, max_pivots=max_pivots, rule=rule)`` on this
        object; only a root at ``"optimum"`` enters the tree, any other status is passed through.
        The tree is walked level by level with the rules of ``branch.Tree``, the same walk as
        ``batch.solve_batch_integer_arrays``: the pick is ``smx_host_branch_pick``, the children
        are ``smx_host_branch``'s tables (include/smx.h) as new objects on this one's backend, and
        each is solved by ``solve(rule="dual")`` capped at ``warm_pivots`` (default:
        ``max_pivots``) -- on every backend, so on the device and sharded backends this is
        correct, not fast.  A child that ends at "incorrect system" on a row that misses by more
        than ``int_tol`` is empty (``Tree.children``; a constant that misses zero from below by
        less is written to the children as zero); one that ends anywhere else but an optimum,
        a node at ``max_depth`` and what a frontier past ``max_nodes`` children leaves out stay
        open and make the status ``"limit"``.
        ``int_tol`` is how far from a whole number a marked variable may stand and count as whole:
        1e-6 is a convention of LP-based integer solvers, not a measured number."""
        from . import branch
        _lib.rule_code(rule)
        mask = branch.mask_of(integers, self.m)
        Pw = max_pivots if warm_pivots is None else warm_pivots
        if max_nodes is None:
            max_nodes = branch.default_max_nodes(self.n + 1 + int(max_depth), self.m + 1)
        tree = branch.Tree(1, max_depth, max_nodes, int_tol)
        self.solve(record_history=False, max_pivots=max_pivots, rule=rule)
        function = list(self.function)
        frontier, nodes, level = [], [self], 0
        if tree.start([self.status]):
            frontier = [(0, 0, self.solution().objective)]
        codes = {"optimum": _lib.OPTIMUM, "cap": _lib.PIVOT}
        codes.update({text: code for code, text in MESSAGES.items()})
        picks = [self._branch_pick(mask, int_tol)] if frontier else []
        while frontier:
            parents = tree.close(level, frontier, [v[0] for v in picks],
                                 lambda qs: [nodes[q].solution().x for q in qs])
            if not parents:
                break
            level += 1
            kids, status = [], []
            for q, _, _ in parents:
                for child in nodes[q]._branch(picks[q][1], int_tol):
                    out = child.solve(record_history=False, max_pivots=Pw, rule="dual")
                    kids.append(child)
                    status.append(codes[str(out[-1]) if child.status == "error" else child.status])
            nodes = kids
            picks = [c._branch_pick(mask, int_tol) for c in kids]
            frontier = tree.children(level, parents, status, [c.pivots for c in kids],
                                     [c.solution().objective for c in kids],
                                     [v[3] for v in picks], [v[4] for v in picks])
        return tree.answer(0, function, mask)

    # ---------------------------------------------------------------- the hot path -------
    def _rule_twin(self):
        """A host tableau holding the current table: where a backend's own selection takes no
        rule (device, sharded), the host twins of include/smx.h decide and pivot on it and the
        result is uploaded again -- correct, not fast, as ``what_if`` is."""
        from .host import HostTableau
        return HostTableau(self._dense_table(), self.n, self.m, self.flen)

    def pick_element(self, rule="reference") -> (bool, int, int, float):
        """simplex.py:70-141: selection kernels on the device, outcome mapped to the
        reference's return tuple / ValueError.  ``rule="dual"`` decides by SMX_RULE_DUAL
        (include/smx.h): natively on the host backend, on a host copy of the table elsewhere."""
        code = _lib.rule_code(rule)
        self._twin = None
        if code == _lib.RULE_REFERENCE:
            status, r, c, e = self._dev.pick()
        elif self.backend == "host":
            status, r, c, e = self._dev.pick(code)
        else:
            self._twin = self._rule_twin()
            status, r, c, e = self._twin.pick(code)
        if status == _lib.PIVOT:
            if self._pristine:
                e = self._initial[r][c]
            return True, r, c, e
        if status == _lib.OPTIMUM:
            x1, x2 = self.find_optimum()
            return False, x1, x2, self.f(x1, x2)
        if status in MESSAGES:
            raise ValueError(MESSAGES[status])
        if status == _lib.FSHORT:
            # the reference indexes function[idx] past its end (simplex.py:95-96)
            raise IndexError("list index out of range")
        raise RuntimeError(f"unexpected selection status {status}")

    def _apply(self, r, c):
        """The part of recalculate_matrix after its pick_element (simplex.py:149-177)."""
        self.row[c], self.column[r] = self.column[r], self.row[c]   # simplex.py:152
        if self.flen > self.m + 1 or (self.flen < self.m and c >= self.flen):
            # the reference's step 2 / step 4 index the f-row out of range (simplex.py:159-175)
            raise IndexError("list index out of range")
        first_int = self._pristine and self._int0 is not None
        twin = getattr(self, "_twin", None)
        if twin is not None:       # the pick came from the host twin: pivot there, then upload
            twin.apply_selected()
            if first_int:
                self._int_first_fix(r, c, twin)
            self._dev.upload(twin.download())
            self._twin = None
        else:
            self._dev.apply_selected()
            if first_int:
                self._int_first_fix(r, c)
        self._pristine = False
        self.pivot_log.append((r, c))

    def _int_first_fix(self, r, c, dev=None):
        """The first pivot of a table with int entries just ran (r, c) on ``dev`` (default: this
        object's tableau): give its zero results the signs the reference's int arithmetic gives
        them (smx_int_first_fix)."""
        mask = None if self._int0 is True else self._int0
        (self._dev if dev is None else dev).int_first_fix(mask, r, c)
        self._int_hist = (mask, r, c)
        self._int0 = None

    def _int_first_after_run(self, before, done, dev=None):
        """After a chained run that began at the caller's table: the int fix of its first pivot
        (the chained loops run that pivot alone while one is pending).  True when applied."""
        if self._int0 is None or before != 0 or done < 1 or not self._pristine:
            return False
        r, c = (int(x) for x in (self._dev if dev is None else dev).read_log(0, 1)[0])
        self._int_first_fix(r, c, dev)
        return True

    def recalculate_matrix(self):
        """simplex.py:143-177."""
        _is_successful, r, c, _ = self.pick_element()
        if not _is_successful:
            return
        self._apply(r, c)

    def _track(self, r, c, detect_cycles):
        """Feed a pivot to the opt-in cycle detector; True when the basis has repeated."""
        if not detect_cycles:
            return False
        if self._tracker is None:
            self._tracker = BasisTracker(self.n, self.m)
            for rr, cc in self.pivot_log[:-1]:
                self._tracker.pivot(rr, cc)
        if self._tracker.pivot(r, c) is not None:
            self.cycle = self._tracker.cycle
            return True
        return False

    LAZY_ELEMENTS = 1 << 20   # above this many tableau entries get_solution snapshots lazily

    def get_solution(self, max_pivots=None, detect_cycles=False, lazy=None, chunk=256,
                     rule="reference"):
        """simplex.py:179-199.  Opt-in additions (defaults = the reference's behaviour):
        ``max_pivots`` bounds the loop (the list ends, ``status == 'cap'``); ``detect_cycles``
        ends it when the basis repeats (``status == 'cycle'``, ``self.cycle``).  ``lazy``
        (default: automatic above ``LAZY_ELEMENTS`` entries) runs the chained device loop and
        returns ``LazyInfo`` snapshots whose tables are materialised on access.  ``rule``
        selects the selection rule of every step (``pick_element``); ``"dual"`` runs step by step."""
        code = _lib.rule_code(rule)
        if lazy is None:
            lazy = (self.n + 1) * (self.m + 1) > self.LAZY_ELEMENTS
        lazy = lazy and self.backend != "host"   # device checkpoints + replay need a device
        lazy = lazy and code == _lib.RULE_REFERENCE
        if lazy and self.flen in (self.m, self.m + 1) and self.flen >= 2:
            return self._get_solution_lazy(max_pivots, detect_cycles, chunk)
        # every snapshot is a fresh acyclic list of lists: pause the cyclic collector so its
        # passes do not rescan the growing history (the reference pays that; the result is equal)
        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            return self._get_solution_eager(max_pivots, detect_cycles, rule)
        finally:
            if gc_was_on:
                gc.enable()

    def _get_solution_eager(self, max_pivots, detect_cycles, rule="reference"):
        result = []
        result.append(self._snapshot(0, 0, 0))
        done = 0
        while True:
            try:
                is_successful, i, j, e = self.pick_element(rule)
            except ValueError as exc:
                result.append(Error(str(exc)))
                self.status = "error"
                return result
            if not is_successful:
                self.status = "optimum"
                break
            if max_pivots is not None and done >= max_pivots:
                self.status = "cap"
                break
            result[-1].i = i
            result[-1].j = j
            self._apply(i, j)   # recalculate_matrix() without re-running the selection
            done += 1
            x1, x2 = self.find_optimum()
            result.append(self._snapshot(x1, x2, self.f(x1, x2)))
            if self._track(i, j, detect_cycles):
                self.status = "cycle"
                break
        return result

    def _get_solution_lazy(self, max_pivots, detect_cycles, chunk):
        """get_solution's loop (simplex.py:184-198) chained on the device; the (i, j) of every
        step and its (x1, x2) come from the device rings, tables from History on demand."""
        hist = History(self, every=chunk)
        first = LazyInfo(self.row, self.column, hist, self.pivots, None, None, 0, 0, 0,
                         table=copy.deepcopy(self.table) if self._pristine else None)
        result = [first]
        dev = self._dev
        budget = float("inf") if max_pivots is None else int(max_pivots)
        start = self.pivots
        status = None
        while self.pivots - start < budget:
            # chunks end on multiples of `chunk` from the history's base, where hist.checkpoint
            # keeps a table: after an int table's lone first pivot the next chunk is one shorter,
            # so the later checkpoints are taken (else every replay starts at step 0)
            k = chunk - (self.pivots - start) % chunk
            k = int(min(k, budget - (self.pivots - start), dev.log_cap))
            if self._int0 is not None and self._pristine:
                k = 1                      # the first pivot of an int table runs alone
            before = dev.step
            dev.run(k, graph=(k == chunk))
            ctl = dev.sync_state()
            done = int(ctl["npivots"])
            fixed = self._int_first_after_run(before, done)
            logs = dev.read_log(before, done)
            xs = dev.read_xhist(before, done)
            cycled = False
            for (r, c), (v1, v2) in zip(logs, xs):
                r, c = int(r), int(c)
                result[-1].i, result[-1].j = r, c
                self.row[c], self.column[r] = self.column[r], self.row[c]   # simplex.py:152
                self.pivot_log.append((r, c))
                self._pristine = False
                if fixed:                  # the ring holds the pre-fix values of pivot 0
                    x1, x2 = self.find_optimum()
                    fixed = False
                else:
                    x1 = float(v1) if 'x1' in self.column else 0            # simplex.py:51-68
                    x2 = float(v2) if 'x2' in self.column else 0
                result.append(LazyInfo(self.row, self.column, hist, self.pivots, None, None,
                                       x1, x2, self.f(x1, x2)))
                cycled = self._track(r, c, detect_cycles) or cycled   # stop after this chunk
            hist.checkpoint(self.pivots)
            if cycled:
                status = "cycle"
                break
            if ctl["term"]:
                status = int(ctl["sel_status"])
                break
        if status is None:
            self.status = "cap"
        elif status == "cycle":
            self.status = "cycle"
        elif status == _lib.OPTIMUM:
            self.status = "optimum"
        elif status in MESSAGES:
            self.status = "error"
            result.append(Error(MESSAGES[status]))
        return result

    # ---------------------------------------------------------------- additions ----------
    def step(self, rule="reference"):
        """One pick + pivot under ``rule``; returns pick_element's tuple (raises like it)."""
        res = self.pick_element(rule)
        if res[0]:
            self._apply(res[1], res[2])
        return res

    def solve(self, record_history=True, max_pivots=None, chunk=256, graph=True,
              detect_cycles=False, rule="reference"):
        """``get_solution`` (record_history=True) or the chained fast path: pivots run on the
        device in chunks of ``chunk`` with no host synchronisation inside a chunk; returns
        ``[Info(initial, i/j of the first pivot), Info(final)]`` plus a trailing ``Error``.
        ``detect_cycles`` stops at the end of the chunk in which the basis first repeats.

        ``rule``: ``"reference"`` (the default: the reference's pick_element) or ``"dual"``
        (SMX_RULE_DUAL of include/smx.h: from a table with negative constants and no negative
        f-row entry, as ``what_if(drhs)`` and ``add_constraints`` leave after an optimum, every
        step is a dual-simplex step and the run terminates, up to degenerate cycling; anywhere
        else a step is the reference's).  On the host backend the chain is the library's host
        twin with the same chunk protocol (a pristine int table still runs its first pivot
        alone).  On the device and sharded backends ``"dual"`` is correct, not fast, as
        ``what_if`` and ``add_constraints`` are: the table comes down, the host twin runs the
        chain and the result is uploaded again.  ``pivots``, ``pivot_log``, ``row`` / ``column``,
        ``status``, ``solution()`` and ``ranging()`` are right afterwards on every backend.  An
        unknown rule raises ValueError."""
        code = _lib.rule_code(rule)
        if record_history:
            return self.get_solution(max_pivots=max_pivots, detect_cycles=detect_cycles,
                                     rule=rule)
        if self.flen not in (self.m, self.m + 1) or self.flen < 2:
            return self._solve_stepwise(max_pivots, detect_cycles, rule)
        twin = code != _lib.RULE_REFERENCE and self.backend != "host"
        big = ((self.n + 1) * (self.m + 1) > self.LAZY_ELEMENTS and self.backend != "host"
               and not twin)
        hist = History(self, every=1 << 62) if big else None    # one checkpoint: the start
        if big:
            first = LazyInfo(self.row, self.column, hist, self.pivots, None, None, 0, 0, 0)
        else:
            first = self._snapshot(0, 0, 0)
        start = self.pivots
        budget = float("inf") if max_pivots is None else int(max_pivots)
        dev = self._rule_twin() if twin else self._dev
        status = None
        while self.pivots - start < budget:
            k = int(min(chunk, budget - (self.pivots - start), dev.log_cap))
            if self._int0 is not None and self._pristine:
                k = 1                      # the first pivot of an int table runs alone
            before = dev.step
            if code == _lib.RULE_REFERENCE:
                dev.run(k, graph=graph and k == chunk)
            else:
                dev.run(k, rule=code)
            ctl = dev.sync_state()
            done = int(ctl["npivots"])
            self._int_first_after_run(before, done, dev)
            cycled = False
            for r, c in dev.read_log(before, done):
                r, c = int(r), int(c)
                self.row[c], self.column[r] = self.column[r], self.row[c]
                self.pivot_log.append((r, c))
                cycled = self._track(r, c, detect_cycles) or cycled
            if done > 0:
                self._pristine = False
            if ctl["term"]:
                status = int(ctl["sel_status"])
                break
            if cycled:
                status = "cycle"
                break
        if twin and self.pivots > start:     # the twin's final table goes back to the backend
            self._dev.upload(dev.download())
        out = [first]
        if self.pivots > start:
            first.i, first.j = self.pivot_log[start]
        x1, x2 = self.find_optimum()
        if big:   # the final table is the current device table: materialise it on access
            hist.checkpoint_now()
            out.append(LazyInfo(self.row, self.column, hist, self.pivots, None, None, x1, x2,
                                self.f(x1, x2)))
        else:
            out.append(self._snapshot(x1, x2, self.f(x1, x2)))
        if status is None:
            self.status = "cap"
        elif status == "cycle":
            self.status = "cycle"
        elif status == _lib.OPTIMUM:
            self.status = "optimum"
        elif status in MESSAGES:
            self.status = "error"
            out.append(Error(MESSAGES[status]))
        else:
            raise RuntimeError(f"unexpected terminal status {status}")
        return out

    def _solve_stepwise(self, max_pivots, detect_cycles=False, rule="reference"):
        first = self._snapshot(0, 0, 0)
        out = [first]
        done = 0
        while max_pivots is None or done < max_pivots:
            try:
                ok, i, j, _ = self.pick_element(rule)
            except ValueError as exc:
                x1, x2 = self.find_optimum()
                out.append(self._snapshot(x1, x2, self.f(x1, x2)))
                out.append(Error(str(exc)))
                self.status = "error"
                return out
            if not ok:
                break
            if done == 0:
                first.i, first.j = i, j
            self._apply(i, j)
            done += 1
            if self._track(i, j, detect_cycles):
                break
        if self.cycle is not None and detect_cycles:
            self.status = "cycle"
        else:
            self.status = "optimum" if (max_pivots is None or done < max_pivots) else "cap"
        x1, x2 = self.find_optimum()
        out.append(self._snapshot(x1, x2, self.f(x1, x2)))
        return out
