"""Branch and bound over solved LPs: the bookkeeping of the tree, stated once.

``SimplexMethod.solve_integer`` (one problem, nodes on the host twins) and
``batch.solve_batch_integer_arrays`` (a launch of problems, nodes in device buffers) walk the same
tree level by level: ``Tree`` is everything they share -- which node becomes an incumbent, which is
pruned, which is expanded, which stays open -- so that both report the same statuses and counts.
What a node is, the pick and the children are the contract of include/smx.h (smx_batch_branch*).

The method minimises ``function . x`` (it stops where no f-row entry is negative), so a node whose
objective is not BELOW its problem's incumbent cannot improve it and is pruned; a child's
objective is never below its parent's.
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np

from . import _lib

# What ``solve_integer`` answers for one problem.  ``status``: "optimal" (every node was closed and
# an integral one was found), "infeasible" (every node was closed, none integral), "limit" (a node
# could be neither closed nor expanded) or the root LP's own status ("error", "cap"); ``x`` [m]:
# the best integral answer with the marked variables rounded to the nearest whole number (None
# without one), ``x_raw`` as the table gave it; ``objective``: function[0]*x[0] + ... on the
# rounded ``x``, summed left to right (+inf without an answer); ``bound``: no integral answer has
# an objective below it (the objective when "optimal", +inf when "infeasible"); ``nodes``: LPs
# solved, the root included; ``warm_pivots``: the pivots of all but the root; ``depth``: the
# deepest level a node was solved at.
IntegerSolution = namedtuple("IntegerSolution",
                             "status x x_raw objective bound nodes warm_pivots depth")

INT_TOL = 1e-6       # a convention of LP-based integer solvers, not a measured number


def default_max_nodes(rows: int, cols: int, budget: int = 1 << 30) -> int:
    """``max_nodes`` by default: the children of one level whose tables of ``rows`` x ``cols``
    doubles fit, beside their parents', under ``budget`` bytes (batch.GM_TABLE_BUDGET)."""
    return max(2, int(budget) // (2 * max(1, int(rows) * int(cols) * 8)))


def mask_of(integers, m: int) -> np.ndarray:
    """``integers`` (None: every variable; else m truth values) as the int32 mask of the pick."""
    if integers is None:
        return np.ones(m, dtype=np.int32)
    mask = (np.asarray(integers).reshape(-1) != 0).astype(np.int32)
    if mask.shape != (m,):
        raise ValueError(f"integers must hold one entry per variable ({m})")
    return mask


def ordered_objective(function, x) -> float:
    """function[0]*x[0] + function[1]*x[1] + ..., each product rounded on its own, summed strictly
    left to right: smx_batch_solution's sum."""
    xs = [float(v) for v in x]
    objective = float(function[0]) * xs[0]
    for k in range(1, len(xs)):
        objective = objective + float(function[k]) * xs[k]
    return float(objective)


class Tree:
    """The trees of ``count`` problems, walked level by level.  A node is known here by its index
    in the current level's buffers, its problem and its objective; the caller solves, picks and
    branches."""

    def __init__(self, count: int, max_depth: int, max_nodes: int, int_tol: float = INT_TOL):
        self.tol = float(int_tol)
        self.max_depth = int(max_depth)
        self.max_nodes = int(max_nodes)
        self.inc_obj = [math.inf] * count
        self.inc_x = [None] * count
        self.open = [[] for _ in range(count)]              # objectives of nodes left open
        self.root = [None] * count                           # a root status that ends the problem
        self.nodes = [0] * count
        self.warm = [0] * count
        self.depth = [0] * count

    def start(self, statuses):
        """The roots: ``statuses[k]`` is "optimum" or the name that ends problem k.  Returns the
        problems that enter the tree."""
        live = []
        for k, name in enumerate(statuses):
            self.nodes[k] = 1
            if name == "optimum":
                live.append(k)
            else:
                self.root[k] = name
        return live

    def close(self, level, frontier, bvar, fetch_x):
        """One level's host step.  ``frontier``: [(node, problem, objective)] of the nodes at an
        optimum; ``bvar[node]`` the pick's; ``fetch_x(nodes)`` the x rows of the named nodes.
        Updates the incumbents, then returns the nodes to expand as [(node, problem, objective)]
        in node order; what can be neither closed nor expanded is left open."""
        best = {}
        for q, k, obj in frontier:
            if bvar[q] < 0 and obj < self.inc_obj[k]:
                self.inc_obj[k] = obj
                best[k] = q
        if best:
            ks = sorted(best)
            for k, x in zip(ks, fetch_x([best[k] for k in ks])):
                self.inc_x[k] = np.array(x, dtype=np.float64)
        expand = []
        for q, k, obj in frontier:
            if bvar[q] < 0:
                continue
            if obj != obj:                                   # a NaN objective bounds nothing
                self.open[k].append(-math.inf)
            elif obj < self.inc_obj[k]:
                expand.append((q, k, obj))
        if level >= self.max_depth:
            keep, rest = [], expand
        else:
            order = sorted(expand, key=lambda e: (e[2], e[0]))
            keep, rest = order[:self.max_nodes // 2], order[self.max_nodes // 2:]
        for _, k, obj in rest:
            self.open[k].append(obj)
        return sorted(keep)

    def children(self, level, parents, status, npivots, objective, bneg, bmin):
        """The children of ``parents`` (``close``'s result) solved at ``level``: child 2i and
        2i + 1 belong to parents[i]; ``bneg`` / ``bmin`` are the pick's on the children's final
        tables.  Returns the next frontier.

        The kernels compare with zero exactly, and a constant that is zero in exact arithmetic can
        stand at -1e-16 after a few pivots, so SMX_INCORRECT alone is no proof in floating point.
        It is one where the row behind it misses by more than the tolerance (``bneg`` below
        ``-int_tol``): the child is empty.  Where no row at all misses by more than the tolerance
        (``bmin``) the table is feasible within it and, having stayed dual feasible, is read as
        an optimum.  Anything between stays open."""
        frontier = []
        for c in range(2 * len(parents)):
            _, k, pobj = parents[c // 2]
            self.nodes[k] += 1
            self.warm[k] += int(npivots[c])
            self.depth[k] = max(self.depth[k], level)
            st = int(status[c])
            if st == _lib.INCORRECT:
                if bneg[c] < -self.tol:                      # from a dual-feasible table: empty
                    continue
                if bmin[c] >= -self.tol:
                    st = _lib.OPTIMUM
            if st == _lib.OPTIMUM:
                frontier.append((c, k, float(objective[c])))
            else:                # a capped or failed warm run: the parent's objective still bounds it
                self.open[k].append(pobj)
        return frontier

    def answer(self, k, function, mask) -> IntegerSolution:
        counts = (self.nodes[k], self.warm[k], self.depth[k])
        if self.root[k] is not None:
            return IntegerSolution(self.root[k], None, None, math.inf, -math.inf, *counts)
        x_raw = self.inc_x[k]
        x = objective = None
        if x_raw is not None:
            m = len(mask)
            x = x_raw[:m].copy()
            x[mask != 0] = np.rint(x[mask != 0])
            x_raw = x_raw[:m].copy()
            objective = ordered_objective(function, x)
        if self.open[k]:
            bound = min(self.open[k])
            if objective is not None:
                bound = min(bound, objective)
            return IntegerSolution("limit", x, x_raw, math.inf if x is None else objective,
                                   bound, *counts)
        if x is None:
            return IntegerSolution("infeasible", None, None, math.inf, math.inf, *counts)
        return IntegerSolution("optimal", x, x_raw, objective, objective, *counts)
