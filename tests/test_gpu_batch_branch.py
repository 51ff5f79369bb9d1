"""GPU: branch and bound on the device -- k_batch_branch_pick and k_batch_branch alone through the
C ABI at their wave, workgroup and envelope edges, on the hand-made columns and on degenerate
inputs, against branch_util's restatement (the pick) and cuts_util's (the children); the chain two
levels deep on and across all three tiers against the dual rule's restatement on the restated
tables; solve_batch_integer against SimplexMethod.solve_integer() on the host engine; and
solve_integer() on the device backend.  Everything compares by bit pattern."""
from __future__ import annotations

import numpy as np
import pytest

import branch_util as bu
import cuts_util as cu
import dual_util as du
import ranging_util as ru
import solution_util as su
from batch_util import case

pytestmark = pytest.mark.gpu

GUARD = 64


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def _guarded(torch, count, dtype, poison):
    """A device buffer of `count` elements between two poisoned guard bands -> (whole, view)."""
    whole = torch.full((count + 2 * GUARD,), poison, dtype=dtype, device="cuda")
    return whole, whole[GUARD:GUARD + count]


def _guards_intact(pairs):
    for whole, poison in pairs:
        h = whole.cpu().numpy()
        assert (h[:GUARD] == poison).all() and (h[-GUARD:] == poison).all(), "guard band"


def _pack(nodes, Rmax, ldb):
    """nodes: [(T, n, m, basis, nonbasis)], or None for a node whose dims (Rmax, ldb) lie outside
    the block -> host arrays final, dims, basis, nonbasis, func with padding that would show."""
    Q = len(nodes)
    final = np.full((Q, Rmax, ldb), 3.25)
    dims = np.zeros((Q, 3), dtype=np.int32)
    ba = np.full((Q, Rmax), 7, dtype=np.int32)
    nb = np.full((Q, ldb), 7, dtype=np.int32)
    func = np.arange(Q * ldb, dtype=np.float64).reshape(Q, ldb) + 0.5
    for q, node in enumerate(nodes):
        if node is None:
            dims[q] = (Rmax, ldb, ldb)
            continue
        T, n, m, basis, nonbasis = node
        final[q, :n + 1, :m + 1] = np.asarray(T)[:n + 1, :m + 1]
        dims[q] = (n, m, m)
        ba[q, :n], nb[q, :m] = basis, nonbasis
    return final, dims, ba, nb, func


# ----------------------------------------------------------------------------------------------
# the pick alone
def _pick_launch(nodes, Rmax, ldb, ints, lp, tol):
    """One smx_batch_branch_pick launch; `ints` [B][m...] rows are padded to ldb with ones that
    must not be read past m, `lp` [Q].  Every output is compared with branch_util.pick, between
    poisoned guard bands.  Returns (bvar, brow, bval, bneg, bmin)."""
    import torch
    from simplex_mi355x import _lib
    Q, B = len(nodes), len(ints)
    final, dims, ba, _, _ = _pack(nodes, Rmax, ldb)
    h_ints = np.ones((B, ldb), dtype=np.int32)
    for b, row in enumerate(ints):
        h_ints[b, :len(row)] = row
    h_lp = np.asarray(lp, dtype=np.int32)
    d_in = [torch.from_numpy(a).to("cuda") for a in (final, dims, ba, h_ints, h_lp)]
    outs = [_guarded(torch, Q, torch.int32, 77), _guarded(torch, Q, torch.int32, 77),
            _guarded(torch, Q, torch.float64, 7.0), _guarded(torch, Q, torch.float64, 7.0),
            _guarded(torch, Q, torch.float64, 7.0)]
    _lib.check(_lib.load().smx_batch_branch_pick(
        d_in[0].data_ptr(), d_in[1].data_ptr(), Q, Rmax, ldb, d_in[2].data_ptr(),
        d_in[3].data_ptr(), B, d_in[4].data_ptr(), float(tol), *(v.data_ptr() for _, v in outs),
        torch.cuda.current_stream().cuda_stream), "smx_batch_branch_pick")
    _guards_intact(zip((w for w, _ in outs), (77, 77, 7.0, 7.0, 7.0)))
    got = [v.cpu().numpy() for _, v in outs]
    for q, node in enumerate(nodes):
        mine = tuple(a[q].item() for a in got)
        if node is None or not 0 <= h_lp[q] < B:
            exp = (-1, -1, 0.0, 0.0, 0.0)
        else:
            T, n, m, basis, _ = node
            exp = bu.pick(T, n, m, basis, h_ints[h_lp[q]], tol)
        bu.same_pick(mine, exp, (q, Rmax, ldb))
    return got


SHAPES = [(63, 63), (64, 64), (65, 65), (5, 255), (5, 256), (5, 257), (257, 3), (1, 1),
          (1, 8000), (8000, 1)]


def _seeded(n, m, seed):
    from simplex_mi355x import lp
    T = lp.dense_tableau("uniform", seed, n, m)
    basis, nonbasis = ru.seeded_labels(n, m, seed)
    return T, n, m, basis, nonbasis


@pytest.mark.parametrize("n,m", SHAPES, ids=[f"{n}x{m}" for n, m in SHAPES])
def test_pick_at_wave_and_envelope_edges(n, m):
    """Five seeded nodes under seeded label permutations (more than one workgroup of four waves),
    two masks, tight blocks and blocks with padding."""
    nodes = [_seeded(n, m, 3 + q) for q in range(5)]
    g = np.random.default_rng([n, m])
    ints = [(g.random(m) < 0.7).astype(np.int32), np.ones(m, dtype=np.int32)]
    wide = n + m + 8 <= 8192
    got = _pick_launch(nodes, n + 1 + wide, m + 1 + 2 * wide, ints, [0, 1, 0, 1, 1], bu.TOL)
    assert (got[0] >= 0).any() or m == 1 or n == 1
    _pick_launch(nodes, n + 1, m + 1, ints, [1, 1, 0, 0, 1], 0.0)


def test_pick_reduces_across_the_wavefront_and_past_row_256():
    """Whole constants everywhere but three rows: the winner sits past the first wavefront's 64
    rows and past row 256; then a tie at .5 whose lower code sits in the later row."""
    n, m = 300, 320
    T = np.ones((n + 1, m + 1))
    T[:n, m] = np.arange(n) + 2.0
    basis = np.arange(n, dtype=np.int32)                     # x1..x300 on the rows
    nonbasis = np.arange(n, n + m, dtype=np.int32)
    T[5, m], T[70, m], T[290, m] = 2.125, 9.25, 3.5
    tie = T.copy()
    tie_basis = basis.copy()
    tie[5, m], tie[70, m], tie[290, m] = 7.5, 4.0, 1.5
    tie_basis[5], tie_basis[290] = 290, 5                    # the lower code in the later row
    got = _pick_launch([(T, n, m, basis, nonbasis), (tie, n, m, tie_basis, nonbasis)], n + 1,
                       m + 1, [np.ones(m, dtype=np.int32)], [0, 0], bu.TOL)
    assert (got[0][0], got[1][0], got[2][0]) == (290, 290, 3.5)
    assert (got[0][1], got[1][1], got[2][1]) == (5, 290, 1.5)


HANDMADE = bu.handmade()


@pytest.mark.parametrize("hm", HANDMADE, ids=[c[0] for c in HANDMADE])
def test_handmade_columns_on_the_device(hm):
    """Each hand-made column as nodes 0, 1 and 4 of a five-node launch; node 2 has dims outside
    the block, node 3 names a problem outside 0..B-1."""
    name, T, n, m, basis, ints, tol, pin = hm
    nonbasis = np.arange(m, dtype=np.int32)
    mine = (T, n, m, basis, nonbasis)
    err, host = bu.host_pick(T, n, m, basis, ints, tol)
    assert err == 0
    bu.check_handmade(hm, host)
    for lp3 in (2, -1):
        got = _pick_launch([mine, mine, None, mine, mine], n + 3, m + 2,
                           [ints, np.zeros(m, dtype=np.int32)], [0, 0, 0, lp3, 0], tol)
        for q in (0, 1, 4):
            bu.same_pick(tuple(a[q].item() for a in got), host, (name, q))
        assert got[0][2] == -1 and got[0][3] == -1


# ----------------------------------------------------------------------------------------------
# the branch alone
def _branch_launch(nodes, src, brow, Rmax, ldb, Rout, snap=0.0):
    """One smx_batch_branch launch on `nodes` (as in `_pack`) for the parents `src` with the rows
    `brow` [Q]: every output block compared whole with what the contract says, every output
    poisoned before and between poisoned guard bands.  Returns tabs_c."""
    import torch
    from simplex_mi355x import _lib
    Q, Qc = len(nodes), len(src)
    final, dims, ba, nb, func = _pack(nodes, Rmax, ldb)
    h_src = np.asarray(src, dtype=np.int32)
    h_brow = np.asarray(brow, dtype=np.int32)
    d_in = [torch.from_numpy(a).to("cuda") for a in (final, dims, ba, nb, func, h_src, h_brow)]
    w_t, d_t = _guarded(torch, 2 * Qc * Rout * ldb, torch.float64, 7.0)
    w_d, d_d = _guarded(torch, 2 * Qc * 3, torch.int32, 77)
    w_b, d_b = _guarded(torch, 2 * Qc * Rout, torch.int32, 77)
    w_n, d_n = _guarded(torch, 2 * Qc * ldb, torch.int32, 77)
    w_f, d_f = _guarded(torch, 2 * Qc * ldb, torch.float64, 7.0)
    _lib.check(_lib.load().smx_batch_branch(
        d_in[0].data_ptr(), d_in[1].data_ptr(), Q, Rmax, ldb, d_in[2].data_ptr(),
        d_in[3].data_ptr(), d_in[4].data_ptr(), d_in[5].data_ptr(), d_in[6].data_ptr(), Qc, Rout,
        float(snap), d_t.data_ptr(), d_d.data_ptr(), d_b.data_ptr(), d_n.data_ptr(),
        d_f.data_ptr(), torch.cuda.current_stream().cuda_stream), "smx_batch_branch")
    _guards_intact(((w_t, 7.0), (w_d, 77), (w_b, 77), (w_n, 77), (w_f, 7.0)))
    tabs_c = d_t.cpu().numpy().reshape(2 * Qc, Rout, ldb)
    dims_c = d_d.cpu().numpy().reshape(2 * Qc, 3)
    basis_c = d_b.cpu().numpy().reshape(2 * Qc, Rout)
    nonbasis_c = d_n.cpu().numpy().reshape(2 * Qc, ldb)
    func_c = d_f.cpu().numpy().reshape(2 * Qc, ldb)
    for i, q in enumerate(h_src):
        for child in range(2):
            k, what = 2 * i + child, (i, int(q), child, Rout)
            exp = np.zeros((Rout, ldb))
            bexp = np.full(Rout, -1, dtype=np.int32)
            nexp = np.full(ldb, -1, dtype=np.int32)
            fexp = np.zeros(ldb)
            dexp = [0, 0, 0]
            if 0 <= q < Q:
                fexp, dexp = func[q], dims[q].tolist()
                if nodes[q] is None:                         # n = Rmax - 1, a relayout, dims kept
                    exp[:Rmax] = final[q]
                    bexp[:Rmax - 1] = ba[q, :Rmax - 1]
                    nexp = nb[q]
                else:
                    T, n, m, basis, nonbasis = nodes[q]
                    p = int(h_brow[q])
                    nexp[:m] = nonbasis
                    bexp[:n] = basis
                    exp[:n] = bu.snapped(final[q, :n], n, m, snap)
                    if 0 <= p < n and 0 <= basis[p] < m and n + 1 < Rout:
                        E = bu.children(T, n, m, basis, nonbasis, p)[child]
                        exp[n, :m + 1] = E[n]
                        exp[n + 1] = final[q, n]
                        bexp[n] = m + n
                        dexp = [n + 1, m, m]
                    else:
                        exp[n] = final[q, n]
            assert dims_c[k].tolist() == dexp, what
            assert su.same_floats(tabs_c[k], exp, nan_aware=True), what
            assert np.array_equal(basis_c[k], bexp), what
            assert np.array_equal(nonbasis_c[k], nexp), what
            assert su.same_floats(func_c[k], fexp), what
    return tabs_c


def _variable_rows(node, count):
    _, n, m, basis, _ = node
    rows = [p for p in range(n) if basis[p] < m]
    assert rows
    return [rows[(7 * i) % len(rows)] for i in range(count)]


@pytest.mark.parametrize("n,m", SHAPES, ids=[f"{n}x{m}" for n, m in SHAPES])
def test_branch_at_tile_and_envelope_edges(n, m):
    """Two seeded parents under seeded label permutations, both expanded, with Rmax_out at n + 2
    and above it, tight blocks and blocks with padding; every output element is compared."""
    nodes = []
    for q in range(2):
        # the first seed whose permutation puts a variable on a row
        nodes.append(next(nd for nd in (_seeded(n, m, s) for s in range(3 + q, 60, 2))
                          if (nd[3] < m).any()))
    brow = [_variable_rows(node, 1)[0] for node in nodes]
    wide = n + m + 10 <= 8192
    _branch_launch(nodes, [0, 1], brow, n + 1, m + 1, n + 2)
    if wide:
        _branch_launch(nodes, [1, 0], brow, n + 1 + 1, m + 1 + 2, n + 5)


def test_src_lists_with_gaps_repeats_and_entries_out_of_range():
    """Six nodes, of which node 2 has dims outside the block: src skips nodes, names one twice
    and names -1 and Q; brow holds a slack's row, -1 and n."""
    n, m = 9, 6
    nodes = [_seeded(n, m, 20 + q) for q in range(6)]
    nodes[2] = None
    brow = [_variable_rows(nodes[q], 1)[0] if nodes[q] else 0 for q in range(6)]
    slack = [p for p in range(n) if nodes[3][3][p] >= m][0]
    brow[3], brow[4] = slack, -1
    tabs = _branch_launch(nodes, [5, 0, 5, -1, 2, 6, 3, 4], brow, n + 1, m + 1, n + 4)
    assert su.same_floats(tabs[0], tabs[4]) and su.same_floats(tabs[1], tabs[5])
    brow[4] = n
    _branch_launch(nodes, [4, 1], brow, n + 1, m + 1, n + 2)
    # n + 1 >= Rmax_out: no room for the new row, two relayouts
    _branch_launch(nodes, [0, 1], brow, n + 1, m + 1, n + 1)


def test_snap_and_nan_payloads_on_the_device():
    n, m = 6, 4
    T, _, _, basis, nonbasis = _seeded(n, m, 2)
    T = T.copy()
    rows = _variable_rows((T, n, m, basis, nonbasis), 1)
    others = [p for p in range(n) if p != rows[0]]
    T[others[0], m], T[others[1], m], T[others[2], m] = -1e-7, -2e-6, -0.0
    T[others[3], 1] = np.float64(np.frombuffer(np.uint64(0x7ff8000000000abc).tobytes(), "f8")[0])
    tabs = _branch_launch([(T, n, m, basis, nonbasis)], [0], rows, n + 1, m + 1, n + 3, snap=1e-6)
    assert tabs[0, others[0], m] == 0 and not np.signbit(tabs[0, others[0], m])
    assert tabs[1, others[1], m] == -2e-6 and np.signbit(tabs[1, others[2], m])
    assert np.array_equal(su.bits(tabs[0, others[3]]), su.bits(T[others[3]]))
    err, e0, e1, _ = bu.host_branch(T, n, m, basis, nonbasis, rows[0], snap=1e-6)
    assert err == 0
    assert su.same_floats(tabs[0, :n + 2], e0, nan_aware=True)
    assert su.same_floats(tabs[1, :n + 2], e1, nan_aware=True)


def test_every_refusal():
    """Both entry points with real device pointers: each bad argument alone is refused with
    hipErrorInvalidValue and nothing is written; Q = 0 and Qc = 0 return without a launch."""
    import torch
    from simplex_mi355x import _lib
    L = _lib.load()
    Q, Qc, B, Rmax, ldb, Rout = 3, 2, 2, 4, 3, 6
    t = {"final": torch.zeros(Q * Rmax * ldb, dtype=torch.float64, device="cuda"),
         "dims": torch.tensor([[3, 2, 2]] * Q, dtype=torch.int32, device="cuda"),
         "basis": torch.zeros(Q * Rmax, dtype=torch.int32, device="cuda"),
         "nonbasis": torch.ones(Q * ldb, dtype=torch.int32, device="cuda"),
         "func": torch.zeros(Q * ldb, dtype=torch.float64, device="cuda"),
         "src": torch.tensor([0, 2], dtype=torch.int32, device="cuda"),
         "brow": torch.zeros(Q, dtype=torch.int32, device="cuda"),
         "ints": torch.ones(B * ldb, dtype=torch.int32, device="cuda"),
         "lp": torch.zeros(Q, dtype=torch.int32, device="cuda")}
    o = {"tabs_c": torch.full((2 * Qc * Rout * ldb,), 7.0, dtype=torch.float64, device="cuda"),
         "dims_c": torch.full((2 * Qc * 3,), 77, dtype=torch.int32, device="cuda"),
         "basis_c": torch.full((2 * Qc * Rout,), 77, dtype=torch.int32, device="cuda"),
         "nonbasis_c": torch.full((2 * Qc * ldb,), 77, dtype=torch.int32, device="cuda"),
         "func_c": torch.full((2 * Qc * ldb,), 7.0, dtype=torch.float64, device="cuda"),
         "bvar": torch.full((Q,), 77, dtype=torch.int32, device="cuda"),
         "brow_o": torch.full((Q,), 77, dtype=torch.int32, device="cuda"),
         "bval": torch.full((Q,), 7.0, dtype=torch.float64, device="cuda"),
         "bneg": torch.full((Q,), 7.0, dtype=torch.float64, device="cuda"),
         "bmin": torch.full((Q,), 7.0, dtype=torch.float64, device="cuda")}
    stream = torch.cuda.current_stream().cuda_stream

    def ptrs(null):
        return {k: (None if k == null else v.data_ptr()) for k, v in {**t, **o}.items()}

    def branch(null=None, **kw):
        a = dict(Q=Q, Qc=Qc, Rmax=Rmax, ldb=ldb, Rout=Rout)
        a.update(kw)
        p = ptrs(null)
        return L.smx_batch_branch(p["final"], p["dims"], a["Q"], a["Rmax"], a["ldb"], p["basis"],
                                  p["nonbasis"], p["func"], p["src"], p["brow"], a["Qc"],
                                  a["Rout"], 0.0, p["tabs_c"], p["dims_c"], p["basis_c"],
                                  p["nonbasis_c"], p["func_c"], stream)

    def pick(null=None, **kw):
        a = dict(Q=Q, B=B, Rmax=Rmax, ldb=ldb)
        a.update(kw)
        p = ptrs(null)
        return L.smx_batch_branch_pick(p["final"], p["dims"], a["Q"], a["Rmax"], a["ldb"],
                                       p["basis"], p["ints"], a["B"], p["lp"], 0.0, p["bvar"],
                                       p["brow_o"], p["bval"], p["bneg"], p["bmin"], stream)
    for kw in (dict(Q=-1), dict(Qc=-1), dict(Qc=1 << 30), dict(Rout=Rmax - 1),
               dict(Rmax=1, Rout=1), dict(ldb=1), dict(ldb=8190), dict(Rout=8190)):
        assert branch(**kw) == 1, kw
    for name in ("final", "dims", "basis", "nonbasis", "func", "src", "brow", "tabs_c", "dims_c",
                 "basis_c", "nonbasis_c", "func_c"):
        assert branch(null=name) == 1, name
    for kw in (dict(Q=-1), dict(B=-1), dict(Rmax=1), dict(ldb=1), dict(ldb=8190)):
        assert pick(**kw) == 1, kw
    for name in ("final", "dims", "basis", "ints", "lp", "bvar", "brow_o", "bval", "bneg", "bmin"):
        assert pick(null=name) == 1, name
    assert branch(Qc=0) == 0 and pick(Q=0) == 0
    torch.cuda.synchronize()
    for name, v in o.items():
        assert (v == (7.0 if v.dtype == torch.float64 else 77)).all(), name
    assert branch() == 0 and pick() == 0
    torch.cuda.synchronize()
    assert (o["dims_c"].cpu().numpy().reshape(-1, 3) == [4, 2, 2]).all()
    assert (o["bvar"] == -1).all()
    for Rmax_out, ldb_, fits in ((2, 2, 1), (8190, 2, 1), (1, 3, 0), (8191, 2, 0), (-1, 4, 0)):
        assert L.smx_batch_branch_fits(Rmax_out, ldb_) == fits
        assert L.smx_batch_cuts_fits(Rmax_out, ldb_) == fits


# ----------------------------------------------------------------------------------------------
# the chain, two levels deep
def _two_levels(members, cap, Pw, kernel, depth=2):
    """members: [(kind, n, m, seed, flen)] -> the driver's own steps (base solve, pick, branch,
    warm solve under the dual rule, solution from the children's labels), two levels deep, every
    pick, every child's start table, final table, status, pivot log and labels against the
    restatements on the oracle's root tables.  Returns (base tier, warm tier, nodes solved); the
    warm runs must have pivoted, or nothing was chained."""
    import torch
    from simplex_mi355x import _lib, batch
    refs = [case(kind, n, m, seed, cap, flen) for kind, n, m, seed, flen in members]
    B = len(members)
    Rmax = max(n for _, n, _, _, _ in members) + 1
    ldb = max(m for _, _, m, _, _ in members) + 1
    tabs = np.zeros((B, Rmax, ldb))
    dims = np.zeros((B, 3), dtype=np.int32)
    mirror = []
    for q, ((_, n, m, _, flen), ref) in enumerate(zip(members, refs)):
        tabs[q, :n + 1, :m + 1] = ref[0]
        dims[q] = (n, m, flen)
        basis, nonbasis, _ = su.replay(ref[5], n, m)
        mirror.append((ref[2], n, m, flen, basis, nonbasis))
    which = batch.choose_kernel(Rmax, ldb, kernel)
    Rout = Rmax + depth
    warm = batch.warm_kernel(which, Rout, ldb)
    L = _lib.load()
    dev = torch.device("cuda")
    stream = torch.cuda.current_stream(dev)
    d_dims = torch.from_numpy(dims).to(dev)
    run, d_func, sol, _ = batch._enqueue_base(L, stream, which, torch.from_numpy(tabs).to(dev),
                                              d_dims, cap)
    node = (run[0], d_dims, sol[3], sol[4], d_func)
    d_ints = torch.ones((B, ldb), dtype=torch.int32, device=dev)
    h_lp = np.arange(B, dtype=np.int32)
    solved = pivots = 0
    for level in range(1, depth + 1):
        picks = batch._device_pick(L, stream, node, d_ints, torch.from_numpy(h_lp).to(dev), bu.TOL)
        got = [a.cpu().numpy() for a in picks]
        src = []
        for q, (T, n, m, flen, basis, nonbasis) in enumerate(mirror):
            exp = bu.pick(T, n, m, basis, np.ones(m, dtype=np.int32), bu.TOL)
            bu.same_pick(tuple(a[q].item() for a in got), exp, (level, q))
            if exp[0] >= 0:
                src.append(q)
        assert src, level
        h_src = np.array(src, dtype=np.int32)
        kids = batch._device_branch(L, stream, node, torch.from_numpy(h_src).to(dev), picks[1],
                                    Rout, bu.TOL)
        d_out, d_rc, _, d_st, d_np, _ = batch._device_solve(L, stream, warm, kids[0], kids[1], Pw,
                                                            rule=_lib.RULE_DUAL)
        wsol = batch._device_solution(L, stream, d_out, kids[1], Pw, d_rc, d_np, kids[4],
                                      (kids[2], kids[3], 1))
        start, final = kids[0].cpu().numpy(), d_out.cpu().numpy()
        st, npv, rc = d_st.cpu().numpy(), d_np.cpu().numpy(), d_rc.cpu().numpy()
        wba, wnb = wsol[3].cpu().numpy(), wsol[4].cpu().numpy()
        nxt = []
        for i, q in enumerate(src):
            T, n, m, flen, basis, nonbasis = mirror[q]
            down, up, bc = bu.children(T, n, m, basis, nonbasis, int(got[1][q]))
            for child, E in enumerate((down, up)):
                k, what = 2 * i + child, (level, q, child)
                E = bu.snapped(E, n, m, bu.TOL)
                assert su.same_floats(start[k, :n + 2, :m + 1], E), (what, "start")
                Tw, wst, done, log, _ = du.run(E, n + 1, m, flen, Pw, du.DUAL)
                assert (int(st[k]), int(npv[k])) == (wst, done), (what, st[k], npv[k], wst, done)
                assert np.array_equal(rc[k, :done], np.asarray(log).reshape(-1, 2)), (what, "log")
                assert su.same_floats(final[k, :n + 2, :m + 1], Tw), (what, "final")
                wb, wn = cu.warm_labels(bc, nonbasis, log, n + 1, m)
                assert np.array_equal(wba[k, :n + 1], wb), (what, "basis")
                assert np.array_equal(wnb[k, :m], wn), (what, "nonbasis")
                nxt.append((Tw, n + 1, m, flen, wb, wn))
                solved += 1
                pivots += done
        mirror = nxt
        h_lp = np.repeat(h_lp[h_src], 2)
        node = (d_out, kids[1], wsol[3], wsol[4], kids[4])
    assert pivots > 0
    return which, warm, solved


def test_chain_on_the_wavefront_tier():
    which, warm, solved = _two_levels([("uniform", 3, 2, 0, 2), ("uniform", 40, 7, 1, 8),
                                       ("mixed", 20, 20, 0, 20)], 64, 64, "wave")
    assert (which, warm) == ("wave", "wave") and solved >= 6


def test_a_63_row_root_whose_children_leave_the_wavefront_tier():
    which, warm, _ = _two_levels([("uniform", 63, 63, 0, 63), ("uniform", 63, 40, 1, 40)], 64, 32,
                                 "wave")
    assert (which, warm) == ("wave", "workgroup")


def test_chain_on_the_workgroup_tier():
    which, warm, _ = _two_levels([("uniform", 100, 100, 0, 100)], 256, 32, "workgroup")
    assert (which, warm) == ("workgroup", "workgroup")


def test_a_root_at_the_lds_edge_whose_children_go_to_the_global_memory_tier():
    from simplex_mi355x.batch import gm_fits, wg_lds_bytes
    ldb = 141
    Rmax = max(R for R in range(100, 400) if wg_lds_bytes(R, ldb) >= 0)
    assert wg_lds_bytes(Rmax + 1, ldb) < 0 and gm_fits(Rmax + 2, ldb)
    which, warm, _ = _two_levels([("uniform", Rmax - 1, ldb - 1, 0, ldb - 1)], 16, 16, "auto")
    assert (which, warm) == ("workgroup", "global")


def test_chain_on_the_global_memory_tier():
    which, warm, _ = _two_levels([("uniform", 141, 141, 0, 141)], 64, 16, "global")
    assert (which, warm) == ("global", "global")


# ----------------------------------------------------------------------------------------------
# the public calls
def _host_answer(cons, func, **kw):
    import simplex
    return simplex.SimplexMethod(cons, func, device="cpu").solve_integer(**kw)


def _same_answer(got, exp, what):
    assert got.status == exp.status, (what, got, exp)
    assert (got.nodes, got.warm_pivots, got.depth) == (exp.nodes, exp.warm_pivots, exp.depth), \
        (what, got, exp)
    assert (got.x is None) == (exp.x is None), what
    if exp.x is not None:
        assert su.same_floats(got.x, exp.x) and su.same_floats(got.x_raw, exp.x_raw), what
    assert su.same_floats(got.objective, exp.objective), what
    assert su.same_floats(got.bound, exp.bound), what


def test_solve_batch_integer_equals_the_host_engine_on_the_meaning_set():
    """The first 64 seeds in one call, mixed shapes: status, rounded x, objective, bound, node
    and warm-pivot counts and depth are SimplexMethod.solve_integer()'s on the host engine, and
    every "optimal" is the enumerated minimum."""
    from simplex_mi355x.batch import solve_batch_integer
    problems = [bu.problem(*bu.instance(seed)) for seed in range(64)]
    got = solve_batch_integer(problems, max_pivots=256, max_depth=16)
    assert len(got) == 64
    for seed, (r, (cons, func)) in enumerate(zip(got, problems)):
        _same_answer(r, _host_answer(cons, func, max_pivots=256, max_depth=16), seed)
        if r.status == "optimal":
            assert r.objective == float(bu.brute_of(seed)), seed
    assert sum(r.status == "optimal" for r in got) >= 61


def test_masks_limits_and_roots_through_the_batch():
    from simplex_mi355x.batch import solve_batch_integer
    pinned = ([[-1.0, -1.0, 6.0], [-9.0, -5.0, 45.0]], [-8.0, -5.0])
    empty = ([[1.0, 0.0, -0.25], [-1.0, 0.0, 0.75], [0.0, -1.0, 3.0]], [-1.0, -1.0])
    wrong = ([[1.0, 1.0, -2.0], [-1.0, -1.0, 1.0]], [-1.0, -1.0])
    problems = [pinned, pinned, pinned, empty, wrong]
    masks = [None, [1, 0], [0, 0], None, None]
    got = solve_batch_integer(problems, masks)
    assert [r.status for r in got] == ["optimal", "optimal", "optimal", "infeasible", "error"]
    assert got[0].x.tolist() == [5.0, 0.0] and got[0].objective == -40.0
    for r, (cons, func), mask in zip(got, problems, masks):
        _same_answer(r, _host_answer(cons, func, integers=mask, max_pivots=256), mask)
    for kw in (dict(max_depth=1), dict(max_depth=0), dict(warm_pivots=0), dict(max_nodes=2)):
        r = solve_batch_integer([pinned], **kw)[0]
        _same_answer(r, _host_answer(*pinned, max_pivots=256, **kw), kw)
        if "max_nodes" not in kw:
            assert r.status == "limit" and r.bound <= -40.0 <= r.objective
    assert solve_batch_integer([]) == []


def test_solve_integer_on_the_device_backend():
    import simplex
    pinned = ([[-1.0, -1.0, 6.0], [-9.0, -5.0, 45.0]], [-8.0, -5.0])
    empty = ([[1.0, 0.0, -0.25], [-1.0, 0.0, 0.75], [0.0, -1.0, 3.0]], [-1.0, -1.0])
    for (cons, func), kw in ((pinned, {}), (pinned, dict(integers=[1, 0])),
                             (pinned, dict(max_depth=1)), (empty, {})):
        sm = simplex.SimplexMethod(cons, func, device="cuda:0")
        assert sm.backend == "hip"
        _same_answer(sm.solve_integer(**kw), _host_answer(cons, func, **kw), kw)
