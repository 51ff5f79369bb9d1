"""The one-pivot update kernel's test cases on the CPU: update_util's restated launch geometry gives,
at the 256 CUs of an MI355X, what each shape of test_gpu_update_variants.py is there for; the
thresholds and the variant table it copies are the ones in csrc/smx_kernels.hip; and the host-only
smx_tune_set / smx_tune_get keep their contract.  Nothing here touches a GPU.
"""
from __future__ import annotations

import ctypes
import os
import re

import pytest

import update_util as uu
from conftest import PKG_DIR

CUS = 256   # an MI355X; the GPU tests evaluate the same properties at the device's own count
KERNELS = os.path.join(PKG_DIR, "csrc", "smx_kernels.hip")


def _nparts(rows, m):
    from simplex_mi355x import _lib
    return _lib.load().smx_nparts_for(rows, m)


# -- geometry -------------------------------------------------------------------------------------
def test_geometry_by_hand():
    """update_grid on a case small enough to follow: 10 rows x 300 columns on 2 CUs, 3 workgroups
    per CU.  R = 11, 3 chunks, 33 units; 6 workgroups = 24 waves = 2 x lcm(3, 4), nothing to trim;
    need = ceil(33 / 4) = 9 does not bind.  NW = 24: qs = 8, rs = 0; 2 / 1 / 1 iterations.  With 1
    reserved workgroup: 5 workgroups = 20 waves, cut to 12 (a multiple of 12, but under 3/4 of 20:
    refused), so 20 waves, qs = 6, rs = 2."""
    g = uu.geometry(10, 299, 2, 3)
    assert (g.blocks, g.NW, g.nchunks, g.units, g.qs, g.rs, g.need, g.trimmed) == \
        (6, 24, 3, 33, 8, 0, 9, False)
    assert g.iters == {1: 2, 2: 1, 4: 1}
    g = uu.geometry(10, 299, 2, 3, reserved=1)
    assert (g.blocks, g.NW, g.qs, g.rs, g.trimmed) == (5, 20, 6, 2, False)
    # a trim that is taken: 7 workgroups = 28 waves -> 24
    g = uu.geometry(10, 299, 7, 1)
    assert (g.blocks, g.NW, g.rs, g.trimmed) == (6, 24, 0, True)
    # the launch never has fewer workgroups than nparts
    assert uu.geometry(1, 1, 256, 5, nparts=3).NW == 12


@pytest.mark.parametrize("shape", list(uu.SHAPES), ids=lambda s: "{}x{}".format(*s))
def test_shape_gives_what_it_is_there_for(shape):
    bpc = uu.SHAPES[shape][0]
    g = uu.geometry(*shape, CUS, bpc)
    assert (g.blocks, g.NW, g.nchunks, g.rs, tuple(g.iters[u] for u in (1, 2, 4))) == \
        uu.CENSUS_256[shape]
    uu.check_property(shape, g)
    assert uu.table_bytes(*shape) <= uu.LA_SWEEP_TABLE


def test_shapes_cover_the_geometries():
    """Every property once at least; a batch with out-of-range slots only, a ragged last batch and
    a chunk change between real units for U = 2 and U = 4 are all there."""
    assert {p for _, p in uu.SHAPES.values()} == {"tiny", "exact", "need", "ragged", "walk",
                                                  "production"}
    assert set(uu.SHAPES) == set(uu.CENSUS_256) and set(uu.CHAIN_SHAPES) == set(uu.RESERVED_256)
    walk = uu.geometry(40, 16500, CUS, 1)
    assert not walk.trimmed and walk.blocks == CUS and walk.blocks < walk.need   # the CU cap binds
    # trim refused: the largest multiple of lcm(129, 4) = 516 waves is under 3/4 of 1024
    assert (1024 - 1024 % 516) * 4 < 1024 * 3


@pytest.mark.parametrize("shape", uu.CHAIN_SHAPES, ids=lambda s: "{}x{}".format(*s))
def test_fused_chain_geometry(shape):
    """The fused chain's launches reserve nparts workgroups below 256 MiB: the shapes keep their
    properties with them."""
    bpc = uu.SHAPES[shape][0]
    nparts = _nparts(*shape)
    assert not uu.la_sweeps(*shape)
    g = uu.geometry(*shape, CUS, bpc, reserved=nparts, nparts=nparts)
    assert (nparts, g.blocks, g.NW, g.rs, tuple(g.iters[u] for u in (1, 2, 4))) == \
        uu.RESERVED_256[shape]
    uu.check_property(shape, g)


@pytest.mark.parametrize("case", uu.SHARD_CASES, ids=lambda c: "{}x{}".format(*c[1:3]))
def test_shard_geometry(case):
    from simplex_mi355x.sharded import row_range
    _kind, n, m, ranks, bpc, _k, prop = case
    assert uu.rank_rows(n, ranks) == [hi - lo for lo, hi in
                                      (row_range(n, p, ranks) for p in range(ranks))]
    for rows in uu.rank_rows(n, ranks):
        nparts = _nparts(rows, m)
        for fused in (0, 1):
            g = uu.rank_geometry(rows, m, CUS, bpc, bool(fused), nparts, ranks)
            assert (nparts, g.NW, g.rs, tuple(g.iters[u] for u in (1, 2, 4))) == \
                uu.SHARD_256[n, m][fused, rows]
            uu.check_property((n, m), g, prop)


def test_look_ahead_sweep_sizes():
    """4100 x 8192 doubles is four rows past 256 MiB; 4096 x 8192 is 256 MiB exactly and keeps the
    reserved workgroups (the comparison is `>`)."""
    assert uu.leading_dim(uu.LA_M) == 8192
    assert uu.table_bytes(uu.LA_N_BELOW, uu.LA_M) == uu.LA_SWEEP_TABLE
    assert not uu.la_sweeps(uu.LA_N_BELOW, uu.LA_M) and uu.la_sweeps(uu.LA_N, uu.LA_M)
    assert uu.table_bytes(uu.LA_N, uu.LA_M) - uu.LA_SWEEP_TABLE == 4 * 8192 * 8
    nparts = _nparts(uu.LA_N, uu.LA_M)
    assert nparts == _nparts(uu.LA_N_BELOW, uu.LA_M) == 32
    above = uu.geometry(uu.LA_N, uu.LA_M, CUS, uu.LA_BPC, 0, nparts)
    below = uu.geometry(uu.LA_N_BELOW, uu.LA_M, CUS, uu.LA_BPC, nparts, nparts)
    assert (above.blocks, above.NW, above.rs, tuple(above.iters.values())) == \
        (1280, 5120, 0, (52, 26, 13))
    assert (below.blocks, below.NW, below.rs, tuple(below.iters.values())) == \
        (1248, 4992, 0, (53, 27, 14))
    assert len(uu.LA_CASES) == 4
    assert [c for c in uu.LA_CASES if c[2] == uu.LA_N_BELOW] == [("uniform", -1, uu.LA_N_BELOW)]
    assert uu.VARIANTS[7] == (4, 1, 0, 1)


# -- the sources ----------------------------------------------------------------------------------
def _source():
    with open(KERNELS) as fh:
        return fh.read()


def _constant(name):
    mt = re.search(r"constexpr\s+int(?:64_t)?\s+" + name + r"\s*=\s*(\d+)(?:ll)?\s*(?:<<\s*(\d+))?\s*;",
                   _source())
    assert mt, name
    return int(mt.group(1)) << int(mt.group(2) or 0)


def test_thresholds_match_the_sources():
    assert _constant("kCacheTable") == uu.CACHE_TABLE
    assert _constant("kLaSweepTable") == uu.LA_SWEEP_TABLE
    assert _constant("kFirstDiagVariant") == uu.FIRST_DIAG_VARIANT
    mt = re.search(r"constexpr\s+int\s+kLargeVariant\s*=\s*(\d+)\s*,\s*kSmallVariant\s*=\s*(\d+)\s*;",
                   _source())
    assert mt and (int(mt.group(2)), int(mt.group(1))) == (uu.SMALL_VARIANT, uu.LARGE_VARIANT)
    common = open(os.path.join(PKG_DIR, "csrc", "smx_common.hpp")).read()
    blk = int(re.search(r"constexpr\s+int\s+kUpdBlock\s*=\s*(\d+)\s*;", common).group(1))
    wave = int(re.search(r"constexpr\s+int\s+kWave\s*=\s*(\d+)\s*;", common).group(1))
    assert blk // wave == uu.UPD_WAVES and 2 * wave == uu.CHUNK


def test_variant_table_matches_the_sources():
    """The kVariants initialiser and the template arguments upd_fn hands out, variant by variant."""
    mt = re.search(r"kVariants\[\]\s*=\s*\{(.*?)\};", _source(), flags=re.S)
    assert mt
    rows = [tuple(int(x) for x in row.split(","))
            for row in re.findall(r"\{\s*([\d\s,]+?)\s*\}", mt.group(1))]
    assert tuple(rows[:uu.FIRST_DIAG_VARIANT]) == uu.VARIANTS
    assert len(rows) == uu.FIRST_DIAG_VARIANT + 2
    fn = re.search(r"UpdFn upd_fn\(int v\) \{(.*?)\n\}", _source(), flags=re.S).group(1)
    cases = dict(re.findall(r"case (\d+): return k_update<MODE, ([^>]+)>;", fn))
    flag = {"true": 1, "false": 0}
    for v, (u, nts, ntl, pipe) in enumerate(uu.VARIANTS):
        args = [a.strip() for a in cases[str(v)].split(",")]
        assert len(args) == 4, (v, args)    # no DIAG argument below kFirstDiagVariant
        assert (int(args[0]), flag[args[1]], flag[args[2]], flag[args[3]]) == (u, nts, ntl, pipe), v
    assert {u for u, *_ in uu.VARIANTS} == set(uu.UNITS_IN_FLIGHT)
    assert any(p for *_, p in uu.VARIANTS) and any(not s for _, s, _, _ in uu.VARIANTS)


# -- smx_tune_set / smx_tune_get (host-only) ------------------------------------------------------
def _get(L):
    v = [ctypes.c_int32() for _ in range(6)]
    assert L.smx_tune_get(*(ctypes.byref(x) for x in v)) == 0
    return dict(zip(("variant", "bpc", "nvariants", "units", "vec", "nt"), (x.value for x in v)))


def test_tune_set_and_get_contract(monkeypatch):
    from simplex_mi355x import _lib
    monkeypatch.delenv("SMX_ALLOW_DIAG", raising=False)   # the opt-in is read at every call
    L = _lib.load()
    before = _get(L)
    try:
        nv = before["nvariants"]
        assert nv == uu.FIRST_DIAG_VARIANT + 2
        assert L.smx_tune_set(-2, 3) == 0
        for bad in (nv, nv + 1, 1 << 20):
            assert L.smx_tune_set(bad, 4) != 0
        for diag in range(uu.FIRST_DIAG_VARIANT, nv):   # wrong-bits timing variants: refused
            assert L.smx_tune_set(diag, 4) != 0
        got = _get(L)
        assert (got["variant"], got["bpc"]) == (-1, 3)   # a refused call changes nothing
        for v, (u, _nts, _ntl, _pipe) in enumerate(uu.VARIANTS):
            assert L.smx_tune_set(v, -1) == 0
            got = _get(L)
            assert (got["variant"], got["bpc"], got["units"], got["vec"], got["nt"]) == \
                (v, 3, u, 2, uu.nt_bits(v)), v
        assert L.smx_tune_set(-1, 5) == 0                # -1 keeps the variant
        assert (_get(L)["variant"], _get(L)["bpc"]) == (len(uu.VARIANTS) - 1, 5)
        assert L.smx_tune_set(-1, -1) == 0               # and a negative bpc the override
        assert (_get(L)["variant"], _get(L)["bpc"]) == (len(uu.VARIANTS) - 1, 5)
        assert L.smx_tune_set(-2, -1) == 0               # -2 restores automatic
        got = _get(L)
        assert (got["variant"], got["bpc"]) == (-1, 5)
        # automatic reports the variant of tables that stream from HBM
        assert (got["units"], got["nt"]) == (uu.VARIANTS[uu.LARGE_VARIANT][0],
                                             uu.nt_bits(uu.LARGE_VARIANT))
        assert L.smx_tune_get(None, None, None, None, None, None) == 0
    finally:
        L.smx_tune_set(before["variant"] if before["variant"] >= 0 else -2, before["bpc"])
    assert _get(L) == before
