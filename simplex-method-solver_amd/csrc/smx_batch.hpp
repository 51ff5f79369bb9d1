// smx_batch.hpp -- k_copy (copy-ceiling probe) and k_batch (many small LPs, one wavefront each)
// Part of libsmx (compiled as one translation unit by smx_kernels.hip; not a standalone header).
#pragma once
#pragma clang fp contract(off)

namespace {

// ---------------------------------------------------------------------------------------------
// k_copy: the box's streaming read+write ceiling, measured next to the update in bench.py
// (the best shapes of tools/hbm_probe.hip: a grid-stride copy with U 16-B loads per lane).
template <int U>
__global__ void k_copy(const dbl2* __restrict__ a, dbl2* __restrict__ b, int64_t n) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t st = (int64_t)gridDim.x * blockDim.x;
    for (; i + (U - 1) * st < n; i += U * st) {
        dbl2 v[U];
#pragma unroll
        for (int k = 0; k < U; ++k) v[k] = a[i + k * st];
#pragma unroll
        for (int k = 0; k < U; ++k) b[i + k * st] = v[k];
    }
    for (; i < n; i += st) b[i] = a[i];
}

// ---------------------------------------------------------------------------------------------
// k_batch: many small LPs, one wavefront each (the UI's workload, m = 2,
// n = 3..20, main.py:309-313).  Lane i holds row i of its LP in registers (rows 0..n, the
// f-row is lane n), so the whole get_solution loop (simplex.py:184-198) runs inside one launch:
// phase 1 by a ballot (simplex.py:72-76), the pivot row and the f-row by shuffles
// (:81-85, :94-98), the ratio test by the same wave arg-min as k_select (:105-141), and every
// element with the same (t*e - pr*pc)/e as k_update (:155-175).  Per step: (r, c), (x1, x2) of
// the new table (find_optimum, :51-68) and optionally the table itself (the Info snapshots).
// The body is smx_batch_body.hpp, which k_batch_dual shares.
template <int CMAX>
__device__ __forceinline__ double pick(const double (&x)[CMAX], int j) {
    double v = 0.0;
#pragma unroll
    for (int q = 0; q < CMAX; ++q) v = (q == j) ? x[q] : v;
    return v;
}

template <int CMAX>
__global__ __launch_bounds__(256) void k_batch(
    const double* __restrict__ tabs, const int32_t* __restrict__ dims, int B, int Rmax, int ldb,
    int max_pivots, double* __restrict__ out, int32_t* __restrict__ rc,
    double* __restrict__ xv, double* __restrict__ snaps, int32_t* __restrict__ status_out,
    int32_t* __restrict__ np_out) {
    constexpr int RULE = SMX_RULE_REFERENCE;
#include "smx_batch_body.hpp"
}

// k_batch_dual: k_batch under SMX_RULE_DUAL (include/smx.h); everything else is the same text.
template <int CMAX>
__global__ __launch_bounds__(256) void k_batch_dual(
    const double* __restrict__ tabs, const int32_t* __restrict__ dims, int B, int Rmax, int ldb,
    int max_pivots, double* __restrict__ out, int32_t* __restrict__ rc,
    double* __restrict__ xv, double* __restrict__ snaps, int32_t* __restrict__ status_out,
    int32_t* __restrict__ np_out) {
    constexpr int RULE = SMX_RULE_DUAL;
#include "smx_batch_body.hpp"
}

}  // namespace
