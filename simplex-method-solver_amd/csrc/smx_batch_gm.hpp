// smx_batch_gm.hpp -- k_batch_gm (many LPs past one CU's LDS, one workgroup each, tableau in
// global memory)
// Part of libsmx (compiled as one translation unit by smx_kernels.hip; not a standalone header).
#pragma once
#pragma clang fp contract(off)

namespace {

// ---------------------------------------------------------------------------------------------
// k_batch_gm: k_batch_wg (smx_batch_wg.hpp) with the table left in global memory.  One workgroup
// per LP; the workgroup copies tabs[b] to out[b] and runs wg_pivot_loop in place on out[b], row
// pitch ldb.  Arguments, layouts and status codes are k_batch_wg's.
//
// Dynamic LDS: s_prow[ldb], s_pcol[Rmax] and, with MIRRORS, s_frow[ldb], s_bcol[Rmax],
// 16 * (Rmax + ldb) bytes in all.  MIRRORS = false takes 8 * (Rmax + ldb) bytes; measured
//  it is the faster of the two -- the two compares per element of the update cost
// more than a column walk per step -- and the default.  U, the loads issued ahead of the
// divisions: 1 is k_batch_wg's loop, 8 is the default.  RULE is wg_pivot_loop's
// (with MIRRORS a dual step reads the f-row from s_frow).  out is a plain pointer, as
// wg_pivot_loop's "Between threads" requires of the working table.
template <bool MIRRORS, int U, int RULE>
__global__ __launch_bounds__(kWgMaxBlock) void k_batch_gm(
    const double* __restrict__ tabs, const int32_t* __restrict__ dims, int B, int Rmax, int ldb,
    int max_pivots, double* out, int32_t* __restrict__ rc, double* __restrict__ xv,
    double* __restrict__ snaps, int32_t* __restrict__ status_out, int32_t* __restrict__ np_out) {
    extern __shared__ double s_gm[];   // s_prow[ldb], s_pcol[Rmax]; MIRRORS: s_frow[ldb], s_bcol[Rmax]
    double* s_prow = s_gm;
    double* s_pcol = s_prow + ldb;
    double* s_frow = s_pcol + Rmax;                        // touched only with MIRRORS
    double* s_bcol = s_frow + ldb;
    WgLp lp;
    if (!wg_lp(dims, B, Rmax, ldb, status_out, np_out, lp)) return;
    const int b = blockIdx.x;
    const int R = lp.n + 1;
    const size_t tab_elems = (size_t)Rmax * ldb;
    const size_t hs = (size_t)b * max_pivots;
    const WgWalk w0(threadIdx.x, blockDim.x, lp.m + 1);
    const double* src = tabs + (size_t)b * tab_elems;
    double* T = out + (size_t)b * tab_elems;               // the working table
    for (WgWalk w = w0; w.i < R; w.next()) {
        const double v = src[w.i * ldb + w.j];
        T[w.i * ldb + w.j] = v;
        if (MIRRORS) {
            if (w.j == lp.m) s_bcol[w.i] = v;
            if (w.i == lp.n) s_frow[w.j] = v;
        }
    }
    __syncthreads();
    wg_pivot_loop<U, MIRRORS, true, RULE>(
        T, ldb, s_prow, s_pcol, s_frow, s_bcol, lp, w0, max_pivots, rc + 2 * hs, xv + 2 * hs,
        snaps ? snaps + hs * tab_elems : nullptr, ldb, tab_elems, status_out + b, np_out + b);
}

// Host: one launch of the instance (MIRRORS, U, RULE) with `block` threads per LP.  max_lds is the
// envelope's largest dynamic LDS.
using GmLaunch = int(int, int, const double*, const int32_t*, int, int, int, int, double*,
                     int32_t*, double*, double*, int32_t*, int32_t*, hipStream_t);

template <bool MIRRORS, int U, int RULE>
int launch_batch_gm(int block, int max_lds, const double* tabs, const int32_t* dims, int B,
                    int Rmax, int ldb, int max_pivots, double* out, int32_t* rc, double* xv,
                    double* snaps, int32_t* status, int32_t* npivots, hipStream_t st) {
    if (const int err = wg_raise_lds_limit<k_batch_gm<MIRRORS, U, RULE>>(max_lds)) return err;
    hipLaunchKernelGGL((k_batch_gm<MIRRORS, U, RULE>), dim3(B), dim3(block),
                       (size_t)(MIRRORS ? 16 : 8) * ((size_t)Rmax + ldb), st, tabs, dims, B, Rmax,
                       ldb, max_pivots, out, rc, xv, snaps, status, npivots);
    return (int)hipGetLastError();
}

}  // namespace
