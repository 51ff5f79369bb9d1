// smx_batch_gm.hpp -- k_batch_gm (many LPs past one CU's LDS, one workgroup each, tableau in
// global memory)
// Part of libsmx (compiled as one translation unit by smx_kernels.hip; not a standalone header).
#pragma once
#pragma clang fp contract(off)

namespace {

// ---------------------------------------------------------------------------------------------
// k_batch_gm: k_batch_wg (smx_batch_wg.hpp) with the table left in global memory.  One workgroup
// per LP; the workgroup copies tabs[b] to out[b] and runs the whole get_solution loop
// (simplex.py:184-198) in place on out[b], row pitch ldb.  Arguments, layouts, status codes and
// the label tracking are k_batch_wg's; so are the per-step decision (smx_batch_wg.hpp:84-177)
// and the per-element arithmetic (:186-196) -- only where the operands come from differs.
//
// Dynamic LDS: s_prow[ldb], s_pcol[Rmax] (the old pivot row and column, copied out before the
// update) and, with MIRRORS, s_frow[ldb], s_bcol[Rmax] (mirrors of the f-row and the "-b" column),
// 16 * (Rmax + ldb) bytes in all.  A mirror entry is written by the thread that writes that table
// element, with the same value, so the two scans of a step and the ratio test's "-b" operand never
// walk a column of global memory at stride ldb.  MIRRORS = false reads the table instead and
// takes 8 * (Rmax + ldb) bytes; measured it is the faster of the two -- the two
// compares per element of the update cost more than a column walk per step -- and the default.
//
// The update walks the table as k_batch_wg does, U elements of the thread's walk at a time: the U
// loads are issued before the first division, so one workgroup alone (a small batch) does not
// wait out a global-memory round trip per element.  U = 1 is k_batch_wg's loop as it stands; 8 is
// the default.
//
// Between threads: during the update every element is read and written by one thread and every
// right-hand side comes from LDS.  What a thread wrote is read by other threads of the same
// workgroup only after a __syncthreads(), which orders global memory at workgroup scope; the
// working table is reached through a plain pointer (no const __restrict__), so no load is hoisted
// over a barrier or served from a read-only path.  An LP never spans workgroups: no flags, no
// spinning, no co-residency.
template <bool MIRRORS, int U>
__global__ __launch_bounds__(kWgMaxBlock) void k_batch_gm(
    const double* __restrict__ tabs, const int32_t* __restrict__ dims, int B, int Rmax, int ldb,
    int max_pivots, double* out, int32_t* __restrict__ rc, double* __restrict__ xv,
    double* __restrict__ snaps, int32_t* __restrict__ status_out, int32_t* __restrict__ np_out) {
    extern __shared__ double s_gm[];   // s_prow[ldb], s_pcol[Rmax]; MIRRORS: s_frow[ldb], s_bcol[Rmax]
    __shared__ int s_nb[kWgMaxWaves];
    __shared__ int s_nf[kWgMaxWaves];
    __shared__ int s_p1[kWgMaxWaves];
    __shared__ First s_f[kWgMaxWaves];
    __shared__ Cand s_c[kWgMaxWaves];
    double* s_prow = s_gm;
    double* s_pcol = s_prow + ldb;
    double* s_frow = s_pcol + Rmax;                        // touched only with MIRRORS
    double* s_bcol = s_frow + ldb;
    const int tid = threadIdx.x;
    const int nt = blockDim.x;
    const int lane = tid & (kWave - 1);
    const int wid = tid >> 6;
    const int nw = nt >> 6;
    const int b = blockIdx.x;
    if (b >= B) return;
    const int n = dims[3 * b], m = dims[3 * b + 1], flen = dims[3 * b + 2];
    if (n < 1 || m < 1 || n + 1 > Rmax || m + 1 > ldb) {   // outside the launch's padding
        if (tid == 0) {
            status_out[b] = SMX_IDLE;
            np_out[b] = 0;
        }
        return;
    }
    const int R = n + 1, C = m + 1;
    const int fscan = flen < m ? flen : m;
    const size_t tab_elems = (size_t)Rmax * ldb;
    double* T = out + (size_t)b * tab_elems;               // the working table
    // this thread's walk over the R x C elements: (i0, j0), then nt elements further each time
    const int i0 = tid / C, j0 = tid - i0 * C;
    const int di = nt / C, dj = nt - di * C;
    {
        const double* src = tabs + (size_t)b * tab_elems;
        for (int i = i0, j = j0; i < R;) {
            const double v = src[(size_t)i * ldb + j];
            T[(size_t)i * ldb + j] = v;
            if (MIRRORS) {
                if (j == m) s_bcol[i] = v;
                if (i == n) s_frow[j] = v;
            }
            i += di;
            j += dj;
            if (j >= C) {
                j -= C;
                ++i;
            }
        }
    }
    __syncthreads();
    int p1 = (m >= 1) ? -1 : SMX_ABSENT;   // label positions of 'x1', 'x2' (simplex.py:30)
    int p2 = (m >= 2) ? -2 : SMX_ABSENT;
    int status = SMX_PIVOT;
    int np = 0;
    const double* Tb = T + m;                               // the "-b" column
    const double* Tf = T + (size_t)n * ldb;                 // the f-row
    for (int step = 0; step < max_pivots; ++step) {
        // first row with b < 0 (simplex.py:72-76) and first f-row entry < 0 (:94-98) together
        int nb = SMX_NONE, nf = SMX_NONE;
        for (int i = tid; i < n; i += nt) {
            if ((MIRRORS ? s_bcol[i] : Tb[(size_t)i * ldb]) < 0.0) {
                nb = i;
                break;
            }
        }
        for (int j = tid; j < fscan; j += nt) {
            if ((MIRRORS ? s_frow[j] : Tf[j]) < 0.0) {
                nf = j;
                break;
            }
        }
        nb = wave_min_int(nb);
        nf = wave_min_int(nf);
        if (lane == 0) {
            s_nb[wid] = nb;
            s_nf[wid] = nf;
        }
        __syncthreads();
        nb = wg_merge_min(s_nb, nw, lane);
        nf = wg_merge_min(s_nf, nw, lane);
        int r = SMX_NONE, c = SMX_NONE;
        bool have_col = false;                               // s_pcol[0..n) already holds column c
        if (nb != SMX_NONE) {                                // phase 1 (simplex.py:72-91)
            r = nb;
            const double* rowp = T + (size_t)r * ldb;
            int p = SMX_NONE;
            for (int j = tid; j < m; j += nt) {
                if (rowp[j] > 0.0) {
                    p = j;
                    break;
                }
            }
            p = wave_min_int(p);
            if (lane == 0) s_p1[wid] = p;
            __syncthreads();
            c = wg_merge_min(s_p1, nw, lane);
            if (c == SMX_NONE) {
                status = SMX_INCORRECT;
                break;
            }
        } else {
            c = nf;
            if (c == SMX_NONE) {
                status = (flen < m) ? SMX_FSHORT : SMX_OPTIMUM;
                break;
            }
            First f{SMX_NONE, 0.0};                          // simplex.py:111-136
            Cand bc = cand_none();
            for (int i = tid; i < n; i += nt) {
                const double a = T[(size_t)i * ldb + c];
                const double bb = MIRRORS ? s_bcol[i] : Tb[(size_t)i * ldb];
                s_pcol[i] = a;                               // the old pivot column, on the way
                if (a != 0.0) {
                    const double v = bb / a;
                    if (i < f.idx) {
                        f.idx = i;
                        f.v = v;
                    }
                    if (!isnan(v)) {
                        const Cand x = classify(v, i);
                        bc = cand_sel(better(x, bc), x, bc);
                    }
                }
            }
            have_col = true;
            f = wave_first(f);
            bc = wave_best(bc);
            if (lane == 0) {
                s_f[wid] = f;
                s_c[wid] = bc;
            }
            __syncthreads();
            f = First{SMX_NONE, 0.0};
            bc = cand_none();
            if (lane < nw) {
                f = s_f[lane];
                bc = s_c[lane];
            }
            f = wave_first(f);
            bc = wave_best(bc);
            if (f.idx == SMX_NONE) {
                status = SMX_NOT_CONVERGE;
                break;
            }
            if (isnan(f.v)) {
                r = f.idx;
            } else if (bc.cls >= 2) {
                status = SMX_NOT_CONVERGE;
                break;
            } else {
                r = bc.idx;
            }
        }
        // the Jordan step (simplex.py:149-177) in place: every right-hand side is the OLD table,
        // so the old pivot row and pivot column (with e) leave the table first
        for (int j = tid; j < C; j += nt) s_prow[j] = T[(size_t)r * ldb + j];
        for (int i = have_col ? n + tid : tid; i < R; i += nt) s_pcol[i] = T[(size_t)i * ldb + c];
        __syncthreads();
        const double e = s_pcol[r];
        const size_t hs = (size_t)b * max_pivots + step;
        double* snap = snaps ? snaps + hs * tab_elems : nullptr;
        for (int i = i0, j = j0; i < R;) {
            double t[U];
            int ui[U], uj[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {                    // every load of the group first
                ui[u] = i;
                uj[u] = j;
                t[u] = 0.0;
                if (i < R) {
                    t[u] = T[(size_t)i * ldb + j];
                    i += di;
                    j += dj;
                    if (j >= C) {
                        j -= C;
                        ++i;
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (ui[u] >= R) break;                       // the walk ended inside the group
                const int ei = ui[u], ej = uj[u];
                const size_t at = (size_t)ei * ldb + ej;
                double num;
                if (ei == r) {
                    num = (ej == c) ? 1.0 : -t[u];
                } else {
                    const double t1 = t[u] * e;
                    const double t2 = s_prow[ej] * s_pcol[ei];
                    num = (ej == c) ? t[u] : (t1 - t2);
                }
                const double v = num / e;
                T[at] = v;
                if (MIRRORS) {
                    if (ej == m) s_bcol[ei] = v;
                    if (ei == n) s_frow[ej] = v;
                }
                if (snap) snap[at] = v;
            }
        }
        __syncthreads();
        p1 = move_label(p1, r, c);
        p2 = move_label(p2, r, c);
        if (tid == 0) {
            rc[2 * hs] = r;
            rc[2 * hs + 1] = c;
            xv[2 * hs] = (p1 >= 0) ? (MIRRORS ? s_bcol[p1] : Tb[(size_t)p1 * ldb]) : 0.0;
            xv[2 * hs + 1] = (p2 >= 0) ? (MIRRORS ? s_bcol[p2] : Tb[(size_t)p2 * ldb]) : 0.0;
        }
        ++np;
    }
    if (tid == 0) {
        status_out[b] = status;
        np_out[b] = np;
    }
}

// Host: one launch of the instance (MIRRORS, U) with `block` threads per LP.  max_lds is the
// envelope's largest dynamic LDS; the thinnest shapes pass the 64 KiB default, so each instance
// raises its limit once.
using GmLaunch = int(int, int, const double*, const int32_t*, int, int, int, int, double*,
                     int32_t*, double*, double*, int32_t*, int32_t*, hipStream_t);

template <bool MIRRORS, int U>
int launch_batch_gm(int block, int max_lds, const double* tabs, const int32_t* dims, int B,
                    int Rmax, int ldb, int max_pivots, double* out, int32_t* rc, double* xv,
                    double* snaps, int32_t* status, int32_t* npivots, hipStream_t st) {
    static const hipError_t attr_err = hipFuncSetAttribute(
        (const void*)k_batch_gm<MIRRORS, U>, hipFuncAttributeMaxDynamicSharedMemorySize, max_lds);
    if (attr_err != hipSuccess) return (int)attr_err;
    hipLaunchKernelGGL((k_batch_gm<MIRRORS, U>), dim3(B), dim3(block),
                       (size_t)(MIRRORS ? 16 : 8) * ((size_t)Rmax + ldb), st, tabs, dims, B, Rmax, ldb, max_pivots,
                       out, rc, xv, snaps, status, npivots);
    return (int)hipGetLastError();
}

}  // namespace
