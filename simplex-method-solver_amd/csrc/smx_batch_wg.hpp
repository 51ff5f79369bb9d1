// smx_batch_wg.hpp -- k_batch_wg (many mid-sized LPs, one workgroup each, tableau in LDS)
// Part of libsmx (compiled as one translation unit by smx_kernels.hip; not a standalone header).
#pragma once
#pragma clang fp contract(off)

namespace {

// ---------------------------------------------------------------------------------------------
// k_batch_wg: the LPs one row or one column past k_batch's wavefront envelope, up to what one
// CU's LDS holds.  One workgroup per LP; the whole get_solution loop (simplex.py:184-198) runs
// inside one launch on the LP's (n+1) x (m+1) table in LDS, row pitch ldl (odd: a walk down the
// pivot column or the "-b" column touches 32 different bank pairs per 32-lane group).
//
// Dynamic LDS: s_T[Rmax * ldl], s_prow[ldb], s_pcol[Rmax] -- wg_lds_bytes() on the host is the
// only place that sizes it.  Threads cover the table as a flat index over (row, column): lanes run
// along columns and wrap into the next row, waves advance down the rows, so global and LDS
// accesses are contiguous and a 66-column row does not leave 62 lanes of a second pass idle.
//
// Per step the decision is k_batch's (smx_batch.hpp:64-111), each candidate set reduced over the
// workgroup: wave reduction, per-wave partials in LDS, one barrier, and the partials merged by a
// wave.  Every wave runs that merge on the same partials, so every thread holds (status, r, c)
// read from LDS, the loop exit is uniform and no second barrier is needed to broadcast it.
constexpr int kWgMaxBlock = 1024;
constexpr int kWgMaxWaves = kWgMaxBlock / kWave;

__device__ __forceinline__ int wg_merge_min(const int* s, int nw, int lane) {
    return wave_min_int(lane < nw ? s[lane] : SMX_NONE);
}

__global__ __launch_bounds__(kWgMaxBlock) void k_batch_wg(
    const double* __restrict__ tabs, const int32_t* __restrict__ dims, int B, int Rmax, int ldb,
    int ldl, int max_pivots, double* __restrict__ out, int32_t* __restrict__ rc,
    double* __restrict__ xv, double* __restrict__ snaps, int32_t* __restrict__ status_out,
    int32_t* __restrict__ np_out) {
    extern __shared__ double s_wg[];   // s_T[Rmax * ldl], s_prow[ldb], s_pcol[Rmax]
    __shared__ int s_nb[kWgMaxWaves];
    __shared__ int s_nf[kWgMaxWaves];
    __shared__ int s_p1[kWgMaxWaves];
    __shared__ First s_f[kWgMaxWaves];
    __shared__ Cand s_c[kWgMaxWaves];
    double* s_T = s_wg;
    double* s_prow = s_T + (size_t)Rmax * ldl;
    double* s_pcol = s_prow + ldb;
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
    // this thread's walk over the R x C elements: (i0, j0), then nt elements further each time
    const int i0 = tid / C, j0 = tid - i0 * C;
    const int di = nt / C, dj = nt - di * C;
    {
        const double* src = tabs + (size_t)b * tab_elems;
        for (int i = i0, j = j0; i < R;) {
            s_T[i * ldl + j] = src[(size_t)i * ldb + j];
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
    const double* s_b = s_T + m;                 // the "-b" column
    const double* s_frow = s_T + n * ldl;        // the f-row
    for (int step = 0; step < max_pivots; ++step) {
        // first row with b < 0 (simplex.py:72-76) and first f-row entry < 0 (:94-98) together
        int nb = SMX_NONE, nf = SMX_NONE;
        for (int i = tid; i < n; i += nt) {
            if (s_b[i * ldl] < 0.0) {
                nb = i;
                break;
            }
        }
        for (int j = tid; j < fscan; j += nt) {
            if (s_frow[j] < 0.0) {
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
        if (nb != SMX_NONE) {                                // phase 1 (simplex.py:72-91)
            r = nb;
            const double* rowp = s_T + r * ldl;
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
                const double a = s_T[i * ldl + c];
                const double bb = s_b[i * ldl];
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
        for (int j = tid; j < C; j += nt) s_prow[j] = s_T[r * ldl + j];
        for (int i = tid; i < R; i += nt) s_pcol[i] = s_T[i * ldl + c];
        __syncthreads();
        const double e = s_pcol[r];
        const size_t hs = (size_t)b * max_pivots + step;
        double* snap = snaps ? snaps + hs * tab_elems : nullptr;
        for (int i = i0, j = j0; i < R;) {
            const double t = s_T[i * ldl + j];
            double num;
            if (i == r) {
                num = (j == c) ? 1.0 : -t;
            } else {
                const double t1 = t * e;
                const double t2 = s_prow[j] * s_pcol[i];
                num = (j == c) ? t : (t1 - t2);
            }
            const double v = num / e;
            s_T[i * ldl + j] = v;
            if (snap) snap[(size_t)i * ldb + j] = v;
            i += di;
            j += dj;
            if (j >= C) {
                j -= C;
                ++i;
            }
        }
        __syncthreads();
        p1 = move_label(p1, r, c);
        p2 = move_label(p2, r, c);
        if (tid == 0) {
            rc[2 * hs] = r;
            rc[2 * hs + 1] = c;
            xv[2 * hs] = (p1 >= 0) ? s_b[p1 * ldl] : 0.0;
            xv[2 * hs + 1] = (p2 >= 0) ? s_b[p2 * ldl] : 0.0;
        }
        ++np;
    }
    {
        double* dst = out + (size_t)b * tab_elems;
        for (int i = i0, j = j0; i < R;) {
            dst[(size_t)i * ldb + j] = s_T[i * ldl + j];
            i += di;
            j += dj;
            if (j >= C) {
                j -= C;
                ++i;
            }
        }
    }
    if (tid == 0) {
        status_out[b] = status;
        np_out[b] = np;
    }
}

}  // namespace
