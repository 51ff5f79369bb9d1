// smx_batch_wg.hpp -- the get_solution loop of one workgroup on one LP (wg_pivot_loop), shared by
// k_batch_wg here and k_batch_gm (smx_batch_gm.hpp), and k_batch_wg (many mid-sized LPs, one
// workgroup each, tableau in LDS)
// Part of libsmx (compiled as one translation unit by smx_kernels.hip; not a standalone header).
#pragma once
#pragma clang fp contract(off)

namespace {

constexpr int kWgMaxBlock = 1024;
constexpr int kWgMaxWaves = kWgMaxBlock / kWave;

__device__ __forceinline__ int wg_merge_min(const int* s, int nw, int lane) {
    return wave_min_int(lane < nw ? s[lane] : SMX_NONE);
}

// A thread's walk over the R x C elements of a table: element tid, then nt elements further each
// time, as a flat index over (row, column).  Lanes run along columns and wrap into the next row,
// waves advance down the rows, so global and LDS accesses are contiguous and a 66-column row does
// not leave 62 lanes of a second pass idle.  Built once per kernel (two divisions) and copied per
// pass: for (WgWalk w = w0; w.i < R; w.next()).
struct WgWalk {
    int i, j, di, dj, C;
    __device__ __forceinline__ WgWalk(int tid, int nt, int C_)
        : i(tid / C_), j(tid - i * C_), di(nt / C_), dj(nt - di * C_), C(C_) {}
    __device__ __forceinline__ void next() {
        i += di;
        j += dj;
        if (j >= C) {
            j -= C;
            ++i;
        }
    }
};

// This workgroup's LP: false when it has none (past the batch) or when the LP lies outside the
// launch's padding, which is reported as SMX_IDLE.
struct WgLp {
    int n, m, flen;
};

__device__ __forceinline__ bool wg_lp(const int32_t* __restrict__ dims, int B, int Rmax, int ldb,
                                      int32_t* __restrict__ status_out,
                                      int32_t* __restrict__ np_out, WgLp& lp) {
    const int b = blockIdx.x;
    if (b >= B) return false;
    lp = WgLp{dims[3 * b], dims[3 * b + 1], dims[3 * b + 2]};
    if (lp.n < 1 || lp.m < 1 || lp.n + 1 > Rmax || lp.m + 1 > ldb) {
        if (threadIdx.x == 0) {
            status_out[b] = SMX_IDLE;
            np_out[b] = 0;
        }
        return false;
    }
    return true;
}

// ---------------------------------------------------------------------------------------------
// wg_pivot_loop: the whole get_solution loop (simplex.py:184-198) of one workgroup on its LP's
// (n+1) x (m+1) working table T, row pitch ld, in place.  T is LDS for k_batch_wg and global
// memory for k_batch_gm; a table of either envelope holds under 2^31 elements, so element offsets
// are int.  s_prow[m+1] and s_pcol[n+1] (LDS) take the old pivot row and column of a step;
// rc, xv, snap (row pitch ldb, tab_elems per step; may be null) are this LP's outputs, and
// status_out / np_out its two result words.
//
// Per step the decision is k_batch's (smx_batch.hpp), each candidate set reduced over the
// workgroup: wave reduction, per-wave partials in LDS, one barrier, and the partials merged by a
// wave.  Every wave runs that merge on the same partials, so every thread holds (status, r, c)
// read from LDS, the loop exit is uniform and no second barrier is needed to broadcast it.
//
// What differs between the callers is compile time:
//   U        elements of the thread's walk whose loads are issued before the first division of
//            the update, so that one workgroup alone does not wait out a global-memory round trip
//            per element; 1 (load, divide, store, element by element) for LDS.
//   MIRRORS  s_frow[m+1], s_bcol[n+1] mirror the f-row and the "-b" column: a mirror entry is
//            written by the thread that writes that table element, with the same value, so the
//            two scans of a step and the ratio test's "-b" operand never walk a column of T.
//            Without it both pointers are unused.
//   STASH    the ratio test leaves the pivot column it reads in s_pcol on the way, which saves a
//            second walk down that column of T.
//   RULE     the selection rule (include/smx.h).  Under SMX_RULE_DUAL a step with a negative "-b"
//            and no negative f-row entry (nb and nf are reduced together anyway) and flen >= m is
//            a dual step: one pass over row r in which each thread keeps the best (NaN-ness, q, j)
//            of its columns, q = f[j] / T[r][j] (the f-row operand from s_frow with MIRRORS), then
//            the wave reduction, partials in s_c, one barrier and the merge by every wave, as the
//            ratio test does.  It takes the place of phase 1's first-positive scan; no LDS is
//            added.  Every other step, and every step under SMX_RULE_REFERENCE, is the code below
//            unchanged.
//
// Between threads: during the update every element is read and written by one thread and every
// right-hand side comes from s_prow / s_pcol.  What a thread wrote is read by other threads of the
// same workgroup only after a __syncthreads(), which orders LDS and global memory at workgroup
// scope; T is a plain pointer (no const __restrict__), so no load is hoisted over a barrier or
// served from a read-only path.  An LP never spans workgroups: no flags, no spinning, no
// co-residency.
template <int U, bool MIRRORS, bool STASH, int RULE>
__device__ __forceinline__ void wg_pivot_loop(
    double* T, int ld, double* s_prow, double* s_pcol, double* s_frow, double* s_bcol,
    const WgLp lp, const WgWalk w0, int max_pivots, int32_t* __restrict__ rc,
    double* __restrict__ xv, double* __restrict__ snap, int ldb, size_t tab_elems,
    int32_t* __restrict__ status_out, int32_t* __restrict__ np_out) {
    __shared__ int s_nb[kWgMaxWaves];
    __shared__ int s_nf[kWgMaxWaves];
    __shared__ int s_p1[kWgMaxWaves];
    __shared__ First s_f[kWgMaxWaves];
    __shared__ Cand s_c[kWgMaxWaves];
    const int tid = threadIdx.x;
    const int nt = blockDim.x;
    const int lane = tid & (kWave - 1);
    const int wid = tid >> 6;
    const int nw = nt >> 6;
    const int n = lp.n, m = lp.m, flen = lp.flen;
    const int R = n + 1, C = m + 1;
    const int fscan = flen < m ? flen : m;
    int p1 = (m >= 1) ? -1 : SMX_ABSENT;   // label positions of 'x1', 'x2' (simplex.py:30)
    int p2 = (m >= 2) ? -2 : SMX_ABSENT;
    int status = SMX_PIVOT;
    int np = 0;
    const double* Tb = T + m;                    // the "-b" column
    const double* Tf = T + n * ld;               // the f-row
    for (int step = 0; step < max_pivots; ++step) {
        // first row with b < 0 (simplex.py:72-76) and first f-row entry < 0 (:94-98) together
        int nb = SMX_NONE, nf = SMX_NONE;
        for (int i = tid; i < n; i += nt) {
            if ((MIRRORS ? s_bcol[i] : Tb[i * ld]) < 0.0) {
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
            const double* rowp = T + r * ld;
            if (RULE == SMX_RULE_DUAL && (nf == SMX_NONE && flen >= m)) {   // a dual step
                Cand bq = cand_none();
                for (int j = tid; j < m; j += nt) {
                    const double a = rowp[j];
                    if (a > 0.0) {
                        const Cand x = dual_cand((MIRRORS ? s_frow[j] : Tf[j]) / a, j);
                        bq = cand_sel(dual_better(x, bq), x, bq);
                    }
                }
                bq = wave_dual(bq);
                if (lane == 0) s_c[wid] = bq;
                __syncthreads();
                bq = cand_none();
                if (lane < nw) bq = s_c[lane];
                c = wave_dual(bq).idx;
            } else {
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
            }
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
                const double a = T[i * ld + c];
                const double bb = MIRRORS ? s_bcol[i] : Tb[i * ld];
                if (STASH) s_pcol[i] = a;                    // the old pivot column, on the way
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
            have_col = STASH;
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
        for (int j = tid; j < C; j += nt) s_prow[j] = T[r * ld + j];
        for (int i = have_col ? n + tid : tid; i < R; i += nt) s_pcol[i] = T[i * ld + c];
        __syncthreads();
        const double e = s_pcol[r];
        double* sn = snap ? snap + step * tab_elems : nullptr;
        // one element: t is the old T[i][j]; the new value goes to the table, its mirrors and
        // the snapshot
        const auto put = [&](int i, int j, double t) {
            double num;
            if (i == r) {
                num = (j == c) ? 1.0 : -t;
            } else {
                const double t1 = t * e;
                const double t2 = s_prow[j] * s_pcol[i];
                num = (j == c) ? t : (t1 - t2);
            }
            const double v = num / e;
            T[i * ld + j] = v;
            if (MIRRORS) {
                if (j == m) s_bcol[i] = v;
                if (i == n) s_frow[j] = v;
            }
            if (sn) sn[i * ldb + j] = v;
        };
        if (U == 1) {
            // written without the group arrays: through them the compiler waits for t before it
            // issues the two LDS reads of the right-hand side (3.5 % of k_batch_wg)
            for (WgWalk w = w0; w.i < R; w.next()) put(w.i, w.j, T[w.i * ld + w.j]);
        } else {
            for (WgWalk w = w0; w.i < R;) {
                double t[U];
                int ui[U], uj[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {                // every load of the group first
                    ui[u] = w.i;
                    uj[u] = w.j;
                    t[u] = 0.0;
                    if (w.i < R) {
                        t[u] = T[w.i * ld + w.j];
                        w.next();
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (ui[u] >= R) break;                   // the walk ended inside the group
                    put(ui[u], uj[u], t[u]);
                }
            }
        }
        __syncthreads();
        p1 = move_label(p1, r, c);
        p2 = move_label(p2, r, c);
        if (tid == 0) {
            rc[2 * step] = r;
            rc[2 * step + 1] = c;
            xv[2 * step] = (p1 >= 0) ? (MIRRORS ? s_bcol[p1] : Tb[p1 * ld]) : 0.0;
            xv[2 * step + 1] = (p2 >= 0) ? (MIRRORS ? s_bcol[p2] : Tb[p2 * ld]) : 0.0;
        }
        ++np;
    }
    if (tid == 0) {
        *status_out = status;
        *np_out = np;
    }
}

// ---------------------------------------------------------------------------------------------
// k_batch_wg: the LPs one row or one column past k_batch's wavefront envelope, up to what one
// CU's LDS holds.  One workgroup per LP: the table goes into LDS at row pitch ldl (odd: a walk
// down the pivot column or the "-b" column touches 32 different bank pairs per 32-lane group),
// wg_pivot_loop runs on it in one launch, and the final table goes to out.
//
// Dynamic LDS: s_T[Rmax * ldl], s_prow[ldb], s_pcol[Rmax] -- wg_lds_bytes() on the host is the
// only place that sizes it.  RULE is wg_pivot_loop's.
template <int RULE>
__global__ __launch_bounds__(kWgMaxBlock) void k_batch_wg(
    const double* __restrict__ tabs, const int32_t* __restrict__ dims, int B, int Rmax, int ldb,
    int ldl, int max_pivots, double* __restrict__ out, int32_t* __restrict__ rc,
    double* __restrict__ xv, double* __restrict__ snaps, int32_t* __restrict__ status_out,
    int32_t* __restrict__ np_out) {
    extern __shared__ double s_wg[];   // s_T[Rmax * ldl], s_prow[ldb], s_pcol[Rmax]
    double* s_T = s_wg;
    double* s_prow = s_T + (size_t)Rmax * ldl;
    double* s_pcol = s_prow + ldb;
    WgLp lp;
    if (!wg_lp(dims, B, Rmax, ldb, status_out, np_out, lp)) return;
    const int b = blockIdx.x;
    const int R = lp.n + 1;
    const size_t tab_elems = (size_t)Rmax * ldb;
    const size_t hs = (size_t)b * max_pivots;
    const WgWalk w0(threadIdx.x, blockDim.x, lp.m + 1);
    const double* src = tabs + (size_t)b * tab_elems;
    for (WgWalk w = w0; w.i < R; w.next()) s_T[w.i * ldl + w.j] = src[w.i * ldb + w.j];
    __syncthreads();
    wg_pivot_loop<1, false, false, RULE>(
        s_T, ldl, s_prow, s_pcol, nullptr, nullptr, lp, w0, max_pivots, rc + 2 * hs, xv + 2 * hs,
        snaps ? snaps + hs * tab_elems : nullptr, ldb, tab_elems, status_out + b, np_out + b);
    double* dst = out + (size_t)b * tab_elems;
    for (WgWalk w = w0; w.i < R; w.next()) dst[w.i * ldb + w.j] = s_T[w.i * ldl + w.j];
}

// Host: raise a kernel's dynamic-LDS limit to max_lds, once per kernel (the thinnest shapes of
// both envelopes pass the 64 KiB default).
template <auto Kernel>
int wg_raise_lds_limit(int max_lds) {
    static const hipError_t err = hipFuncSetAttribute(
        (const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, max_lds);
    return (int)err;
}

}  // namespace
