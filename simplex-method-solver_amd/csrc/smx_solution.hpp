// smx_solution.hpp -- k_batch_solution (every LP's final table and pivot log turned into its
// solution on the device: all of x, the duals, the objective and the two label arrays)
// Part of libsmx (compiled as one translation unit by smx_kernels.hip; not a standalone header).
#pragma once
#pragma clang fp contract(off)

namespace {

constexpr int kSolWaves = 4;               // LPs per block, one wavefront each
constexpr unsigned kSolCol = 0x8000u;      // s_inv: the label stands over a column (non-basic)

// What one lane of a wave wrote to LDS, read by the other lanes of the same wave.  A wave's LDS
// instructions issue and complete in order, so the hardware needs nothing; the two fences keep the
// compiler from moving an LDS access across this point.
__device__ __forceinline__ void sol_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---------------------------------------------------------------------------------------------
// k_batch_solution: one wavefront per LP, kSolWaves LPs per block, after any of the three batch
// kernels.  Labels are int32 codes: k in 0..m-1 is 'x{k+1}', m+i is 'y{i+1}'.
//   basis[i]     label of constraint row i: m+i at the start
//   nonbasis[j]  label of column j: j at the start
//   a logged pivot (r, c) swaps basis[r] with nonbasis[c] (simplex.py:152); an entry outside
//   r < n, c < m is skipped
//   x[k]         T[i][m] where basis[i] == k, else +0.0 (find_optimum, simplex.py:51-68, for
//                every variable)
//   duals[i]     T[n][j] where nonbasis[j] == m+i, else +0.0
//   objective    p[0] + p[1] + ... + p[m-1], p[k] = func[k] * x[k]: every product rounded on its
//                own, the sum strictly left to right from p[0], no FMA
// Padding: x, duals +0.0, basis, nonbasis -1.  An LP whose dims lie outside the block gets padding
// only and objective +0.0.
//
// Dynamic LDS, private to each wave (sol_lds_bytes() on the host is the only place that sizes it):
// uint16 s_basis[Rmax], s_nonb[ldb], s_inv[Rmax + ldb] -- 4 * (Rmax + ldb) bytes; codes and
// positions stay below Rmax + ldb <= 8192 < kSolCol.  The wave loads 64 log entries at a time,
// lane 0 applies them in order; every code then stands in exactly one place, so the inverse map
// s_inv[code] (row i, or kSolCol | column j) is written once per entry with no two lanes on one
// address, and every output element is written exactly once, as a gather.  No workgroup barrier:
// a wave never reads what another wave wrote.  What a lane reads back from s_inv is range-checked
// before it indexes the table.
//
// kFrom (smx_batch_solution_from): LP b starts from the labels basis0[b / group] / nonbasis0[b /
// group] (as an earlier call wrote them) instead of the identity -- a warm run on a scenario table
// carries on from its base LP's final labels.  Every start code is range-checked before it enters
// LDS; an LP with a code outside 0..n+m-1 at i < n or j < m gets the padding values only (a wave
// ballot decides it).  Duplicate codes are the caller's error: s_inv then holds a stale or a
// contended entry, and what is read back from it is range-checked as always.
template <bool kFrom>
__global__ __launch_bounds__(kSolWaves * kWave) void k_batch_solution(
    const double* __restrict__ final, const int32_t* __restrict__ dims, int B, int Rmax, int ldb,
    int max_pivots, const int32_t* __restrict__ rc, const int32_t* __restrict__ npivots,
    const double* __restrict__ func, double* __restrict__ x, double* __restrict__ duals,
    double* __restrict__ objective, int32_t* __restrict__ basis, int32_t* __restrict__ nonbasis,
    const int32_t* __restrict__ basis0, const int32_t* __restrict__ nonbasis0, int group) {
    extern __shared__ uint16_t s_sol[];
    const int lane = threadIdx.x & (kWave - 1);
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // the LP's scalars: SGPRs
    const int b = blockIdx.x * kSolWaves + wid;
    if (b >= B) return;                          // the whole wave; nothing below spans waves
    const int n = dims[3 * b], m = dims[3 * b + 1];
    double* xb = x + (size_t)b * ldb;
    double* db = duals + (size_t)b * Rmax;
    int32_t* bb = basis + (size_t)b * Rmax;
    int32_t* nb = nonbasis + (size_t)b * ldb;
    const auto padding = [&]() {
        for (int i = lane; i < Rmax; i += kWave) {
            db[i] = 0.0;
            bb[i] = -1;
        }
        for (int j = lane; j < ldb; j += kWave) {
            xb[j] = 0.0;
            nb[j] = -1;
        }
        if (lane == 0) objective[b] = 0.0;
    };
    if (n < 1 || m < 1 || n >= Rmax || m >= ldb) {
        padding();
        return;
    }
    uint16_t* s_basis = s_sol + (size_t)wid * 2 * (Rmax + ldb);
    uint16_t* s_nonb = s_basis + Rmax;
    uint16_t* s_inv = s_nonb + ldb;
    if constexpr (kFrom) {
        const int32_t* b0 = basis0 + (size_t)(b / group) * Rmax;
        const int32_t* n0 = nonbasis0 + (size_t)(b / group) * ldb;
        bool bad = false;
        for (int i = lane; i < n; i += kWave) {
            const int code = b0[i];
            const bool ok = code >= 0 && code < n + m;
            bad |= !ok;
            s_basis[i] = (uint16_t)(ok ? code : 0);
        }
        for (int j = lane; j < m; j += kWave) {
            const int code = n0[j];
            const bool ok = code >= 0 && code < n + m;
            bad |= !ok;
            s_nonb[j] = (uint16_t)(ok ? code : 0);
        }
        if (__ballot(bad) != 0ull) {                 // the whole wave alike
            padding();
            return;
        }
    } else {
        for (int i = lane; i < n; i += kWave) s_basis[i] = (uint16_t)(m + i);
        for (int j = lane; j < m; j += kWave) s_nonb[j] = (uint16_t)j;
    }
    sol_wave_sync();
    int np = npivots[b];
    np = np < 0 ? 0 : (np > max_pivots ? max_pivots : np);
    const int32_t* log = rc + 2 * (size_t)b * max_pivots;
    for (int s0 = 0; s0 < np; s0 += kWave) {
        int r = -1, c = -1;
        if (s0 + lane < np) {
            r = log[2 * (s0 + lane)];
            c = log[2 * (s0 + lane) + 1];
        }
        const int cnt = np - s0 < kWave ? np - s0 : kWave;
        for (int q = 0; q < cnt; ++q) {
            const int rq = __builtin_amdgcn_readlane(r, q);      // q is uniform: scalars
            const int cq = __builtin_amdgcn_readlane(c, q);
            if (lane == 0 && rq >= 0 && rq < n && cq >= 0 && cq < m) {
                const uint16_t t = s_basis[rq];
                s_basis[rq] = s_nonb[cq];
                s_nonb[cq] = t;
            }
        }
    }
    sol_wave_sync();
    for (int i = lane; i < Rmax; i += kWave) {
        int code = -1;
        if (i < n) {
            code = s_basis[i];
            s_inv[code] = (uint16_t)i;
        }
        bb[i] = code;
    }
    for (int j = lane; j < ldb; j += kWave) {
        int code = -1;
        if (j < m) {
            code = s_nonb[j];
            s_inv[code] = (uint16_t)(kSolCol | (unsigned)j);
        }
        nb[j] = code;
    }
    sol_wave_sync();
    const double* T = final + (size_t)b * Rmax * ldb;
    const double* Tf = T + (size_t)n * ldb;      // the f-row
    const double* Tb = T + m;                    // the "-b" column
    for (int i = lane; i < Rmax; i += kWave) {
        double v = 0.0;
        if (i < n) {
            const unsigned w = s_inv[m + i];
            const int j = (int)(w & (kSolCol - 1));
            if ((w & kSolCol) && j < m) v = Tf[j];
        }
        db[i] = v;
    }
    const double* fb = func + (size_t)b * ldb;
    double sum = 0.0;
    for (int k0 = 0; k0 < ldb; k0 += kWave) {
        const int k = k0 + lane;
        double v = 0.0, p = 0.0;
        if (k < m) {
            const unsigned w = s_inv[k];
            if (!(w & kSolCol) && (int)w < n) v = Tb[(size_t)w * ldb];
            p = fb[k] * v;
        }
        if (k < ldb) xb[k] = v;
        // the ordered sum: the products of this chunk in lane order, by every lane alike
        const int cnt = m - k0 < kWave ? m - k0 : kWave;
        for (int q = 0; q < cnt; ++q) {
            const double pq = readlane_d(p, q);
            sum = (k0 + q == 0) ? pq : sum + pq;
        }
    }
    if (lane == 0) objective[b] = sum;
}

}  // namespace
