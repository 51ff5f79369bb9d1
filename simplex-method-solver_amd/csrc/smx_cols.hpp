// smx_cols.hpp -- new variables on a solved LP: the table a warm re-solve starts from when columns
// are added to the original problem.  k_batch_cols (one workgroup per column set, after
// k_batch_solution) and host_cols (one table on the host) form every sum with scn_delta and
// scn_rhs_term of smx_scenario.hpp, so the arithmetic is stated once: a new column is step 2 of a
// scenario whose "constants" are the column's coefficients.
// Part of libsmx (compiled as one translation unit by smx_kernels.hip; not a standalone header).
//
// The contract (include/smx.h).  T is a final table ([n+1][m+1], f-row = row n, "-b" =
// column m) under the labels basis[p] / nonbasis[j] (k < m is 'x{k+1}', m + i is 'y{i+1}'); a new
// variable is a vector a[0..n]: a[i], i < n, its coefficient in constraint i of the ORIGINAL
// problem, a[n] its entry in `function`.  The widened table W of K' columns has T's columns
// 0..m-1, the new columns m..m+K'-1 and T's column m as column m+K'.  New column kappa, every row
// p = 0..n; every product rounded on its own, the sum strictly in this order, no FMA:
//   v = a[basis[p] - m] if p < n and m <= basis[p] < m + n (the column's own bits), a[n] if p == n,
//       else +0.0
//   j = 0..m-1 ascending, nonbasis[j] = m + i with 0 <= i < n and a[i] != 0:   v = v - T[p][j] * a[i]
//   W[p][m+kappa] = v
// A code outside 0..n+m-1 names nothing.  Labels are recoded as if the variables had been appended
// to the original: c < m stays, m + i becomes m + K' + i, new column kappa is m + kappa, anything
// else -1.
#pragma once
#pragma clang fp contract(off)

namespace {

constexpr int kColBlock = 256;
constexpr int kColWaves = kColBlock / kWave;
constexpr int kColPass = 4;               // new columns whose sums one walk over T's columns feeds

// The code a base label has in the LP widened by kc variables, -1 for a code that names nothing.
__host__ __device__ __forceinline__ int32_t col_recode(int code, int n, int m, int kc) {
    return (code >= 0 && code < m) ? code : ((code >= m && code < m + n) ? code + kc : -1);
}

// ---------------------------------------------------------------------------------------------
// k_batch_cols: one 256-thread workgroup per column set q = b * S + s (grid = B * S), after
// k_batch_solution, whose basis [B][Rmax] and nonbasis [B][ldb] it reads beside final, dims and the
// original objective rows func [B][ldb].  cols [B][S][K][Rmax] (entry n_b the cost), ncols [B][S].
// Outputs tabs_v [B*S][Rmax][ldb_out], func_v [B*S][ldb_out], dims_v [B*S][3], basis_v
// [B*S][Rmax], nonbasis_v [B*S][ldb_out]; ldb_out >= ldb (the host checks it).  A set that is not
// taken (ncols outside 0..K, m + ncols >= ldb_out, flen < m) counts 0 columns; an LP whose dims lie
// outside the block is handled as m = ldb - 1 without columns, keeps its dims and gets labels -1
// and func_v +0.0.
//
// Every element of the output block is written exactly once and nothing is read back from it, so
// there is no barrier:
//   relayout     a flat coalesced walk over the Rmax x ldb_out block: columns 0..m-1 from T, column
//                m + K' from T's column m, +0.0 past it and in the new columns' rows past n; the
//                new columns' rows 0..n are left to their sums
//   new columns  lane = row: an item is (pass of kColPass columns, block of 64 rows), the waves
//                take the items w, w + 4, ...  The columns of T are walked in chunks of 64 whose
//                labels the lanes load together with the pass's coefficients on them; a ballot per
//                new column names the T columns over a slack with a coefficient, and one
//                wave-uniform loop over the union reads each such column once (one element a lane,
//                a stride of ldb) for all new columns of the pass.  A coefficient is a scalar, so
//                a new column that skips a T column branches uniformly and its sum keeps ascending j.
// No LDS, no scratch: kColPass running sums per lane.
__global__ __launch_bounds__(kColBlock) void k_batch_cols(
    const double* __restrict__ final, const int32_t* __restrict__ dims, int B, int S, int Rmax,
    int ldb, const int32_t* __restrict__ basis, const int32_t* __restrict__ nonbasis,
    const double* __restrict__ func, const double* __restrict__ cols,
    const int32_t* __restrict__ ncols, int K, int ldb_out, double* __restrict__ tabs_v,
    double* __restrict__ func_v, int32_t* __restrict__ dims_v, int32_t* __restrict__ basis_v,
    int32_t* __restrict__ nonbasis_v) {
    const int q = blockIdx.x;
    const int b = q / S;
    if (b >= B) return;
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n0 = dims[3 * b], m0 = dims[3 * b + 1], flen = dims[3 * b + 2];
    const bool inside = n0 >= 1 && m0 >= 1 && n0 < Rmax && m0 < ldb;
    const int n = inside ? n0 : Rmax - 1;                    // rows above the f-row
    const int m = inside ? m0 : ldb - 1;                     // the "-b" column
    int kc = ncols[q];
    if (!inside || kc < 0 || kc > K || m + kc >= ldb_out || flen < m) kc = 0;
    const double* T = final + (size_t)b * Rmax * ldb;
    double* W = tabs_v + (size_t)q * Rmax * ldb_out;
    const int32_t* bb = basis + (size_t)b * Rmax;
    const int32_t* nb = nonbasis + (size_t)b * ldb;
    const double* A = cols + (size_t)q * K * Rmax;

    if (tid < 3) dims_v[3 * (size_t)q + tid] = dims[3 * b + tid] + (tid == 0 ? 0 : kc);
    int32_t* bv = basis_v + (size_t)q * Rmax;
    for (int i = tid; i < Rmax; i += kColBlock)
        bv[i] = (inside && i < n) ? col_recode(bb[i], n, m, kc) : -1;
    int32_t* nv = nonbasis_v + (size_t)q * ldb_out;
    const double* fb = func + (size_t)b * ldb;
    double* fv = func_v + (size_t)q * ldb_out;
    for (int j = tid; j < ldb_out; j += kColBlock) {
        const bool old = inside && j < m, fresh = j >= m && j < m + kc;     // kc > 0: inside
        nv[j] = old ? col_recode(nb[j], n, m, kc) : (fresh ? j : -1);       // m + kappa at j
        fv[j] = old ? fb[j] : (fresh ? A[(size_t)(j - m) * Rmax + n] : 0.0);
    }

    // ---- relayout: Rmax + ldb_out <= 8192, so every count below is under 2^25
    {
        const int dp = kColBlock / ldb_out, dj = kColBlock % ldb_out;
        const int last = m + kc;
        int p = tid / ldb_out, j = tid % ldb_out;
        while (p < Rmax) {
            const double* row = T + (size_t)p * ldb;
            double* out = W + (size_t)p * ldb_out;
            if (j < m) out[j] = row[j];
            else if (j == last) out[j] = row[m];
            else if (j > last || p > n) out[j] = 0.0;
            p += dp;
            j += dj;
            if (j >= ldb_out) {
                j -= ldb_out;
                ++p;
            }
        }
    }
    if (kc == 0) return;                                     // the whole workgroup alike

    // ---- new columns
    const int nblocks = (n + kWave) / kWave;                 // rows 0..n
    const int npass = (kc + kColPass - 1) / kColPass;
    for (int it = wid; it < npass * nblocks; it += kColWaves) {
        const int c0 = (it / nblocks) * kColPass;
        const int p = (it % nblocks) * kWave + lane;
        const int cnt = kc - c0 < kColPass ? kc - c0 : kColPass;
        const bool on = p <= n;
        const int code = p < n ? bb[p] : -1;
        const double* row = T + (size_t)(on ? p : n) * ldb;
        const double* a[kColPass];
        double v[kColPass];
#pragma unroll
        for (int c = 0; c < kColPass; ++c) {
            a[c] = A + (size_t)(c0 + (c < cnt ? c : 0)) * Rmax;
            v[c] = p == n ? a[c][n] : scn_delta(code, m, m + n, a[c]);
        }
        for (int j0 = 0; j0 < m; j0 += kWave) {
            const int lab = j0 + lane < m ? nb[j0 + lane] : -1;
            double d[kColPass];
            unsigned long long mask[kColPass], any = 0ull;
#pragma unroll
            for (int c = 0; c < kColPass; ++c) {
                d[c] = c < cnt ? scn_delta(lab, m, m + n, a[c]) : 0.0;
                mask[c] = __ballot(d[c] != 0.0);
                any |= mask[c];
            }
            while (any) {
                const int l = __builtin_ctzll(any);
                any &= any - 1;
                const double t = row[j0 + l];
#pragma unroll
                for (int c = 0; c < kColPass; ++c)
                    if ((mask[c] >> l) & 1ull) v[c] = scn_rhs_term(v[c], t, readlane_d(d[c], l));
            }
        }
        if (on) {
#pragma unroll
            for (int c = 0; c < kColPass; ++c)
                if (c < cnt) W[(size_t)p * ldb_out + m + c0 + c] = v[c];
        }
    }
}

// The same rule as a plain loop over one host table with leading dimension ld; A [K][n+1], W
// [n+1][ld_out] receives columns 0..m+K of every row, basis_out [n] and nonbasis_out [m+K] the
// recoded labels.
void host_cols(const double* T, int64_t ld, int n, int m, const int32_t* basis,
               const int32_t* nonbasis, const double* A, int K, double* W, int64_t ld_out,
               int32_t* basis_out, int32_t* nonbasis_out) {
    for (int p = 0; p <= n; ++p) {
        const double* row = T + (int64_t)p * ld;
        double* out = W + (int64_t)p * ld_out;
        for (int j = 0; j < m; ++j) out[j] = row[j];
        out[m + K] = row[m];
        for (int c = 0; c < K; ++c) {
            const double* a = A + (int64_t)c * (n + 1);
            double v = p == n ? a[n] : scn_delta(basis[p], m, m + n, a);
            for (int j = 0; j < m; ++j)
                v = scn_rhs_term(v, row[j], scn_delta(nonbasis[j], m, m + n, a));
            out[m + c] = v;
        }
    }
    for (int p = 0; p < n; ++p) basis_out[p] = col_recode(basis[p], n, m, K);
    for (int j = 0; j < m; ++j) nonbasis_out[j] = col_recode(nonbasis[j], n, m, K);
    for (int c = 0; c < K; ++c) nonbasis_out[m + c] = m + c;
}

}  // namespace
