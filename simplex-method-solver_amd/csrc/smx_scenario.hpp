// smx_scenario.hpp -- what-if scenarios of a final table: the table a warm re-solve starts from
// when constants and costs of the original LP move.  k_batch_scenario (one workgroup per scenario,
// after k_batch_solution) and host_scenario (one table on the host) share the update steps below,
// so the arithmetic is stated once.
// Part of libsmx (compiled as one translation unit by smx_kernels.hip; not a standalone header).
//
// The contract (include/smx.h).  T is a final table ([n+1][m+1], f-row = row n, "-b" =
// column m) under the labels basis[p] / nonbasis[j] (k < m is 'x{k+1}', m + i is 'y{i+1}'); a
// scenario adds drhs[i] to the constant t_i and dcost[k] to function[k].  A delta that compares
// equal to zero is skipped (a NaN delta is not equal to zero and is applied).  The scenario table
// S is T with row n and column m replaced; every product rounded on its own, every sum strictly in
// the stated order, no FMA:
//   1. f-row, every column j = 0..m:   v = T[n][j];
//        j < m and nonbasis[j] = k < m:            v = v + dcost[k]
//        p = 0..n-1 ascending, basis[p] = k < m:   v = v + dcost[k] * T[p][j]
//        S[n][j] = v
//   2. "-b" column, every row p = 0..n (row n reads step 1's S[n][.]):   v = S[p][m];
//        p < n and basis[p] = m + i:               v = v + drhs[i]
//        j = 0..m-1 ascending, nonbasis[j] = m + i: v = v - S[p][j] * drhs[i]
//        S[p][m] = v
// A code outside 0..n+m-1 names nothing.  func_s[k] = function[k] + dcost[k] (a zero delta
// skipped), +0.0 at k >= m.
#pragma once
#pragma clang fp contract(off)

namespace {

constexpr int kScnBlock = 256;
constexpr int kScnWaves = kScnBlock / kWave;

// The delta the label `code` names in `vec` when it lies in [lo, hi), else +0.0: nothing to apply.
__host__ __device__ __forceinline__ double scn_delta(int code, int lo, int hi, const double* vec) {
    return (code >= lo && code < hi) ? vec[code - lo] : 0.0;
}
// v + d for the entry the changed label stands over itself (and the func_s add)
__host__ __device__ __forceinline__ double scn_own(double v, double d) {
    return d != 0.0 ? v + d : v;
}
// step 1, one row: v + dc * t
__host__ __device__ __forceinline__ double scn_cost_term(double v, double dc, double t) {
    return dc != 0.0 ? v + dc * t : v;
}
// step 2, one column: v - s * d
__host__ __device__ __forceinline__ double scn_rhs_term(double v, double s, double d) {
    return d != 0.0 ? v - s * d : v;
}

// ---------------------------------------------------------------------------------------------
// k_batch_scenario: one 256-thread workgroup per scenario q = b * S + s (grid = B * S), after
// k_batch_solution, whose basis [B][Rmax] and nonbasis [B][ldb] it reads beside final, dims and the
// original objective rows func [B][ldb].  drhs [B][S][Rmax], dcost [B][S][ldb].  Outputs tabs_s
// [B*S][Rmax][ldb], func_s [B*S][ldb], dims_s [B*S][3] (dims of LP b).  An LP whose dims lie
// outside the block gets T's block copied and func_s of +0.0.
//
//   copy    the whole Rmax x ldb block, padding included, by a flat coalesced walk; a workgroup
//           barrier separates it from the writes of the two steps to row n and column m
//   step 1  lane = column: wave w takes the tiles of 64 columns w, w + 4, ...; the rows are walked
//           in chunks of 64 whose labels and deltas the lanes load together, a ballot names the rows
//           with a delta and only those rows are read (a wave-uniform loop: the row index and its
//           delta are scalars), so a wave reads 64 consecutive doubles of each such row
//   step 2  lane = row: wave w takes the blocks of 64 rows w, w + 4, ...; the columns are walked
//           in chunks of 64 in the same way and only the columns over a changed slack are read,
//           straight from the base table (row n from tabs_s, after a second barrier)
// No LDS, no scratch: the running sums are one register per lane.
__global__ __launch_bounds__(kScnBlock) void k_batch_scenario(
    const double* __restrict__ final, const int32_t* __restrict__ dims, int B, int S, int Rmax,
    int ldb, const int32_t* __restrict__ basis, const int32_t* __restrict__ nonbasis,
    const double* __restrict__ func, const double* __restrict__ drhs,
    const double* __restrict__ dcost, double* tabs_s, double* __restrict__ func_s,
    int32_t* __restrict__ dims_s) {
    const int q = blockIdx.x;
    const int b = q / S;
    if (b >= B) return;
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = dims[3 * b], m = dims[3 * b + 1];
    const double* T = final + (size_t)b * Rmax * ldb;
    double* So = tabs_s + (size_t)q * Rmax * ldb;
    const int cnt = Rmax * ldb;                              // Rmax + ldb <= 8192: below 2^25
#pragma unroll 4
    for (int e = tid; e < cnt; e += kScnBlock) So[e] = T[e];
    if (tid < 3) dims_s[3 * (size_t)q + tid] = dims[3 * b + tid];
    const bool inside = n >= 1 && m >= 1 && n < Rmax && m < ldb;
    const double* fb = func + (size_t)b * ldb;
    const double* dc = dcost + (size_t)q * ldb;
    const double* dr = drhs + (size_t)q * Rmax;
    double* fs = func_s + (size_t)q * ldb;
    for (int k = tid; k < ldb; k += kScnBlock)
        fs[k] = (inside && k < m) ? scn_own(fb[k], dc[k]) : 0.0;
    if (!inside) return;                                     // the whole workgroup alike
    __syncthreads();                                         // the copy before the two steps
    const int32_t* bb = basis + (size_t)b * Rmax;
    const int32_t* nb = nonbasis + (size_t)b * ldb;
    const double* Tf = T + (size_t)n * ldb;
    double* Sf = So + (size_t)n * ldb;

    // ---- step 1: costs -> f-row
    for (int j0 = wid * kWave; j0 <= m; j0 += kScnBlock) {
        const int j = j0 + lane;
        const bool on = j <= m;
        double v = on ? Tf[j] : 0.0;
        if (j < m) v = scn_own(v, scn_delta(nb[j], 0, m, dc));
        for (int p0 = 0; p0 < n; p0 += kWave) {
            const int p = p0 + lane;
            const double d = p < n ? scn_delta(bb[p], 0, m, dc) : 0.0;
            unsigned long long mask = __ballot(d != 0.0);
            while (mask) {
                const int l = __builtin_ctzll(mask);
                mask &= mask - 1;
                const double t = on ? T[(size_t)(p0 + l) * ldb + j] : 0.0;
                v = scn_cost_term(v, readlane_d(d, l), t);
            }
        }
        if (on) Sf[j] = v;
    }
    __syncthreads();                                         // row n of S before step 2 reads it

    // ---- step 2: constants -> "-b" column
    for (int p0 = wid * kWave; p0 <= n; p0 += kScnBlock) {
        const int p = p0 + lane;
        const bool on = p <= n;
        const double* row = p < n ? T + (size_t)p * ldb : Sf;
        double v = on ? row[m] : 0.0;
        if (p < n) v = scn_own(v, scn_delta(bb[p], m, m + n, dr));
        for (int j0 = 0; j0 < m; j0 += kWave) {
            const int j = j0 + lane;
            const double d = j < m ? scn_delta(nb[j], m, m + n, dr) : 0.0;
            unsigned long long mask = __ballot(d != 0.0);
            while (mask) {
                const int l = __builtin_ctzll(mask);
                mask &= mask - 1;
                const double s = on ? row[j0 + l] : 0.0;
                v = scn_rhs_term(v, s, readlane_d(d, l));
            }
        }
        if (on) So[(size_t)p * ldb + m] = v;
    }
}

// The same rule as a plain loop over one host table with leading dimension ld; S [n+1][ld_out]
// receives columns 0..m of every row, func_out [m] the scenario's cost vector.
void host_scenario(const double* T, int64_t ld, int n, int m, const int32_t* basis,
                   const int32_t* nonbasis, const double* func, const double* drhs,
                   const double* dcost, double* S, int64_t ld_out, double* func_out) {
    for (int p = 0; p <= n; ++p)
        for (int j = 0; j <= m; ++j) S[(int64_t)p * ld_out + j] = T[(int64_t)p * ld + j];
    for (int j = 0; j <= m; ++j) {
        double v = T[(int64_t)n * ld + j];
        if (j < m) v = scn_own(v, scn_delta(nonbasis[j], 0, m, dcost));
        for (int p = 0; p < n; ++p)
            v = scn_cost_term(v, scn_delta(basis[p], 0, m, dcost), T[(int64_t)p * ld + j]);
        S[(int64_t)n * ld_out + j] = v;
    }
    for (int p = 0; p <= n; ++p) {
        double* row = S + (int64_t)p * ld_out;
        double v = row[m];
        if (p < n) v = scn_own(v, scn_delta(basis[p], m, m + n, drhs));
        for (int j = 0; j < m; ++j)
            v = scn_rhs_term(v, row[j], scn_delta(nonbasis[j], m, m + n, drhs));
        row[m] = v;
    }
    for (int k = 0; k < m; ++k) func_out[k] = scn_own(func[k], dcost[k]);
}

}  // namespace
