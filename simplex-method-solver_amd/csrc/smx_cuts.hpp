// smx_cuts.hpp -- new constraints on a solved LP: the table a warm re-solve starts from when rows
// are added to the original problem.  k_batch_cuts (one workgroup per cut set, after
// k_batch_solution) and host_cuts (one table on the host) form every sum with scn_delta and
// scn_cost_term of smx_scenario.hpp, so the arithmetic is stated once: a cut row is step 1 of a
// scenario whose "costs" are the cut's coefficients.
// Part of libsmx (compiled as one translation unit by smx_kernels.hip; not a standalone header).
//
// The contract (include/smx.h).  T is a final table ([n+1][m+1], f-row = row n, "-b" =
// column m) under the labels basis[p] / nonbasis[j] (k < m is 'x{k+1}', m + i is 'y{i+1}'); a cut
// is a row g[0..m] in the format of a constraint of the ORIGINAL problem.  The extended table E of
// K' cuts has T's rows 0..n-1, the new rows n..n+K'-1 and T's f-row as row n+K'.  New row kappa,
// every column j = 0..m; every product rounded on its own, the sum strictly in this order, no FMA:
//   v = g[nonbasis[j]] if j < m and 0 <= nonbasis[j] < m (the cut's own bits), g[m] if j == m,
//       else +0.0
//   p = 0..n-1 ascending, basis[p] = k < m and g[k] != 0:   v = v + g[k] * T[p][j]
//   E[n+kappa][j] = v
// A code outside 0..n+m-1 names nothing.  The new row's label is m + n + kappa.
#pragma once
#pragma clang fp contract(off)

namespace {

constexpr int kCutBlock = 256;
constexpr int kCutWaves = kCutBlock / kWave;
constexpr int kCutPass = 4;               // cuts whose sums one walk over T's rows feeds

// ---------------------------------------------------------------------------------------------
// k_batch_cuts: one 256-thread workgroup per cut set q = b * S + s (grid = B * S), after
// k_batch_solution, whose basis [B][Rmax] and nonbasis [B][ldb] it reads beside final and dims.
// cuts [B][S][K][ldb] (entry m_b the constant), ncuts [B][S].  Outputs tabs_c
// [B*S][Rmax_out][ldb], dims_c [B*S][3], basis_c [B*S][Rmax_out]; Rmax_out >= Rmax (the host
// checks it).  A set that is not taken (ncuts outside 0..K, n + ncuts >= Rmax_out) counts 0 cuts;
// an LP whose dims lie outside the block is handled as n = Rmax - 1 without cuts and keeps its dims.
//
// Every element of the output block is written exactly once and nothing is read back from it, so
// there is no barrier:
//   copy      rows 0..n-1 by a flat coalesced walk (padding columns included), the f-row to row
//             n + K', +0.0 into the rows past it
//   new rows  lane = column: an item is (pass of kCutPass cuts, tile of 64 columns), the waves
//             take the items w, w + 4, ...  The rows of T are walked in chunks of 64 whose labels
//             the lanes load together with the pass's coefficients on them; a ballot per cut names
//             the rows with a coefficient, and one wave-uniform loop over the union reads each such
//             row once (64 consecutive doubles a wave) for all cuts of the pass.  A cut's
//             coefficient is a scalar, so a cut that skips a row branches uniformly and its sum
//             keeps ascending p.  Columns past m get +0.0.
// No LDS, no scratch: kCutPass running sums per lane.
__global__ __launch_bounds__(kCutBlock) void k_batch_cuts(
    const double* __restrict__ final, const int32_t* __restrict__ dims, int B, int S, int Rmax,
    int ldb, const int32_t* __restrict__ basis, const int32_t* __restrict__ nonbasis,
    const double* __restrict__ cuts, const int32_t* __restrict__ ncuts, int K, int Rmax_out,
    double* __restrict__ tabs_c, int32_t* __restrict__ dims_c, int32_t* __restrict__ basis_c) {
    const int q = blockIdx.x;
    const int b = q / S;
    if (b >= B) return;
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n0 = dims[3 * b], m = dims[3 * b + 1];
    const bool inside = n0 >= 1 && m >= 1 && n0 < Rmax && m < ldb;
    const int n = inside ? n0 : Rmax - 1;                    // rows above the f-row
    int kc = ncuts[q];
    if (!inside || kc < 0 || kc > K || n + kc >= Rmax_out) kc = 0;
    const double* T = final + (size_t)b * Rmax * ldb;
    double* E = tabs_c + (size_t)q * Rmax_out * ldb;
    const int32_t* bb = basis + (size_t)b * Rmax;
    const int32_t* nb = nonbasis + (size_t)b * ldb;

    if (tid < 3) dims_c[3 * (size_t)q + tid] = dims[3 * b + tid] + (tid == 0 ? kc : 0);
    int32_t* bc = basis_c + (size_t)q * Rmax_out;
    for (int i = tid; i < Rmax_out; i += kCutBlock)
        bc[i] = i < n ? bb[i] : (i < n + kc ? m + i : -1);   // m + n + kappa at i = n + kappa

    // ---- copy: Rmax_out + ldb <= 8192, so every count below is under 2^25
    const int head = n * ldb;
#pragma unroll 4
    for (int e = tid; e < head; e += kCutBlock) E[e] = T[e];
    const int frow = (n + kc) * ldb;
    for (int j = tid; j < ldb; j += kCutBlock) E[frow + j] = T[head + j];
    const int end = Rmax_out * ldb;
#pragma unroll 4
    for (int e = frow + ldb + tid; e < end; e += kCutBlock) E[e] = 0.0;
    if (kc == 0) return;                                     // the whole workgroup alike

    // ---- new rows
    const double* G = cuts + (size_t)q * K * ldb;
    const int ntiles = (ldb + kWave - 1) / kWave;
    const int npass = (kc + kCutPass - 1) / kCutPass;
    for (int it = wid; it < npass * ntiles; it += kCutWaves) {
        const int c0 = (it / ntiles) * kCutPass;
        const int j0 = (it % ntiles) * kWave;
        const int j = j0 + lane;
        const int cnt = kc - c0 < kCutPass ? kc - c0 : kCutPass;
        const bool on = j <= m;
        const int code = j < m ? nb[j] : -1;
        double v[kCutPass];
#pragma unroll
        for (int c = 0; c < kCutPass; ++c) {
            const double* g = G + (size_t)(c0 + (c < cnt ? c : 0)) * ldb;
            v[c] = j == m ? g[m] : scn_delta(code, 0, m, g);
        }
        // a tile wholly past column m has nothing to sum
        const int rows = j0 <= m ? n : 0;
        for (int p0 = 0; p0 < rows; p0 += kWave) {
            const int lab = p0 + lane < n ? bb[p0 + lane] : -1;
            double gk[kCutPass];
            unsigned long long mask[kCutPass], any = 0ull;
#pragma unroll
            for (int c = 0; c < kCutPass; ++c) {
                gk[c] = c < cnt ? scn_delta(lab, 0, m, G + (size_t)(c0 + c) * ldb) : 0.0;
                mask[c] = __ballot(gk[c] != 0.0);
                any |= mask[c];
            }
            while (any) {
                const int l = __builtin_ctzll(any);
                any &= any - 1;
                const double t = on ? T[(size_t)(p0 + l) * ldb + j] : 0.0;
#pragma unroll
                for (int c = 0; c < kCutPass; ++c)
                    if ((mask[c] >> l) & 1ull)
                        v[c] = scn_cost_term(v[c], readlane_d(gk[c], l), t);
            }
        }
        if (j < ldb) {
#pragma unroll
            for (int c = 0; c < kCutPass; ++c)
                if (c < cnt) E[(size_t)(n + c0 + c) * ldb + j] = on ? v[c] : 0.0;
        }
    }
}

// The same rule as a plain loop over one host table with leading dimension ld; G [K][m+1], E
// [n+K+1][ld_out] receives columns 0..m of every row, basis_out [n+K] the row labels.
void host_cuts(const double* T, int64_t ld, int n, int m, const int32_t* basis,
               const int32_t* nonbasis, const double* G, int K, double* E, int64_t ld_out,
               int32_t* basis_out) {
    for (int p = 0; p <= n; ++p) {
        double* row = E + (int64_t)(p < n ? p : n + K) * ld_out;
        for (int j = 0; j <= m; ++j) row[j] = T[(int64_t)p * ld + j];
    }
    for (int p = 0; p < n; ++p) basis_out[p] = basis[p];
    for (int c = 0; c < K; ++c) {
        const double* g = G + (int64_t)c * (m + 1);
        double* row = E + (int64_t)(n + c) * ld_out;
        for (int j = 0; j <= m; ++j) {
            double v = j == m ? g[m] : scn_delta(nonbasis[j], 0, m, g);
            for (int p = 0; p < n; ++p)
                v = scn_cost_term(v, scn_delta(basis[p], 0, m, g), T[(int64_t)p * ld + j]);
            row[j] = v;
        }
        basis_out[n + c] = m + n + c;
    }
}

}  // namespace
