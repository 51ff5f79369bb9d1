// smx_ranging.hpp -- sensitivity ranging of a final table: how far a constraint's constant t_i or a
// cost function[k] can move before the basis the method stopped at changes.  k_batch_ranging (one
// workgroup per LP, after k_batch_solution) and host_ranging (one table on the host) share the
// candidate and the ordered take below, so the arithmetic is stated once.
// Part of libsmx (compiled as one translation unit by smx_kernels.hip; not a standalone header).
//
// The contract (include/smx.h).  T is the final table ([n+1][m+1], f-row = row n,
// "-b" = column m); labels are int32 codes (k < m is 'x{k+1}', m + i is 'y{i+1}'), basis[p] over
// row p and nonbasis[j] over column j.  The position of a label decides the rule:
//   row p,    basis[p] = m + i     rhs_lo[i] = T[p][m], sign bit flipped; rhs_hi[i] = +inf
//   column j, nonbasis[j] = m + i  over rows p < n: a = T[p][j], q = T[p][m] / a;
//                                  a > 0: q joins rhs_hi[i] (a minimum),
//                                  a < 0: q joins rhs_lo[i] (a maximum)
//   column j, nonbasis[j] = k < m  cost_lo[k] = T[n][j], sign bit flipped; cost_hi[k] = +inf
//   row p,    basis[p] = k < m     over columns j < m: a = T[p][j], q = (-T[n][j]) / a;
//                                  a > 0: q joins cost_lo[k] (a maximum),
//                                  a < 0: q joins cost_hi[k] (a minimum)
// A zero or NaN a is skipped.  A minimum without a candidate is +inf, a maximum -inf; one NaN
// candidate makes the bound the quiet NaN 0x7ff8000000000000; else the minimum / maximum under the
// total order in which -0.0 stands below +0.0 -- so every bound is independent of the order in
// which candidates are combined.  No FMA, `/` is the correctly rounded division.  A code outside
// 0..n+m-1 is skipped; an output element no valid code names is +0.0.
#pragma once
#pragma clang fp contract(off)

namespace {

constexpr int kRngBlock = 256;
constexpr int kRngWaves = kRngBlock / kWave;
constexpr uint64_t kRngSign = 0x8000000000000000ull;
constexpr uint64_t kRngInf = 0x7FF0000000000000ull;
constexpr uint64_t kRngNaN = 0x7FF8000000000000ull;

__host__ __device__ __forceinline__ double rng_from_bits(uint64_t u) {
    return __builtin_bit_cast(double, u);
}
__host__ __device__ __forceinline__ bool rng_signbit(double v) {
    return (__builtin_bit_cast(uint64_t, v) & kRngSign) != 0;
}
// v with its sign bit flipped (a NaN keeps its payload)
__host__ __device__ __forceinline__ double rng_flip(double v) {
    return rng_from_bits(__builtin_bit_cast(uint64_t, v) ^ kRngSign);
}
// a stands below b (neither a NaN): -0.0 below +0.0
__host__ __device__ __forceinline__ bool rng_below(double a, double b) {
    return a < b || (a == b && rng_signbit(a) && !rng_signbit(b));
}
// The ordered takes: NaN absorbs (and is made the one quiet NaN), else the total order decides.
// Associative and commutative, so partial results combine in any shape.
__host__ __device__ __forceinline__ double rng_take_min(double cur, double q) {
    const bool nan = (cur != cur) | (q != q);
    const double v = rng_below(q, cur) ? q : cur;
    return nan ? rng_from_bits(kRngNaN) : v;
}
__host__ __device__ __forceinline__ double rng_take_max(double cur, double q) {
    const bool nan = (cur != cur) | (q != q);
    const double v = rng_below(cur, q) ? q : cur;
    return nan ? rng_from_bits(kRngNaN) : v;
}
// One candidate q = num / a (one IEEE division).  pos_min: a > 0 sends q to the minimum `mn` and
// a < 0 to the maximum `mx` (the rhs rule); !pos_min the other way round (the cost rule).  A zero
// or NaN a leaves both as they are.  Branch-free: lanes of one wave take different sides.
__host__ __device__ __forceinline__ void rng_candidate(double num, double a, bool pos_min,
                                                       double& mx, double& mn) {
    const bool pos = a > 0.0, neg = a < 0.0;
    const double q = num / a;
    const bool to_mn = pos_min ? pos : neg;
    const bool to_mx = pos_min ? neg : pos;
    mn = to_mn ? rng_take_min(mn, q) : mn;
    mx = to_mx ? rng_take_max(mx, q) : mx;
}

// ---------------------------------------------------------------------------------------------
// k_batch_ranging: one 256-thread workgroup per LP (grid = B), after k_batch_solution, whose
// basis [B][Rmax] and nonbasis [B][ldb] it reads beside final and dims.  Outputs rhs_lo / rhs_hi
// [B][Rmax] and cost_lo / cost_hi [B][ldb]; padding past n / m is +0.0 and an LP whose dims lie
// outside the block gets padding only.
//
// Position space: every row and column forms the bound of the label over it and scatters it to the
// slot that label names (code - m in rhs_*, code in cost_*), range-checked, so no inverse map is
// built.  The labels are a permutation, so every slot has one writer; the prefill with +0.0 is
// separated from the scatter by a workgroup barrier.
//   column pass  tiles of 64 columns, lane = column (a wave reads 64 consecutive doubles of a
//                row), wave w walks rows w, w + 4, ...; the running (lo, hi) stay in registers and
//                the four waves' partials meet in static LDS (two buffers by tile parity, so one
//                barrier per tile), combined and scattered by wave 0.  A tile without a slack label
//                does no division.
//   row pass     wave w takes rows w, w + 4, ...; a row labelled with a variable is walked by the
//                wave's lanes over the columns and reduced by shuffles; no LDS, no barrier.
// Every table element takes part in at most two divisions.  LDS is 8 KiB at any width.
__global__ __launch_bounds__(kRngBlock) void k_batch_ranging(
    const double* __restrict__ final, const int32_t* __restrict__ dims, int B, int Rmax, int ldb,
    const int32_t* __restrict__ basis, const int32_t* __restrict__ nonbasis,
    double* __restrict__ rhs_lo, double* __restrict__ rhs_hi, double* __restrict__ cost_lo,
    double* __restrict__ cost_hi) {
    __shared__ double s_lo[2][kRngWaves][kWave];
    __shared__ double s_hi[2][kRngWaves][kWave];
    const int b = blockIdx.x;
    if (b >= B) return;
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = dims[3 * b], m = dims[3 * b + 1];
    double* rl = rhs_lo + (size_t)b * Rmax;
    double* rh = rhs_hi + (size_t)b * Rmax;
    double* cl = cost_lo + (size_t)b * ldb;
    double* ch = cost_hi + (size_t)b * ldb;
    for (int i = tid; i < Rmax; i += kRngBlock) {
        rl[i] = 0.0;
        rh[i] = 0.0;
    }
    for (int j = tid; j < ldb; j += kRngBlock) {
        cl[j] = 0.0;
        ch[j] = 0.0;
    }
    if (n < 1 || m < 1 || n >= Rmax || m >= ldb) return;    // the whole workgroup alike
    __syncthreads();                                         // prefill before scatter
    const double pinf = rng_from_bits(kRngInf), ninf = rng_from_bits(kRngInf | kRngSign);
    const double* T = final + (size_t)b * Rmax * ldb;
    const double* Tf = T + (size_t)n * ldb;                  // the f-row
    const int32_t* bb = basis + (size_t)b * Rmax;
    const int32_t* nb = nonbasis + (size_t)b * ldb;

    // ---- column pass
    int buf = 0;
    for (int j0 = 0; j0 < m; j0 += kWave, buf ^= 1) {
        const int j = j0 + lane;
        const int code = j < m ? nb[j] : -1;
        const bool slack = code >= m && code < m + n;        // only where j < m
        double lo = ninf, hi = pinf;
        if (__ballot(slack) != 0ull) {                       // every wave sees the same labels
            for (int p = wid; p < n; p += kRngWaves) {
                const double* row = T + (size_t)p * ldb;
                const double a = slack ? row[j] : 0.0;       // a zero a: skipped
                rng_candidate(row[m], a, true, lo, hi);
            }
        }
        s_lo[buf][wid][lane] = lo;
        s_hi[buf][wid][lane] = hi;
        __syncthreads();
        if (wid == 0) {
            if (slack) {
#pragma unroll
                for (int w = 1; w < kRngWaves; ++w) {
                    lo = rng_take_max(lo, s_lo[buf][w][lane]);
                    hi = rng_take_min(hi, s_hi[buf][w][lane]);
                }
                rl[code - m] = lo;
                rh[code - m] = hi;
            } else if (code >= 0 && code < m) {
                cl[code] = rng_flip(Tf[j]);
                ch[code] = pinf;
            }
        }
    }

    // ---- row pass
    for (int p = wid; p < n; p += kRngWaves) {
        const int code = __builtin_amdgcn_readfirstlane(bb[p]);
        const double* row = T + (size_t)p * ldb;
        if (code >= m && code < m + n) {
            if (lane == 0) {
                rl[code - m] = rng_flip(row[m]);
                rh[code - m] = pinf;
            }
        } else if (code >= 0 && code < m) {
            double lo = ninf, hi = pinf;
            for (int j = lane; j < m; j += kWave)
                rng_candidate(rng_flip(Tf[j]), row[j], false, lo, hi);
#pragma unroll
            for (int mask = 32; mask >= 1; mask >>= 1) {
                lo = rng_take_max(lo, __shfl_xor(lo, mask, kWave));
                hi = rng_take_min(hi, __shfl_xor(hi, mask, kWave));
            }
            if (lane == 0) {
                cl[code] = lo;
                ch[code] = hi;
            }
        }
    }
}

// The same rules as a plain loop over one host table with leading dimension ld; outputs
// rhs_lo / rhs_hi [n], cost_lo / cost_hi [m].
void host_ranging(const double* T, int64_t ld, int n, int m, const int32_t* basis,
                  const int32_t* nonbasis, double* rhs_lo, double* rhs_hi, double* cost_lo,
                  double* cost_hi) {
    const double pinf = rng_from_bits(kRngInf), ninf = rng_from_bits(kRngInf | kRngSign);
    const double* Tf = T + (int64_t)n * ld;
    for (int i = 0; i < n; ++i) rhs_lo[i] = rhs_hi[i] = 0.0;
    for (int k = 0; k < m; ++k) cost_lo[k] = cost_hi[k] = 0.0;
    for (int j = 0; j < m; ++j) {
        const int code = nonbasis[j];
        if (code >= m && code < m + n) {
            double lo = ninf, hi = pinf;
            for (int p = 0; p < n; ++p)
                rng_candidate(T[(int64_t)p * ld + m], T[(int64_t)p * ld + j], true, lo, hi);
            rhs_lo[code - m] = lo;
            rhs_hi[code - m] = hi;
        } else if (code >= 0 && code < m) {
            cost_lo[code] = rng_flip(Tf[j]);
            cost_hi[code] = pinf;
        }
    }
    for (int p = 0; p < n; ++p) {
        const int code = basis[p];
        const double* row = T + (int64_t)p * ld;
        if (code >= m && code < m + n) {
            rhs_lo[code - m] = rng_flip(row[m]);
            rhs_hi[code - m] = pinf;
        } else if (code >= 0 && code < m) {
            double lo = ninf, hi = pinf;
            for (int j = 0; j < m; ++j) rng_candidate(rng_flip(Tf[j]), row[j], false, lo, hi);
            cost_lo[code] = lo;
            cost_hi[code] = hi;
        }
    }
}

}  // namespace
