// smx_branch.hpp -- branch and bound on solved LPs: which variable of a solved node to branch on
// (k_batch_branch_pick, host_branch_pick) and the two children's tables and labels
// (k_batch_branch, host_branch).  The pick is stated once in brn_frac / brn_better, which kernel
// and host twin share; a child is the extended table of smx_cuts.hpp for one single-variable cut,
// formed with the same scn_delta / scn_cost_term, so the arithmetic of a new row is stated there.
// Part of libsmx (compiled as one translation unit by smx_kernels.hip; not a standalone header).
//
// The contract (include/smx.h).  A node is a table T ([n+1][m+1], f-row = row n,
// "-b" = column m) under the labels basis[p] / nonbasis[j], with an integrality mask ints[k].
//   pick    every row p < n with basis[p] = k, 0 <= k < m, ints[k] != 0:  v = T[p][m],
//           lo = floor(v), a = v - lo, b = (lo + 1.0) - v, d = b < a ? b : a; a candidate iff
//           d > tol; the pick is the candidate first in the total order (larger d, then lower k,
//           then lower p).  Beside it, of ALL rows p < n: bneg = T[nb][m] at the smallest nb with
//           T[nb][m] < 0 (the row both selection rules look at first, so the row behind an
//           SMX_INCORRECT) and bmin = the smallest negative T[p][m]; +0.0 where none is negative.
//   branch  on row p, basis[p] = k < m, v = T[p][m]: the down child is the extended table of the
//           cut g[k] = -1.0, g[m] = floor(v), the up child that of g[k] = +1.0, g[m] = -ceil(v),
//           all other entries +0.0.  With one coefficient the cuts rule's walk over the rows
//           has one term: E[n][j] = s + c * T[p][j], s = c where nonbasis[j] = k (labels are
//           distinct, so nowhere after a pivot put k on a row), g[m] at j = m, else +0.0.
//   snap    a "-b" entry v of rows 0..n-1 with -snap <= v < 0 is written to both children as
//           +0.0 (brn_snap); snap = 0 snaps nothing and the children are the cuts rule's bits.
#pragma once
#pragma clang fp contract(off)

namespace {

constexpr int kBrnBlock = 256;
constexpr int kBrnWaves = kBrnBlock / kWave;

// One row's candidate: its distance d from the nearest whole number, its variable and its row.
// d is NaN for a NaN or infinite v, which `d > tol` then never takes.
struct Brn {
    double d;
    int k, p;
};
__host__ __device__ __forceinline__ double brn_frac(double v) {
    const double lo = floor(v);
    const double a = v - lo;
    const double b = (lo + 1.0) - v;
    return b < a ? b : a;
}
// The total order of the pick (k = -1 is "no candidate", which loses to any candidate).
__host__ __device__ __forceinline__ bool brn_better(const Brn& a, const Brn& b) {
    if (b.k < 0) return a.k >= 0;
    if (a.k < 0) return false;
    if (a.d != b.d) return a.d > b.d;
    if (a.k != b.k) return a.k < b.k;
    return a.p < b.p;
}
__host__ __device__ __forceinline__ Brn brn_of_row(double v, int code, int m, const int32_t* ints,
                                                  double tol, int p) {
    if (code < 0 || code >= m || ints[code] == 0) return Brn{0.0, -1, -1};
    const double d = brn_frac(v);
    return d > tol ? Brn{d, code, p} : Brn{0.0, -1, -1};
}
// A constant that misses zero from below by at most `snap` is read as zero.
__host__ __device__ __forceinline__ double brn_snap(double v, double snap) {
    return (v < 0.0 && v >= -snap) ? 0.0 : v;
}
// The two cuts' coefficient and constant: child 0 is down, child 1 is up.
__host__ __device__ __forceinline__ double brn_coef(int child) { return child ? 1.0 : -1.0; }
__host__ __device__ __forceinline__ double brn_const(int child, double v) {
    return child ? -ceil(v) : floor(v);
}

// ---------------------------------------------------------------------------------------------
// k_batch_branch_pick: one WAVEFRONT per node, kBrnWaves nodes per workgroup.  A node's input is
// its label array and its strided "-b" column: n values, 3 to 63 for the UI-sized LPs the batch
// calls mostly hold, at most 8189.  A wave takes them in ceil(n / 64) steps with one candidate in
// registers per lane and folds the 64 candidates with six shuffles; a workgroup per node would
// leave three of four waves idle on the common sizes and need LDS and a barrier for a fold that
// touches one value per row.  brn_better is a total order, so the fold's grouping cannot show.
// ints [B][ldb] is read at row lp[q]; a node whose lp is outside 0..B-1 or whose dims are outside
// the block has no candidate.
__global__ __launch_bounds__(kBrnBlock) void k_batch_branch_pick(
    const double* __restrict__ final, const int32_t* __restrict__ dims, int Q, int Rmax, int ldb,
    const int32_t* __restrict__ basis, const int32_t* __restrict__ ints, int B,
    const int32_t* __restrict__ lp, double tol, int32_t* __restrict__ bvar,
    int32_t* __restrict__ brow, double* __restrict__ bval, double* __restrict__ bneg,
    double* __restrict__ bmin) {
    const int lane = threadIdx.x & (kWave - 1);
    const int q = blockIdx.x * kBrnWaves + (threadIdx.x >> 6);
    if (q >= Q) return;                                      // the whole wave alike
    const int n = dims[3 * (size_t)q], m = dims[3 * (size_t)q + 1];
    const int b = lp[q];
    const bool inside = n >= 1 && m >= 1 && n < Rmax && m < ldb && b >= 0 && b < B;
    Brn best{0.0, -1, -1};
    double bestv = 0.0, negv = 0.0, minv = 0.0;
    int negp = INT32_MAX;                                    // the first row with a negative "-b"
    if (inside) {
        const double* T = final + (size_t)q * Rmax * ldb;
        const int32_t* bb = basis + (size_t)q * Rmax;
        const int32_t* in = ints + (size_t)b * ldb;
        for (int p = lane; p < n; p += kWave) {
            const double v = T[(size_t)p * ldb + m];
            const Brn c = brn_of_row(v, bb[p], m, in, tol, p);
            if (brn_better(c, best)) {
                best = c;
                bestv = v;
            }
            if (v < 0.0 && negp == INT32_MAX) {              // p ascends within a lane
                negp = p;
                negv = v;
            }
            if (v < minv) minv = v;
        }
    }
#pragma unroll
    for (int s = 1; s < kWave; s <<= 1) {
        const Brn o{__shfl_xor(best.d, s), __shfl_xor(best.k, s), __shfl_xor(best.p, s)};
        const double ov = __shfl_xor(bestv, s);
        if (brn_better(o, best)) {
            best = o;
            bestv = ov;
        }
        const int op = __shfl_xor(negp, s);
        const double onv = __shfl_xor(negv, s);
        if (op < negp) {
            negp = op;
            negv = onv;
        }
        const double om = __shfl_xor(minv, s);
        if (om < minv) minv = om;
    }
    if (lane == 0) {
        bvar[q] = best.k;
        brow[q] = best.p;
        bval[q] = best.k >= 0 ? bestv : 0.0;
        bneg[q] = negv;
        bmin[q] = minv;
    }
}

// The same rule on one host table with leading dimension ld.
void host_branch_pick(const double* T, int64_t ld, int n, int m, const int32_t* basis,
                      const int32_t* ints, double tol, int32_t* bvar, int32_t* brow,
                      double* bval, double* bneg, double* bmin) {
    Brn best{0.0, -1, -1};
    double bestv = 0.0, negv = 0.0, minv = 0.0;
    bool neg = false;
    for (int p = 0; p < n; ++p) {
        const double v = T[(int64_t)p * ld + m];
        const Brn c = brn_of_row(v, basis[p], m, ints, tol, p);
        if (brn_better(c, best)) {
            best = c;
            bestv = v;
        }
        if (v < 0.0 && !neg) {
            neg = true;
            negv = v;
        }
        if (v < minv) minv = v;
    }
    *bvar = best.k;
    *brow = best.p;
    *bval = best.k >= 0 ? bestv : 0.0;
    *bneg = negv;
    *bmin = minv;
}

// ---------------------------------------------------------------------------------------------
// k_batch_branch: one 256-thread workgroup per PARENT i (grid = Qc); the parent is node src[i] of
// final [Q][Rmax][ldb] / dims [Q][3] / basis [Q][Rmax] / nonbasis [Q][ldb] / func [Q][ldb], the
// row to branch on is brow[src[i]].  Outputs: children 2i (down) and 2i + 1 (up) of tabs_c
// [2Qc][Rmax_out][ldb], dims_c [2Qc][3], basis_c [2Qc][Rmax_out], nonbasis_c [2Qc][ldb], func_c
// [2Qc][ldb]; Rmax_out >= Rmax (the host checks it).  The parent's block is read once and every
// element read is stored twice.  A parent that is not branched (brow outside 0..n-1, a label
// there that is no variable, n + 1 >= Rmax_out, dims outside the block: then n = Rmax - 1) gives
// two relayouts with its dims kept; a src outside 0..Q-1 names no parent and gives two blocks of
// +0.0 with dims (0, 0, 0), labels -1 and func +0.0.
//
// Every element of the outputs is written exactly once and nothing is read back, so there is no
// barrier:
//   copy     rows 0..n-1 by a flat coalesced walk (padding columns included; the "-b" entries
//            through brn_snap), the f-row to row n + 1 (n when not branched), +0.0 into the rows
//            past it
//   new row  lane = column: one read of T[p][j] feeds both children
// No LDS, no scratch.
__global__ __launch_bounds__(kBrnBlock) void k_batch_branch(
    const double* __restrict__ final, const int32_t* __restrict__ dims, int Q, int Rmax, int ldb,
    const int32_t* __restrict__ basis, const int32_t* __restrict__ nonbasis,
    const double* __restrict__ func, const int32_t* __restrict__ src,
    const int32_t* __restrict__ brow, int Qc, int Rmax_out, double snap,
    double* __restrict__ tabs_c,
    int32_t* __restrict__ dims_c, int32_t* __restrict__ basis_c, int32_t* __restrict__ nonbasis_c,
    double* __restrict__ func_c) {
    const int i = blockIdx.x;
    if (i >= Qc) return;
    const int tid = threadIdx.x;
    const int q = src[i];
    const size_t blk = (size_t)Rmax_out * ldb;
    double* E0 = tabs_c + (size_t)(2 * i) * blk;
    double* E1 = E0 + blk;
    int32_t* bc0 = basis_c + (size_t)(2 * i) * Rmax_out;
    int32_t* bc1 = bc0 + Rmax_out;
    int32_t* nc0 = nonbasis_c + (size_t)(2 * i) * ldb;
    int32_t* nc1 = nc0 + ldb;
    double* fc0 = func_c + (size_t)(2 * i) * ldb;
    double* fc1 = fc0 + ldb;
    const int end = Rmax_out * ldb;                          // Rmax_out + ldb <= 8192: under 2^25
    if (q < 0 || q >= Q) {                                   // the whole workgroup alike
        if (tid < 6) dims_c[6 * (size_t)i + tid] = 0;
        for (int e = tid; e < end; e += kBrnBlock) E0[e] = E1[e] = 0.0;
        for (int r = tid; r < Rmax_out; r += kBrnBlock) bc0[r] = bc1[r] = -1;
        for (int j = tid; j < ldb; j += kBrnBlock) {
            nc0[j] = nc1[j] = -1;
            fc0[j] = fc1[j] = 0.0;
        }
        return;
    }
    const int n0 = dims[3 * (size_t)q], m = dims[3 * (size_t)q + 1];
    const bool inside = n0 >= 1 && m >= 1 && n0 < Rmax && m < ldb;
    const int n = inside ? n0 : Rmax - 1;                    // rows above the f-row
    const double* T = final + (size_t)q * Rmax * ldb;
    const int32_t* bb = basis + (size_t)q * Rmax;
    const int32_t* nb = nonbasis + (size_t)q * ldb;
    const double* fn = func + (size_t)q * ldb;
    const int p = brow[q];
    int k = -1;
    if (inside && p >= 0 && p < n && n + 1 < Rmax_out) k = bb[p];
    const int kc = (k >= 0 && k < m) ? 1 : 0;                // 1: branched, 0: a relayout

    if (tid < 6)                                             // children 2i and 2i + 1
        dims_c[6 * (size_t)i + tid] = dims[3 * (size_t)q + tid % 3] + (tid % 3 == 0 ? kc : 0);
    for (int r = tid; r < Rmax_out; r += kBrnBlock)
        bc0[r] = bc1[r] = r < n ? bb[r] : (r < n + kc ? m + r : -1);
    for (int j = tid; j < ldb; j += kBrnBlock) {
        nc0[j] = nc1[j] = (!inside || j < m) ? nb[j] : -1;
        fc0[j] = fc1[j] = fn[j];
    }

    // ---- copy
    const int head = n * ldb;
#pragma unroll 4
    for (int e = tid; e < head; e += kBrnBlock) {
        double t = T[e];
        if (t < 0.0 && t >= -snap && e % ldb == m) t = 0.0;  // brn_snap on column m alone; the
        E0[e] = t;                                           // modulo runs for such values only
        E1[e] = t;
    }
    const int frow = (n + kc) * ldb;
    for (int j = tid; j < ldb; j += kBrnBlock) {
        const double t = T[head + j];
        E0[frow + j] = t;
        E1[frow + j] = t;
    }
#pragma unroll 4
    for (int e = frow + ldb + tid; e < end; e += kBrnBlock) E0[e] = E1[e] = 0.0;
    if (kc == 0) return;                                     // the whole workgroup alike

    // ---- the new row n of both children
    const double* Tp = T + (size_t)p * ldb;
    const double v = Tp[m];
    for (int j = tid; j < ldb; j += kBrnBlock) {
        double e0 = 0.0, e1 = 0.0;
        if (j <= m) {
            const double t = Tp[j];
            const bool own = j < m && nb[j] == k;
            e0 = scn_cost_term(j == m ? brn_const(0, v) : (own ? brn_coef(0) : 0.0), brn_coef(0), t);
            e1 = scn_cost_term(j == m ? brn_const(1, v) : (own ? brn_coef(1) : 0.0), brn_coef(1), t);
        }
        E0[head + j] = e0;
        E1[head + j] = e1;
    }
}

// The same on one host table with leading dimension ld, through host_cuts: E_down and E_up
// [n+2][ld_out] receive columns 0..m of every row, basis_out [n+1] the row labels of both.
void host_branch(const double* T, int64_t ld, int n, int m, const int32_t* basis,
                 const int32_t* nonbasis, int p, double snap, double* E_down, double* E_up,
                 int64_t ld_out, int32_t* basis_out) {
    const int k = basis[p];
    const double v = T[(int64_t)p * ld + m];
    std::vector<double> g((size_t)m + 1);
    for (int child = 0; child < 2; ++child) {
        for (int j = 0; j < m; ++j) g[j] = 0.0;
        g[k] = brn_coef(child);
        g[m] = brn_const(child, v);
        double* E = child ? E_up : E_down;
        host_cuts(T, ld, n, m, basis, nonbasis, g.data(), 1, E, ld_out, basis_out);
        for (int r = 0; r < n; ++r) E[(int64_t)r * ld_out + m] = brn_snap(E[(int64_t)r * ld_out + m], snap);
    }
}

}  // namespace
