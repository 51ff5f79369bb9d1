// smx_sweep.hpp -- the block sweep: T_k -> T_{k+P} for every element (P = peff pivots of the block
// that smx_block.hpp's planner decided), in one pass over the table.
// Part of libsmx (compiled as one translation unit by smx_kernels.hip; not a standalone header).
//
// Every element runs the P steps of chain() (smx_block.hpp); the division takes the hoisted-
// reciprocal form where the operands allow it (the domains at kBndSpan there) and the IEEE
// division otherwise.  In reading order:
//   the per-pivot steps      fast and zero-safe, each stated once on a lane's two columns (dbl2)
//   blk_exact_h              the exact path of one unit
//   the path counters        diagnostic build only
//   BlkChunk                 the chunk a wave is sweeping and which paths it allows
//   BlkRegOps / BlkLdsOps    where a pivot's row slice and (e, y) come from: registers (FORM 4)
//                            or LDS (FORM 5 / 6 / 7 / 8), with the fast and zero-safe row paths
//   blk_row_pairs / _quads   FORM 7's and 8's prefetch loops over row pairs and row quads
//   blk_geom_wave / _wg      a wave's chunk, first row and row stride, per layout
//   blk_sweep_body_flag      the sweep of one block: staging, chunk flags, a row (rowf), a row
//                            pair (pairf), a row quad (quadf), the row loops
//   blk_fixcols, blk_out, k_blk_sweep, k_blk_sweep_rest
// What is written in place where it is used, and not as a function of its own, is so because the
// function form changed the kernels' instructions.
#pragma once
#pragma clang fp contract(off)

namespace {

// ---- the per-pivot steps --------------------------------------------------------------------

// The hoisted-reciprocal quotient n / e (y: fd_prep's refined reciprocal of e): bit-identical to
// the division on the bounded domain (smx_block.hpp, kBndSpan)
__device__ __forceinline__ double fd_fast(double n, double e, double y) {
    const double t = n * y;
    const double r = fma(-e, t, n);
    return fma(r, y, t);
}

// A step's numerators x e - p m (p: the pivot row's values at the lane's columns, m: the row's
// multiplier), every product rounded on its own and formed inside the subtraction: handing the
// products in pre-formed moves them ahead of x e and the compiler schedules the chains differently
__device__ __forceinline__ dbl2 blk_num(dbl2 v, double e, dbl2 p, double m) {
    return dbl2{v[0] * e - p[0] * m, v[1] * e - p[1] * m};
}
// the same with the products b = p m formed ahead on purpose (BlkRegOps)
__device__ __forceinline__ dbl2 blk_num_b(dbl2 v, double e, dbl2 b) {
    return dbl2{v[0] * e - b[0], v[1] * e - b[1]};
}

// The fast step: six instructions per element, no check (bounded operands)
__device__ __forceinline__ dbl2 blk_quot_fast(dbl2 n, double e, double y) {
    return dbl2{fd_fast(n[0], e, y), fd_fast(n[1], e, y)};
}
__device__ __forceinline__ dbl2 blk_step_fast(dbl2 v, dbl2 p, double m, double e, double y) {
    return blk_quot_fast(blk_num(v, e, p, m), e, y);
}

// The zero-safe steps (operands bounded or exact zeros): fd_zero's v_div_fixup, one more
// instruction per element-pivot ...
__device__ __forceinline__ dbl2 blk_quot_zero(dbl2 n, double e, double y) {
    return dbl2{fd_zero(n[0], e, y), fd_zero(n[1], e, y)};
}
// ... or the sign-folded negated division (fd_zneg): the chain carries g_q = -sgn(e_q) x_{q+1},
// so step q's product x_q e_q is g_{q-1} M_q with M_q = -sgn(e_{q-1}) e_q (M_0 = e_0, exact sign
// flips), the divisor |M_q| = |e_q| (a source modifier), the reciprocal ya = |y_q|; the element
// after the block is zf g_{P-1}, zf = -sgn(e_{P-1}).  The fast step's instruction count.
__device__ __forceinline__ dbl2 blk_step_zneg(dbl2 v, dbl2 p, double m, double M, double ya) {
    const dbl2 n = blk_num(v, M, p, m);
    return dbl2{fd_zneg(n[0], fabs(M), ya), fd_zneg(n[1], fabs(M), ya)};
}

// The exact path of one unit (two adjacent columns of one row): every rule of simplex.py:155-175
// with the hardware division, the pivots' rows and columns read from the header as it goes (the
// rare path: no registers held for them across the sweep).  ops.pr(q) returns the chunk's
// pivot-row values of pivot q at this lane's two columns.
template <int P, class OPS>
__device__ __forceinline__ dbl2 blk_exact_h(dbl2 v, int row, int j, const BlkHdr* __restrict__ h,
                                            const double* eq, const OPS& ops, const double* pc) {
#pragma unroll
    for (int q = 0; q < P; ++q) {
        const int rq = h->r[q], cq = h->c[q];
        const dbl2 p = ops.pr(q);
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            const int jj = j + hh;
            double num;
            if (row == rq) {
                num = (jj == cq) ? 1.0 : -v[hh];
            } else {
                const double a = v[hh] * eq[q];
                const double b = p[hh] * pc[q];
                num = (jj == cq) ? v[hh] : (a - b);
            }
            v[hh] = num / eq[q];
        }
    }
    return v;
}

// The flag-form sweep: one row per step of a wave, the planner's per-row flags (blk_rflags) instead
// of per-row checks.  The unchecked fast path needs a bounded chunk (e and the chunk's pivot-row
// values in [2^-100, 2^101), checked once per sweep), a flagged row (no pivot row, every
// multiplier bounded: the planner checked them when it computed them) and bounded inputs (one vote
// per row).  Re-checking the row's P multipliers in the sweep cost ~30 scalar and ~12 vector
// instructions per row beside the 120 fp64 ones, and the row's branch waited on them:
// tools/sweep_lab.hip, 16384^2, P = 10: 894 -> 753 us per sweep (profiles/r03/sweep_lab.jsonl).
// The fast path is straight-line: a per-pivot (uniform, never taken) branch to select a pivot
// column's numerator cost another ~20 % (lab V7 vs V6), so pivot columns are NOT special here.  On
// a flagged row the pivot column's lane computes RN(x e) - RN(e x) = +0 at its step (its element
// IS mul[i][q] there) and carries harmless finite values after it; blk_fixcols (k_blk_sweep_rest)
// then rewrites every pivot column from the planner's multipliers.  Rows or chunks outside the fast
// domain take the zero-safe path, then the window-tracked path (a pivot column's zero numerator
// fails its vote), then the exact path, which applies every rule itself.
//
// The layouts (FORM; 6, 7 and 8 are described at g_sweep_items, kPairPhase and kQuadPhase):
//  4  wave-chunk: every wave keeps one 128-column chunk (w % nchunks) for the whole pass, its
//     pivot-row slices in registers (2P doubles per lane) and e / y in scalar registers -- the
//     fastest up to ~12 pivots (profiles/r03/, tools/sweep_lab2.hip V1);
//  5  workgroup-chunk: the four waves of a workgroup share one chunk (blockIdx % nchunks) and its
//     pivot-row slices live in LDS (P KiB per workgroup), (e, y) pairs in LDS as well: ~60-70
//     VGPRs at any P, so 16-24 pivots per sweep keep 7-8 waves per SIMD instead of spilling
//     scalars (tools/sweep_lab2.hip V3 / V6, profiles/r04b/lab2.jsonl: P = 20 1.33 ms vs 1.43 ms
//     for the register layout at 16384^2).
// Diagnostic build only (-DSMX_PATH_COUNT, Makefile target `diag` -> libsmx_diag.so): how many
// (row, 128-column chunk) units of the flag-form sweep take each path, summed over every launch
// until smx_diag_path_counts reads (and optionally clears) them.  Per wave in registers, one add
// per counter and wave at the end (lane k adds counter k).  The product build has none of it.
// The chunk's part of what they count is read from BlkChunk.
enum : int {
    kPcFast = 0,        // chunk free, row flag 1, bounded inputs: the unchecked fast path
    kPcZero,            // the zero-extended domain (fd_zero / fd_zneg)
    kPcWindow,          // the window-tracked path, vote passed
    kPcWindowFail,      // the window-tracked path, vote failed -> exact
    kPcExact,           // straight to the exact path (a pivot row, or a pivot not ok)
    kPcChunkNotFree,    // units in chunks that are not free (e / pivot-row values)
    kPcChunkNotZok,     // units in chunks that are not even zok
    kPcRowFlag0,        // units of rows with flag 0 (a multiplier unbounded, not zero)
    kPcRowFlag3,        // units of rows with flag 3 (bounded or zero, at least one zero)
    kPcXFail,           // chunk free and flag 1, but an input element out of bounds
    kPcChunkE,          // units in chunks whose pivots fail (e outside the window / bounds)
    kPcChunkP,          // units in chunks with a pivot-row value neither bounded nor zero
    kPcClkCycles,       // per wave: s_memtime ticks (shader clock) over the wave's sweep body
    kPcClkTicks,        // per wave: s_memrealtime ticks (100 MHz) over the same span
    kPcCount
};
#ifdef SMX_PATH_COUNT
__device__ unsigned long long g_path_cnt[kPcCount];
#define SMX_PC_DECL                                                                             \
    uint64_t pc_cnt[kPcCount] = {};                                                             \
    const uint64_t pc_t0 = __builtin_amdgcn_s_memtime();                                        \
    const uint64_t pc_r0 = __builtin_amdgcn_s_memrealtime();
#define SMX_PC(k) (++pc_cnt[(k)])
#define SMX_PC_FLUSH                                                                            \
    do {                                                                                        \
        pc_cnt[kPcClkCycles] = __builtin_amdgcn_s_memtime() - pc_t0;                            \
        pc_cnt[kPcClkTicks] = __builtin_amdgcn_s_memrealtime() - pc_r0;                         \
        const int l_ = threadIdx.x & (kWave - 1);                                               \
        uint64_t v_ = 0;                                                                        \
        _Pragma("unroll") for (int k_ = 0; k_ < kPcCount; ++k_) if (l_ == k_) v_ = pc_cnt[k_];  \
        if (l_ < kPcCount && v_) atomicAdd(&g_path_cnt[l_], (unsigned long long)v_);            \
    } while (0)
#else
#define SMX_PC_DECL
#define SMX_PC(k) ((void)0)
#define SMX_PC_FLUSH ((void)0)
#endif

// FORM 6 (round 6): the LDS layout in work items.  A workgroup of FORM 5 keeps one chunk for all
// its rows, so where a few chunks run a slower path (config 5's block 0: 5 of 257 chunks on the
// window-tracked path) their workgroups finish last and the sweep waits for them (1.33x block 2's
// cycles at 1.05x its instructions).  FORM 6 cuts every workgroup's rows into K
// contiguous segments (K = g_sweep_items) and takes segment k at chunk (c0 + k * stride) mod
// nchunks, stride ~ nchunks / K: for every k the map c0 -> chunk is a shift, so each (chunk,
// segment) is still swept by exactly the workgroups that would have swept it, and a slow chunk's
// rows spread over ~K times as many workgroups.  The pivot-row slices are restaged per item.
__device__ int g_sweep_items = 16;

// FORM 7: the LDS layout in row pairs.  FORM 5's grid, chunk ownership, staging and chunk flags; a
// lane keeps TWO rows of its two columns (rows i0 and i0 + qs of its wave), so each ds_read_b128
// of a pivot's row slice and of its (e, y) feeds four independent chains instead of two: half the
// LDS instructions and returned bytes per element-pivot, and the per-row costs (the scalar round
// trip for flags and multipliers, the input vote, the address arithmetic, the vmcnt hand-over)
// once per two rows.  Two rows' multipliers of all 24 pivots would be 96 scalar registers (round 2
// dropped two-row batches for that: the scalars spilled into vector lanes), so the
// pivots are taken in phases of kPairPhase: 2 rows x 12 multipliers are the 48 scalar registers
// one row x 24 takes in FORM 5, and each phase's multipliers are loaded where the phase begins.
// A pair is fast only when both rows are (flags 1, one vote over both rows' inputs); any other
// pair, and an odd row left at the end, goes row by row through FORM 5's single-row code,
// unchanged.
constexpr int kPairPhase = 12;

// One pivot of a row pair's fast path: four chains, each the one-row fast path's six
// instructions in its order (two products, their difference, t = n y, r = fma(-e, t, n),
// fma(r, y, t)).
__device__ __forceinline__ void blk_pair_step(dbl2& va, dbl2& vb, dbl2 p, dbl2 ey, double ma,
                                              double mb) {
    const double e = ey[0], y = ey[1];
    const dbl2 na = blk_num(va, e, p, ma);
    const dbl2 nb = blk_num(vb, e, p, mb);
    va = blk_quot_fast(na, e, y);
    vb = blk_quot_fast(nb, e, y);
}

// FORM 8: the LDS layout in row quads.  FORM 7's grid, chunk ownership, staging and chunk flags; a
// lane keeps FOUR rows of its two columns (rows i0, i0 + qs, i0 + 2 qs, i0 + 3 qs of its wave), so
// each ds_read_b128 of a pivot's row slice feeds eight chains, and (e, y) are not read from LDS at
// all: a wave-uniform pair returned into 4 VGPRs x 64 lanes was half of FORM 7's LDS reads.  The
// pivots are taken in phases of kQuadPhase; where a phase begins, one scalar round trip loads the
// four rows' multipliers of the phase (4 x 6 doubles, the 48 scalar registers of FORM 7's phase)
// and the phase's e and y (24 more).  A quad is fast only when all four rows exist and are flagged
// 1, the chunk is free and one vote over the eight inputs passes; any other quad, and a tail of
// 1-3 rows, goes row by row through FORM 5's single-row code, unchanged.  Instantiated from
// kQuadMinP pivots on (blk_sweep_fn).
constexpr int kQuadPhase = 6;
constexpr int kQuadMinP = 13;

// One pivot of a row quad's fast path: eight chains, each the one-row fast path's six
// instructions in its order, with e, y and the multipliers as scalar operands.
__device__ __forceinline__ void blk_quad_step(dbl2& v0, dbl2& v1, dbl2& v2, dbl2& v3, dbl2 p,
                                              double e, double y, double m0, double m1, double m2,
                                              double m3) {
    const dbl2 n0 = blk_num(v0, e, p, m0);
    const dbl2 n1 = blk_num(v1, e, p, m1);
    const dbl2 n2 = blk_num(v2, e, p, m2);
    const dbl2 n3 = blk_num(v3, e, p, m3);
    v0 = blk_quot_fast(n0, e, y);
    v1 = blk_quot_fast(n1, e, y);
    v2 = blk_quot_fast(n2, e, y);
    v3 = blk_quot_fast(n3, e, y);
}

// The chunk a wave is sweeping: its place, and which paths its pivots and pivot-row values allow.
// Filled where the sweep stages a chunk (stage, chunk_flags); FORM 6 fills it again for every
// work item.  The diagnostic counters read it too.
struct BlkChunk {
    int ch;        // the chunk: columns [ch * 128, (ch + 1) * 128)
    int j;         // the lane's first column (possibly past C in the last chunk)
    int jc;        // j, kept inside the table for loads
    uint32_t et;   // the largest bnd_term of the pivot elements
    bool pz;       // this lane's pivot-row values are all bounded or an exact +-0
    bool zok;      // bounded or zero throughout (zero-safe path)
    bool free;     // bounded, no zeros (fast path)
};

constexpr int kBlkChunk = 2 * kWave;   // columns of a chunk: two per lane

// ---- the operand sources --------------------------------------------------------------------

// FORM 4: the chunk's pivot-row slices in registers (2P doubles per lane), e / y in scalar
// registers (filled by blk_sweep_body_flag).
template <int P>
struct BlkRegOps {
    dbl2 prs[P];
    double eq[P], yq[P];
    __device__ __forceinline__ dbl2 pr(int q) const { return prs[q]; }
    __device__ __forceinline__ dbl2 ey(int q) const { return dbl2{eq[q], yq[q]}; }
    // the 2P products p * mq first (they do not depend on the chain) and held there:
    // issued back to back, the chains after them run without waiting on any
    // (tools/sweep_lab.hip V1: this order, 750-770 us at P = 10, 16384^2; interleaved
    // with the chains as the compiler otherwise places them, ~850 us)
    __device__ __forceinline__ void products(const double* m, dbl2* bq) const {
#pragma unroll
        for (int q = 0; q < P; ++q) bq[q] = dbl2{prs[q][0] * m[q], prs[q][1] * m[q]};
#pragma unroll
        for (int q = 0; q < P; ++q) asm volatile("" : "+v"(bq[q]));
    }
    __device__ __forceinline__ dbl2 fast(dbl2 v, const double* m) const {
        dbl2 bq[P];
        products(m, bq);
#pragma unroll
        for (int q = 0; q < P; ++q) v = blk_quot_fast(blk_num_b(v, eq[q], bq[q]), eq[q], yq[q]);
        return v;
    }
    // zero-safe with fd_zero.  (Not fd_zneg: with e / y in scalar registers its per-pivot LDS
    // reads cost more than the fixup saved -- config 5 at 12 pivots per sweep, block 0 unchanged
    // and the fast-path blocks 13 % slower, profiles/r06aa/)
    __device__ __forceinline__ dbl2 zero(dbl2 v, const double* m) const {
        dbl2 bq[P];
        products(m, bq);
#pragma unroll
        for (int q = 0; q < P; ++q) v = blk_quot_zero(blk_num_b(v, eq[q], bq[q]), eq[q], yq[q]);
        return v;
    }
};

// FORM 5 / 6 / 7: the workgroup's chunk staged in LDS -- the pivot-row slices (P KiB), the (e, y)
// pairs and fd_zneg's scalars (M_q, |y_q|) and zf (blk_step_zneg) -- read per pivot, few registers
// (the arrays are blk_sweep_body_flag's; it writes the pivots' scalars)
template <int P>
struct BlkLdsOps {
    dbl2 (*s_pr)[kWave];
    dbl2* s_ey;
    dbl2* s_zm;
    double* s_zf;
    int lane;
    // the chunk's slices of the P pivot rows (every thread of the workgroup; a barrier follows)
    __device__ __forceinline__ void stage(const double* __restrict__ pr, int64_t ld, int ch,
                                          int C) const {
        for (int t = threadIdx.x; t < P * kWave; t += kUpdBlock) {
            const int q = t / kWave, jl = ch * kBlkChunk + 2 * (t % kWave);
            s_pr[q][t % kWave] = jl < C ? *reinterpret_cast<const dbl2*>(pr + (int64_t)q * ld + jl)
                                        : dbl2{0.0, 0.0};
        }
    }
    __device__ __forceinline__ dbl2 pr(int q) const { return s_pr[q][lane]; }
    __device__ __forceinline__ dbl2 ey(int q) const { return s_ey[q]; }
    // products inline: the slices and (e, y) come from LDS per pivot
    __device__ __forceinline__ dbl2 fast(dbl2 v, const double* m) const {
#pragma unroll
        for (int q = 0; q < P; ++q) {
            const dbl2 p = pr(q);
            const dbl2 e = ey(q);
            v = blk_step_fast(v, p, m[q], e[0], e[1]);
        }
        return v;
    }
    // zero-safe with the sign-folded negated division
    __device__ __forceinline__ dbl2 zero(dbl2 v, const double* m) const {
#pragma unroll
        for (int q = 0; q < P; ++q) {
            const dbl2 p = pr(q);
            const dbl2 my = s_zm[q];
            v = blk_step_zneg(v, p, m[q], my[0], my[1]);
        }
        return dbl2{v[0] * *s_zf, v[1] * *s_zf};
    }
};

// Rows r0, r0 + qs, ... below hi two at a time (FORM 7; ldc(row): a row's input, pairf(xa, xb,
// row, hi): the sweep of rows row and row + qs).  Prefetch depth 1 over pairs: before a pair's
// registers are used, the ops issued after its two loads are the previous pair's two stores (one
// only for an odd last row, and then no pair follows) and the other pair's two loads: vmcnt(4)
template <class LDC, class PAIRF>
__device__ __forceinline__ void blk_row_pairs(LDC ldc, PAIRF pairf, int r0, int qs, int hi) {
    int i0 = r0;
    dbl2 a0 = ldc(i0), a1 = ldc(i0 + qs);
    dbl2 b0 = ldc(i0 + 2 * qs), b1 = ldc(i0 + 3 * qs);
    asm volatile("s_waitcnt vmcnt(2)" : "+v"(a0), "+v"(a1) :: "memory");
    for (;;) {
        pairf(a0, a1, i0, hi);
        i0 += 2 * qs;
        if (i0 >= hi) break;
        a0 = ldc(i0 + 2 * qs);
        a1 = ldc(i0 + 3 * qs);
        asm volatile("s_waitcnt vmcnt(4)" : "+v"(b0), "+v"(b1) :: "memory");
        pairf(b0, b1, i0, hi);
        i0 += 2 * qs;
        if (i0 >= hi) break;
        b0 = ldc(i0 + 2 * qs);
        b1 = ldc(i0 + 3 * qs);
        asm volatile("s_waitcnt vmcnt(4)" : "+v"(a0), "+v"(a1) :: "memory");
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// Rows r0, r0 + qs, ... below hi four at a time (FORM 8; quadf(x0, x1, x2, x3, row, hi): the
// sweep of rows row .. row + 3 qs).  Prefetch depth 1 over quads: before a quad's registers are
// used, the ops issued after its four loads are the previous quad's four stores (fewer only for a
// tail, and then no quad follows) and the other quad's four loads: vmcnt(8); vmcnt(4) first
template <class LDC, class QUADF>
__device__ __forceinline__ void blk_row_quads(LDC ldc, QUADF quadf, int r0, int qs, int hi) {
    int i0 = r0;
    dbl2 a0 = ldc(i0), a1 = ldc(i0 + qs), a2 = ldc(i0 + 2 * qs), a3 = ldc(i0 + 3 * qs);
    dbl2 b0 = ldc(i0 + 4 * qs), b1 = ldc(i0 + 5 * qs), b2 = ldc(i0 + 6 * qs),
         b3 = ldc(i0 + 7 * qs);
    asm volatile("s_waitcnt vmcnt(4)" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) :: "memory");
    for (;;) {
        quadf(a0, a1, a2, a3, i0, hi);
        i0 += 4 * qs;
        if (i0 >= hi) break;
        a0 = ldc(i0 + 4 * qs);
        a1 = ldc(i0 + 5 * qs);
        a2 = ldc(i0 + 6 * qs);
        a3 = ldc(i0 + 7 * qs);
        asm volatile("s_waitcnt vmcnt(8)" : "+v"(b0), "+v"(b1), "+v"(b2), "+v"(b3) :: "memory");
        quadf(b0, b1, b2, b3, i0, hi);
        i0 += 4 * qs;
        if (i0 >= hi) break;
        b0 = ldc(i0 + 4 * qs);
        b1 = ldc(i0 + 5 * qs);
        b2 = ldc(i0 + 6 * qs);
        b3 = ldc(i0 + 7 * qs);
        asm volatile("s_waitcnt vmcnt(8)" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) :: "memory");
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// A wave's share of the table: its chunk, its first row and the stride to its next row.
struct BlkGeom {
    int ch, base, qs;
};
// wave-chunk (FORM 4): every wave keeps one chunk (w % nchunks) for the whole pass
__device__ __forceinline__ BlkGeom blk_geom_wave(int nchunks, int wib) {
    const int NW = (int)gridDim.x * kUpdWaves;
    const int w = (int)blockIdx.x * kUpdWaves + wib;
    return BlkGeom{w % nchunks, w / nchunks, NW / nchunks};
}
// workgroup-chunk (FORM 5 / 7, FORM 6's first item): the four waves of a workgroup share one
// chunk (blockIdx % nchunks)
__device__ __forceinline__ BlkGeom blk_geom_wg(int nchunks, int wib) {
    return BlkGeom{(int)blockIdx.x % nchunks, ((int)blockIdx.x / nchunks) * kUpdWaves + wib,
                   ((int)gridDim.x / nchunks) * kUpdWaves};
}

// The sweep of one block, every layout.  The operands are loaded or staged here in place (as
// functions taking h and pr they changed FORM 4's and the LDS forms' instructions).
template <int P, int FORM>
__device__ __forceinline__ void blk_sweep_body_flag(const double* Tin, double* Tout, int64_t ld,
                                                    int R, int C, const BlkHdr* __restrict__ h,
                                                    const double* __restrict__ pr,
                                                    const double* __restrict__ mul) {
    constexpr bool LDS = FORM >= 5;
    constexpr bool ITEMS = FORM == 6;
    constexpr bool PAIRS = FORM == 7;
    constexpr bool QUADS = FORM == 8;
    __shared__ dbl2 s_pr[LDS ? P : 1][kWave];
    __shared__ dbl2 s_ey[LDS ? P : 1];
    // the zero-extended path's scalars (M_q, |y_q|) and -sgn(e_{P-1}): blk_step_zneg
    __shared__ dbl2 s_zm[LDS ? P : 1];
    __shared__ double s_zf;
    const int32_t* __restrict__ rfl = blk_rflags(mul, R);
    const int lane = threadIdx.x & (kWave - 1);
    const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // the pivots' rows and columns are NOT held here: the row flags say which rows are pivot
    // rows, and only the exact path (blk_exact_h) needs the indices, which it reads from h --
    // 2P fewer scalar registers (and spills) in the loop
    bool allok = true;
#pragma unroll
    for (int q = 0; q < P; ++q) allok = allok && h->ok[q] != 0;
    constexpr int kChunk = kBlkChunk;
    const int nchunks = (C + kChunk - 1) / kChunk;
    BlkChunk c;
    int base, qs;
    const BlkGeom g = LDS ? blk_geom_wg(nchunks, wib) : blk_geom_wave(nchunks, wib);
    c.ch = g.ch;
    base = g.base;
    qs = g.qs;
    int c0 = 0, K = 1, stride = 1, seg = R;
    if constexpr (ITEMS) {   // K row segments, item k at chunk (c0 + k * stride) % nchunks
        c0 = c.ch;
        K = max(1, min(g_sweep_items, nchunks));
        stride = max(1, nchunks / K);
        seg = ((R + K - 1) / K + qs - 1) / qs * qs;   // a multiple of qs: the same interleave
    }
    c.j = c.ch * kChunk + 2 * lane;
    std::conditional_t<LDS, BlkLdsOps<P>, BlkRegOps<P>> ops;
    if constexpr (LDS) {
        ops = BlkLdsOps<P>{s_pr, s_ey, s_zm, &s_zf, lane};
        ops.stage(pr, ld, c.ch, C);
        if (threadIdx.x < P) {
            const int q = threadIdx.x;
            const double e = h->e[q];
            s_ey[q] = dbl2{e, h->y[q]};
            const double M = q == 0 ? e : (h->e[q - 1] < 0.0 ? e : -e);
            s_zm[q] = dbl2{M, fabs(h->y[q])};
            if (q == P - 1) s_zf = e < 0.0 ? 1.0 : -1.0;
        }
        __syncthreads();
    } else {
#pragma unroll
        for (int q = 0; q < P; ++q) {
            ops.eq[q] = h->e[q];
            ops.yq[q] = h->y[q];
            ops.prs[q] = (c.j < C) ? *reinterpret_cast<const dbl2*>(pr + (int64_t)q * ld + c.j)
                             : dbl2{0.0, 0.0};
        }
    }
    // (the window-tracked path reads the operands through these two: with ops.pr / ops.ey
    // called there directly, FORM 6's and 7's kernels came out in another register order)
    auto PR = [&](int q) -> dbl2 { return ops.pr(q); };
    auto EY = [&](int q) -> dbl2 { return ops.ey(q); };
    const bool kNoFree = g_blk_nofree != 0;
    SMX_PC_DECL
    auto chunk_flags = [&]() {
        uint32_t et = 0, pt = 0;
        bool zok = true;   // every pivot-row value bounded or an exact +-0
#pragma unroll
        for (int q = 0; q < P; ++q) {
            const dbl2 p = ops.pr(q);
            et = max(et, bnd_term(ops.ey(q)[0]));
            if (c.j < C) {
                pt = max(pt, bnd_term(p[0]));
                zok = zok && bnd_or_zero(p[0]);
            }
            if (c.j + 1 < C) {
                pt = max(pt, bnd_term(p[1]));
                zok = zok && bnd_or_zero(p[1]);
            }
        }
        c.et = et;
        c.pz = zok;
        c.zok = !kNoFree && allok && et < kBndSpan && __all(zok);
        c.free = c.zok && __all(pt < kBndSpan);
    };
    chunk_flags();
    double eqa[P];   // the exact path's pivot elements (loaded there, rare)
    // Every vector load of the loop is this inline asm: a load the compiler can see (the slow
    // path's reload) made it put s_waitcnt vmcnt(0) at the head of the fast path, waiting for
    // the next row's prefetch before computing this row (sweep 990 us at P = 10, 16384^2, against
    // 750 us for the lab's loop, tools/sweep_lab.hip).
    c.jc = min(c.j, (C - 1) & ~1);
    auto ldc = [&](int row) {
        dbl2 v;
        const double* p = Tin + (int64_t)min(row, R - 1) * ld + c.jc;
        asm volatile("global_load_dwordx4 %0, %1, off nt" : "=v"(v) : "v"(p) : "memory");
        return v;
    };
    auto rowf = [&](dbl2 x0, int i0) {
        const double* m0 = mul + (int64_t)i0 * kBlkMax;
        double pc0[P];
#pragma unroll
        for (int q = 0; q < P; ++q) pc0[q] = m0[q];
        int rf = rfl[i0];
        // the row's flag and multipliers in ONE scalar round trip: left alone, the compiler
        // waits for the flag, branches, and only then issues the multipliers' loads
#pragma unroll
        for (int q = 0; q < P; ++q) asm volatile("" : "+s"(pc0[q]));
        asm volatile("" : "+s"(rf));
        dbl2 v0 = x0;
        bool ok = false;
        const uint32_t xt = max((uint32_t)__double2hiint(x0[0]) << 1,
                                (uint32_t)__double2hiint(x0[1]) << 1);
#ifdef SMX_PATH_COUNT
        if (!c.free) SMX_PC(kPcChunkNotFree);
        if (!c.zok) SMX_PC(kPcChunkNotZok);
        if (!(allok && c.et < kBndSpan)) SMX_PC(kPcChunkE);
        if (!__all(c.pz)) SMX_PC(kPcChunkP);
        if (rf == 0) SMX_PC(kPcRowFlag0);
        if (rf == 3) SMX_PC(kPcRowFlag3);
        if (c.free && rf == 1 && !__all(xt < kBndXMax)) SMX_PC(kPcXFail);
#endif
        if (c.free && rf == 1 && __all(xt < kBndXMax)) {
            SMX_PC(kPcFast);
            v0 = ops.fast(v0, pc0);
            ok = true;
        } else if (c.zok && (rf & 1) && __all(bnd_or_zero(x0[0]) && bnd_or_zero(x0[1]))) {
            // the zero-extended domain (rf 1 or 3, a chunk or row with exact zeros): the same
            // arithmetic, the division made zero-safe (blk_quot_zero / blk_step_zneg)
            asm volatile("" ::: "memory");   // keeps this path out of the fast path's code
            SMX_PC(kPcZero);
            v0 = ops.zero(v0, pc0);
            ok = true;
        } else if (allok && rf != 2) {   // not a pivot row (rf == 2): the window-tracked path
            // (the one place this step is written: as a function it changed every kernel),
            // numerators checked once per row by a vote.  Exact zeros are inside the domain too
            // (round 6): fd_zero's v_div_fixup gives a zero numerator its sign, every other
            // numerator must lie in the exponent window (a finite nonzero one in it, a normal
            // quotient: div_fixup returns the hoisted sequence's quotient unchanged).  A pivot
            // column's lane computes RN(x e) - RN(e x) = +0 at its step like on the fast path and
            // is rewritten by blk_fixcols.  (Counting zeros as outside sent every unit of a chunk
            // with a pivot-row value outside the bounds to the exact path on config 5's integer
            // tables -- a few chunks' waves 5-10x slower than the rest, block 0 at 2x block 2's
            // time with ~1.2x its instructions: profiles/r06i/7_paths.log, 8_pmcpaths/.)
            uint32_t wt = 0;
#pragma unroll
            for (int q = 0; q < P; ++q) {
                const dbl2 p = PR(q);
                const dbl2 ey = EY(q);
                const double e = ey[0], y = ey[1];
                double n[2];
                n[0] = v0[0] * e - p[0] * pc0[q];
                n[1] = v0[1] * e - p[1] * pc0[q];
                double rr[2];
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const uint32_t tk = win_term(n[k]);
                    wt = max(wt, (dbits(n[k]) << 1) == 0 ? 0u : tk);
                    rr[k] = fd_zero(n[k], e, y);
                }
                v0 = dbl2{rr[0], rr[1]};
            }
            ok = __all(wt < kWinSpan);
            SMX_PC(ok ? kPcWindow : kPcWindowFail);
        } else {
            SMX_PC(kPcExact);
        }
        if (!ok) {
            // reloaded (not written yet, even in place) so x0 need not stay live beside the
            // fast arithmetic; the wait covers the next row's prefetch too (rare path)
            x0 = ldc(i0);
            asm volatile("s_waitcnt vmcnt(0)" : "+v"(x0) :: "memory");
#pragma unroll
            for (int q = 0; q < P; ++q) eqa[q] = h->e[q];
            v0 = blk_exact_h<P>(x0, i0, c.j, h, eqa, ops, pc0);
        }
        if (c.j < C)
            __builtin_nontemporal_store(v0, reinterpret_cast<dbl2*>(Tout + (int64_t)i0 * ld + c.j));
    };
    // FORM 7: rows ia and ia + qs together (xa, xb: their inputs; hi: the end of the wave's rows)
    auto pairf = [&](dbl2 xa, dbl2 xb, int ia, int hi) {
        constexpr int NPH = (P + kPairPhase - 1) / kPairPhase;
        constexpr int P0 = P < kPairPhase ? P : kPairPhase;
        const int ib = ia + qs;
        const bool two = ib < hi;   // (false: an odd row left at the end of the wave's rows)
        const int ibc = two ? ib : ia;   // (nothing read past the table's rows)
        const double* ma = mul + (int64_t)ia * kBlkMax;
        const double* mb = mul + (int64_t)ibc * kBlkMax;
        int rfa = rfl[ia], rfb = rfl[ibc];
        asm volatile("" : "+s"(rfa));
        asm volatile("" : "+s"(rfb));
        const uint32_t xt = max(max((uint32_t)__double2hiint(xa[0]) << 1,
                                    (uint32_t)__double2hiint(xa[1]) << 1),
                                max((uint32_t)__double2hiint(xb[0]) << 1,
                                    (uint32_t)__double2hiint(xb[1]) << 1));
        if (two && c.free && rfa == 1 && rfb == 1 && __all(xt < kBndXMax)) {
            SMX_PC(kPcFast);   // two (row, chunk) units
            SMX_PC(kPcFast);
            dbl2 va = xa, vb = xb;
            double pa[P0], pb[P0];
#pragma unroll
            for (int ph = 0; ph < NPH; ++ph) {
                const int q0 = ph * kPairPhase;
                const int nq = P - q0 < kPairPhase ? P - q0 : kPairPhase;
                // This phase's multipliers of both rows, one scalar round trip, waited for in
                // place.  Their offset passes through an asm together with the chains' values, so
                // the loads are issued here, after the phase before, and not hoisted above it
                // (where two phases' scalars would be live and spill); the first phase's too:
                // loaded beside the flags, ahead of this branch, all 48 were spilled to vector
                // lanes on the way in and read back one by one here.  (The offset, not the
                // pointers: a pointer handed to an asm counts as captured, and every load of the
                // multipliers then turns into a vector load.)
                int o = q0;
                asm volatile("" : "+s"(o) : "v"(va), "v"(vb));
#pragma unroll
                for (int q = 0; q < nq; ++q) {
                    pa[q] = ma[o + q];
                    pb[q] = mb[o + q];
                }
#pragma unroll
                for (int q = 0; q < nq; ++q) {
                    asm volatile("" : "+s"(pa[q]));
                    asm volatile("" : "+s"(pb[q]));
                }
#pragma unroll
                for (int q = 0; q < nq; ++q)
                    blk_pair_step(va, vb, s_pr[q0 + q][lane], s_ey[q0 + q], pa[q], pb[q]);
            }
            // (the values pinned here: left alone, the compiler sinks the last phase's arithmetic
            // into the store's `c.j < C` branch and hoists every LDS read of it above the branch --
            // 124 VGPRs instead of 60 at P = 24)
            asm volatile("" : "+v"(va), "+v"(vb));
            if (c.j < C) {
                __builtin_nontemporal_store(va,
                                            reinterpret_cast<dbl2*>(Tout + (int64_t)ia * ld + c.j));
                __builtin_nontemporal_store(vb,
                                            reinterpret_cast<dbl2*>(Tout + (int64_t)ib * ld + c.j));
            }
        } else {
            // row by row (each loads its own flag and multipliers: not the bench's path)
#pragma nounroll
            for (int s = 0; s < (two ? 2 : 1); ++s) rowf(s ? xb : xa, s ? ib : ia);
        }
    };
    // FORM 8: rows ia, ia + qs, ia + 2 qs, ia + 3 qs together (x0..x3: their inputs; hi: the end of
    // the wave's rows)
    auto quadf = [&](dbl2 x0, dbl2 x1, dbl2 x2, dbl2 x3, int ia, int hi) {
        constexpr int NPH = (P + kQuadPhase - 1) / kQuadPhase;
        constexpr int P0 = P < kQuadPhase ? P : kQuadPhase;
        // rows of the quad inside the wave's rows (1-3: a tail, row by row)
        const int nr = ia + 3 * qs < hi ? 4 : ia + 2 * qs < hi ? 3 : ia + qs < hi ? 2 : 1;
        const bool four = nr == 4;
        const int i1 = four ? ia + qs : ia;   // (nothing read past the table's rows)
        const int i2 = four ? ia + 2 * qs : ia;
        const int i3 = four ? ia + 3 * qs : ia;
        const double* m0 = mul + (int64_t)ia * kBlkMax;
        const double* m1 = mul + (int64_t)i1 * kBlkMax;
        const double* m2 = mul + (int64_t)i2 * kBlkMax;
        const double* m3 = mul + (int64_t)i3 * kBlkMax;
        int rf0 = rfl[ia], rf1 = rfl[i1], rf2 = rfl[i2], rf3 = rfl[i3];
        asm volatile("" : "+s"(rf0));
        asm volatile("" : "+s"(rf1));
        asm volatile("" : "+s"(rf2));
        asm volatile("" : "+s"(rf3));
        auto hi2 = [](dbl2 x) {
            return max((uint32_t)__double2hiint(x[0]) << 1, (uint32_t)__double2hiint(x[1]) << 1);
        };
        const uint32_t xt = max(max(hi2(x0), hi2(x1)), max(hi2(x2), hi2(x3)));
        if (four && c.free && rf0 == 1 && rf1 == 1 && rf2 == 1 && rf3 == 1 &&
            __all(xt < kBndXMax)) {
            SMX_PC(kPcFast);   // four (row, chunk) units
            SMX_PC(kPcFast);
            SMX_PC(kPcFast);
            SMX_PC(kPcFast);
            dbl2 v0 = x0, v1 = x1, v2 = x2, v3 = x3;
            double p0[P0], p1[P0], p2[P0], p3[P0], pe[P0], py[P0];
#pragma unroll
            for (int ph = 0; ph < NPH; ++ph) {
                const int q0 = ph * kQuadPhase;
                const int nq = P - q0 < kQuadPhase ? P - q0 : kQuadPhase;
                // This phase's multipliers of the four rows and its pivots' e and y, one scalar
                // round trip, waited for in place; the offset tied to the chains' values as in
                // pairf (and for its reasons), so a phase's loads are issued after the phase before
                int o = q0;
                asm volatile("" : "+s"(o) : "v"(v0), "v"(v1), "v"(v2), "v"(v3));
#pragma unroll
                for (int q = 0; q < nq; ++q) {
                    p0[q] = m0[o + q];
                    p1[q] = m1[o + q];
                    p2[q] = m2[o + q];
                    p3[q] = m3[o + q];
                    pe[q] = h->e[o + q];
                    py[q] = h->y[o + q];
                }
#pragma unroll
                for (int q = 0; q < nq; ++q) {
                    asm volatile("" : "+s"(p0[q]));
                    asm volatile("" : "+s"(p1[q]));
                    asm volatile("" : "+s"(p2[q]));
                    asm volatile("" : "+s"(p3[q]));
                    asm volatile("" : "+s"(pe[q]));
                    asm volatile("" : "+s"(py[q]));
                }
#pragma unroll
                for (int q = 0; q < nq; ++q)
                    blk_quad_step(v0, v1, v2, v3, s_pr[q0 + q][lane], pe[q], py[q], p0[q], p1[q],
                                  p2[q], p3[q]);
            }
            // (pinned before the store's branch, as in pairf)
            asm volatile("" : "+v"(v0), "+v"(v1), "+v"(v2), "+v"(v3));
            if (c.j < C) {
                double* o0 = Tout + (int64_t)ia * ld + c.j;
                __builtin_nontemporal_store(v0, reinterpret_cast<dbl2*>(o0));
                __builtin_nontemporal_store(v1, reinterpret_cast<dbl2*>(o0 + (int64_t)qs * ld));
                __builtin_nontemporal_store(v2, reinterpret_cast<dbl2*>(o0 + 2 * (int64_t)qs * ld));
                __builtin_nontemporal_store(v3, reinterpret_cast<dbl2*>(o0 + 3 * (int64_t)qs * ld));
            }
        } else {
            // row by row (each loads its own flag and multipliers: not the bench's path)
#pragma nounroll
            for (int s = 0; s < nr; ++s)
                rowf(s == 0 ? x0 : s == 1 ? x1 : s == 2 ? x2 : x3, ia + s * qs);
        }
    };
    if constexpr (!ITEMS) {
        if (base >= R) return;
    }
    for (int it = 0; it < K; ++it) {
        int lo = 0, hi = R;
        if constexpr (ITEMS) {
            lo = it * seg;
            hi = min(R, lo + seg);
            if (it > 0) {
                // the next item's chunk: every wave is done with the previous slices first
                c.ch = (c0 + it * stride) % nchunks;
                c.j = c.ch * kChunk + 2 * lane;
                c.jc = min(c.j, (C - 1) & ~1);
                __syncthreads();
                if constexpr (LDS) ops.stage(pr, ld, c.ch, C);
                __syncthreads();
                chunk_flags();
            }
            if (lo + base >= hi) continue;   // (every wave still meets the barriers above)
        }
        // prefetch depth 1 over single rows: before a register set is used, the ops issued after
        // its load are the previous row's store and the other set's load (vmcnt(2); vmcnt(1)
        // first)
        const int r0 = lo + base;
        if constexpr (PAIRS) {
            blk_row_pairs(ldc, pairf, r0, qs, hi);
            continue;
        }
        if constexpr (QUADS) {
            blk_row_quads(ldc, quadf, r0, qs, hi);
            continue;
        }
        dbl2 a = ldc(r0), b = ldc(r0 + qs);
        asm volatile("s_waitcnt vmcnt(1)" : "+v"(a) :: "memory");
        for (int i0 = r0; i0 < hi; i0 += 2 * qs) {
            rowf(a, i0);
            if (i0 + qs >= hi) break;
            a = ldc(i0 + 2 * qs);
            asm volatile("s_waitcnt vmcnt(2)" : "+v"(b) :: "memory");
            rowf(b, i0 + qs);
            if (i0 + 2 * qs >= hi) break;
            b = ldc(i0 + 3 * qs);
            asm volatile("s_waitcnt vmcnt(2)" : "+v"(a) :: "memory");
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    SMX_PC_FLUSH;   // every exit of the loop lands here (diagnostic build only)
}

// After a flag-form sweep: every element of every pivot column, rewritten from the planner's
// multipliers.  For column c whose LAST pivot in the block is q, the element's value before step q
// is T_{k+q}[i][c] = mul[i][q] (bit for bit, the planner's own chain), so its steps q..P-1 follow
// from mul alone: step q's numerator is the element itself, or 1.0 on the pivot row
// (simplex.py:155-160); later steps apply the full rules with the exact division.  Writes `out`,
// the buffer the sweep wrote.  One (row, pivot) pair per thread, grid-stride.
__device__ __forceinline__ void blk_fixcols(double* out, int64_t ld, int R, int P,
                                            const BlkHdr* __restrict__ h,
                                            const double* __restrict__ mul,
                                            const double* __restrict__ pr) {
    // pairs ordered pivot-major (t = q R + i): a wave's lanes share q, so the pivot rows' values
    // at column c are one address per load; every operand of the chain is loaded before its
    // first step (the loop that loaded them step by step took 9-13 us per block at 16384^2 --
    // a memory round trip per step).  Row i's multipliers come from the transposed copy (the
    // planner's row pass writes it for every row but the f-row, R - 1): a wave's 64 rows are
    // then 8 lines per multiplier instead of 64.
    const double* mT = blk_mulT(mul, R);
    const int64_t pairs = (int64_t)R * P;
    for (int64_t t = (int64_t)blockIdx.x * kUpdBlock + threadIdx.x; t < pairs;
         t += (int64_t)gridDim.x * kUpdBlock) {
        const int q = (int)(t / R), i = (int)(t % R);
        const int c = h->c[q];
        bool last = true;
        for (int q2 = q + 1; q2 < P; ++q2) last = last && h->c[q2] != c;
        if (!last) continue;
        const double* mr = mul + (int64_t)i * kBlkMax;
        const bool frow = i == R - 1;
        double mq[kBlkMax], pc[kBlkMax], eq[kBlkMax];
        int rq[kBlkMax];
#pragma unroll
        for (int q2 = 0; q2 < kBlkMax; ++q2) {
            const bool act = q2 >= q && q2 < P;
            mq[q2] = act ? (frow ? mr[q2] : mT[(int64_t)q2 * R + i]) : 0.0;
            pc[q2] = (act && q2 > q) ? pr[(int64_t)q2 * ld + c] : 0.0;
            eq[q2] = act ? h->e[q2] : 1.0;
            rq[q2] = act ? h->r[q2] : -1;
        }
        double x = 0.0;
#pragma unroll
        for (int q2 = 0; q2 < kBlkMax; ++q2) {
            if (q2 < q || q2 >= P) continue;
            double num;
            if (q2 == q)
                num = (i == rq[q2]) ? 1.0 : mq[q2];
            else if (i == rq[q2])
                num = -x;   // c is not pivot q2's column (q is its last pivot)
            else
                num = x * eq[q2] - pc[q2] * mq[q2];
            x = num / eq[q2];
        }
        out[(int64_t)i * ld + c] = x;
    }
}

// Output: in place when ipx >= 0 and ipx + (pivots applied) is even, else into b_other; the
// chain state's loc records which buffer (in_idx = index of b_in) now holds the newest table.
__device__ __forceinline__ double* blk_out(double* b_in, double* b_other, int ipx, int in_idx,
                                           int applied, BlkHdr* __restrict__ hs) {
    const bool inplace = ipx >= 0 && ((ipx + applied) & 1) == 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) hs->loc = inplace ? in_idx : in_idx ^ 1;
    return inplace ? b_in : b_other;
}

// The sweep of a block that applied all P of its pivots (h->peff == P; otherwise it does nothing
// and k_blk_sweep_rest handles the block): one body per kernel, so the register allocation is
// that body's alone.  FORM 4 / 5 / 6 / 7 / 8: blk_sweep_body_flag's layouts.  Output per blk_out.
template <int P, int FORM>
__global__ __launch_bounds__(kUpdBlock) void k_blk_sweep(double* b_in, double* b_other, int64_t ld,
                                                         int R, int C,
                                                         const BlkHdr* __restrict__ h,
                                                         const double* __restrict__ mul,
                                                         const double* __restrict__ pr,
                                                         BlkHdr* __restrict__ hs, int ipx,
                                                         int in_idx) {
    if (h->peff != P) return;
    double* out = blk_out(b_in, b_other, ipx, in_idx, P, hs);
    blk_sweep_body_flag<P, FORM>(b_in, out, ld, R, C, h, pr, mul);
}

// After k_blk_sweep<P> (one launch, whichever case holds):
// * fix = 1 and the block applied all P pivots (flag form): blk_fixcols, the pivot columns;
// * a block that stopped early (a terminal outcome after 0 < peff < P pivots; once per LP):
//   every element through the peff pivots with the exact division, a rolled loop reading each
//   pivot's operands as it goes -- one small kernel for every count instead of a body per count;
// * otherwise nothing.
// * pctl != nullptr (the chain's last block): workgroup 0's first wave also publishes the chain's
//   final state (k_blk_publish's work, one launch and its gap fewer per chain).
__global__ __launch_bounds__(kUpdBlock) void k_blk_sweep_rest(double* b_in, double* b_other,
                                                              int64_t ld, int R, int C, int P,
                                                              const BlkHdr* __restrict__ h,
                                                              const double* __restrict__ mul,
                                                              const double* __restrict__ pr,
                                                              BlkHdr* __restrict__ hs, int ipx,
                                                              int in_idx, int fix, int ipx_full,
                                                              const smx_part* __restrict__ pparts,
                                                              int pnparts, int pslot, int pparity,
                                                              smx_ctl* __restrict__ pctl) {
    if (pctl != nullptr && blockIdx.x == 0 && threadIdx.x < kWave)
        blk_publish_wave(hs, pparts, pnparts, pslot, pparity, pctl);
    const int peff = h->peff;
    if (peff == P && fix) {
        double* out = (ipx_full >= 0 && ((ipx_full + P) & 1) == 0) ? b_in : b_other;
        blk_fixcols(out, ld, R, P, h, mul, pr);
        return;
    }
    if (peff <= 0 || peff >= P) return;
    double* out = blk_out(b_in, b_other, ipx, in_idx, peff, hs);
    const int64_t half = (C + 1) / 2;   // dbl2 units per row (ld is even)
    const int64_t units = (int64_t)R * half;
    for (int64_t u = (int64_t)blockIdx.x * kUpdBlock + threadIdx.x; u < units;
         u += (int64_t)gridDim.x * kUpdBlock) {
        const int i = (int)(u / half);
        const int j = (int)(u % half) * 2;
        double v[2] = {b_in[(int64_t)i * ld + j], j + 1 < C ? b_in[(int64_t)i * ld + j + 1] : 0.0};
        for (int q = 0; q < peff; ++q) {
            const int rq = h->r[q], cq = h->c[q];
            const double eq = h->e[q], mq = mul[(int64_t)i * kBlkMax + q];
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
                const int jj = j + hh;
                double num;
                if (i == rq) {
                    num = (jj == cq) ? 1.0 : -v[hh];
                } else {
                    const double a = v[hh] * eq;
                    const double b = pr[(int64_t)q * ld + (jj < C ? jj : j)] * mq;
                    num = (jj == cq) ? v[hh] : (a - b);
                }
                v[hh] = num / eq;
            }
        }
        out[(int64_t)i * ld + j] = v[0];
        if (j + 1 < C) out[(int64_t)i * ld + j + 1] = v[1];
    }
}

}  // namespace
