// scenario_shape_probe.hip -- the A/B of DESIGN 9.6: the production k_batch_scenario (step 2 reads
// the changed columns straight from the base table, next to a flat copy) against the tiled shape
// (the copy goes by tiles of 64 rows x 32 columns staged in wave-private LDS with a padded stride,
// lane = row walks each tile's changed columns).  Synthetic operands: B uniform tables of n x m
// under one seeded permutation of the labels, S scenarios each with deltas on a quarter of the
// entries.  The two outputs are compared byte for byte, then both are timed by HIP events,
// alternating, `reps` launches each, three rounds.
// Build (from the repo root):
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -Iinclude -I/opt/rocm/include \
//     -L/opt/rocm/lib -lrccl tools/scenario_shape_probe.hip -o tools/scenario_shape_probe
// Run: tools/scenario_shape_probe [n=100] [m=100] [B=2048] [S=8] [reps=10]
#include "../simplex-method-solver_amd/csrc/smx_kernels.hip"

#include <algorithm>
#include <random>

namespace {

constexpr int kTC = 32;            // tile columns
constexpr int kTLd = kTC + 1;      // padded stride (doubles)

__global__ __launch_bounds__(kScnBlock) void k_scenario_tiled(
    const double* __restrict__ final, const int32_t* __restrict__ dims, int B, int S, int Rmax,
    int ldb, const int32_t* __restrict__ basis, const int32_t* __restrict__ nonbasis,
    const double* __restrict__ func, const double* __restrict__ drhs,
    const double* __restrict__ dcost, double* tabs_s, double* __restrict__ func_s,
    int32_t* __restrict__ dims_s) {
    extern __shared__ double s_t[];
    const int q = blockIdx.x;
    const int b = q / S;
    if (b >= B) return;
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = dims[3 * b], m = dims[3 * b + 1];
    const double* T = final + (size_t)b * Rmax * ldb;
    double* So = tabs_s + (size_t)q * Rmax * ldb;
    if (tid < 3) dims_s[3 * (size_t)q + tid] = dims[3 * b + tid];
    const bool inside = n >= 1 && m >= 1 && n < Rmax && m < ldb;
    const double* fb = func + (size_t)b * ldb;
    const double* dc = dcost + (size_t)q * ldb;
    const double* dr = drhs + (size_t)q * Rmax;
    double* fs = func_s + (size_t)q * ldb;
    for (int k = tid; k < ldb; k += kScnBlock)
        fs[k] = (inside && k < m) ? scn_own(fb[k], dc[k]) : 0.0;
    if (!inside) {
        const int cnt = Rmax * ldb;
        for (int e = tid; e < cnt; e += kScnBlock) So[e] = T[e];
        return;
    }
    const int32_t* bb = basis + (size_t)b * Rmax;
    const int32_t* nb = nonbasis + (size_t)b * ldb;
    const double* Tf = T + (size_t)n * ldb;
    double* Sf = So + (size_t)n * ldb;
    // ---- step 1 as in production; nothing else has written row n yet
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
    __syncthreads();
    // ---- the copy by tiles, step 2 folded in
    double* tile = s_t + (size_t)wid * kWave * kTLd;
    const int cc = lane & (kTC - 1), rr = lane >> 5;
    for (int p0 = wid * kWave; p0 < Rmax; p0 += kScnBlock) {
        const int p = p0 + lane;
        const bool on = p <= n;
        double v = 0.0;
        if (on) v = p < n ? T[(size_t)p * ldb + m] : Sf[m];
        if (p < n) v = scn_own(v, scn_delta(bb[p], m, m + n, dr));
        for (int j0 = 0; j0 < ldb; j0 += kTC) {
            const int j = j0 + cc;
            for (int r = 0; r < kWave; r += 2) {
                const int row = p0 + r + rr;
                if (row < Rmax && j < ldb) {
                    const bool mine = row == n && j <= m;            // step 1 wrote it
                    const double t = mine ? Sf[j] : T[(size_t)row * ldb + j];
                    if (!mine && !(j == m && row < n)) So[(size_t)row * ldb + j] = t;
                    tile[(r + rr) * kTLd + cc] = t;
                }
            }
            sol_wave_sync();
            const int jl = j0 + lane;
            const double d = (lane < kTC && jl < m) ? scn_delta(nb[jl], m, m + n, dr) : 0.0;
            unsigned long long mask = __ballot(d != 0.0);
            while (mask) {
                const int l = __builtin_ctzll(mask);
                mask &= mask - 1;
                const double s = on ? tile[lane * kTLd + l] : 0.0;
                v = scn_rhs_term(v, s, readlane_d(d, l));
            }
            sol_wave_sync();
        }
        if (on) So[(size_t)p * ldb + m] = v;
    }
}

#define CK(x)                                                                    \
    do {                                                                         \
        hipError_t e_ = (x);                                                     \
        if (e_ != hipSuccess) {                                                  \
            printf("%s failed: %s\n", #x, hipGetErrorString(e_));                \
            return 1;                                                            \
        }                                                                        \
    } while (0)

}  // namespace

int main(int argc, char** argv) {
    const int n = argc > 1 ? atoi(argv[1]) : 100, m = argc > 2 ? atoi(argv[2]) : 100;
    const int B = argc > 3 ? atoi(argv[3]) : 2048, S = argc > 4 ? atoi(argv[4]) : 8;
    const int reps = argc > 5 ? atoi(argv[5]) : 10;
    const int Rmax = n + 1, ldb = m + 1;
    if (n < 1 || m < 1 || B < 1 || S < 1 || reps < 1 || !smx_batch_scenario_fits(Rmax, ldb)) {
        printf("bad arguments\n");
        return 1;
    }
    const size_t blk = (size_t)Rmax * ldb, Q = (size_t)B * S;
    std::mt19937_64 g(7);
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    std::vector<double> h_T(B * blk), h_func((size_t)B * ldb), h_dr(Q * Rmax, 0.0), h_dc(Q * ldb, 0.0);
    for (auto& v : h_T) v = u(g);
    for (auto& v : h_func) v = u(g);
    for (auto& v : h_dr) v = u(g) < -0.5 ? u(g) : 0.0;
    for (auto& v : h_dc) v = u(g) < -0.5 ? u(g) : 0.0;
    std::vector<int32_t> perm(n + m), h_ba((size_t)B * Rmax, -1), h_nb((size_t)B * ldb, -1), h_dims(3 * B);
    for (int i = 0; i < n + m; ++i) perm[i] = i;
    std::shuffle(perm.begin(), perm.end(), g);
    for (int b = 0; b < B; ++b) {
        for (int i = 0; i < n; ++i) h_ba[(size_t)b * Rmax + i] = perm[i];
        for (int j = 0; j < m; ++j) h_nb[(size_t)b * ldb + j] = perm[n + j];
        h_dims[3 * b] = n, h_dims[3 * b + 1] = m, h_dims[3 * b + 2] = m;
    }
    double *T, *func, *dr, *dc, *oa, *ob, *fa, *fb2;
    int32_t *ba, *nb, *dims, *da, *db;
    CK(hipMalloc(&T, h_T.size() * 8));
    CK(hipMalloc(&func, h_func.size() * 8));
    CK(hipMalloc(&dr, h_dr.size() * 8));
    CK(hipMalloc(&dc, h_dc.size() * 8));
    CK(hipMalloc(&oa, Q * blk * 8));
    CK(hipMalloc(&ob, Q * blk * 8));
    CK(hipMalloc(&fa, Q * ldb * 8));
    CK(hipMalloc(&fb2, Q * ldb * 8));
    CK(hipMalloc(&ba, h_ba.size() * 4));
    CK(hipMalloc(&nb, h_nb.size() * 4));
    CK(hipMalloc(&dims, h_dims.size() * 4));
    CK(hipMalloc(&da, Q * 3 * 4));
    CK(hipMalloc(&db, Q * 3 * 4));
    CK(hipMemcpy(T, h_T.data(), h_T.size() * 8, hipMemcpyHostToDevice));
    CK(hipMemcpy(func, h_func.data(), h_func.size() * 8, hipMemcpyHostToDevice));
    CK(hipMemcpy(dr, h_dr.data(), h_dr.size() * 8, hipMemcpyHostToDevice));
    CK(hipMemcpy(dc, h_dc.data(), h_dc.size() * 8, hipMemcpyHostToDevice));
    CK(hipMemcpy(ba, h_ba.data(), h_ba.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(nb, h_nb.data(), h_nb.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dims, h_dims.data(), h_dims.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemset(oa, 0x11, Q * blk * 8));
    CK(hipMemset(ob, 0x22, Q * blk * 8));
    const size_t lds = (size_t)kScnWaves * kWave * kTLd * sizeof(double);
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_scenario_tiled),
                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    auto plain = [&]() {
        hipLaunchKernelGGL(k_batch_scenario, dim3((unsigned)Q), dim3(kScnBlock), 0, 0, T, dims, B,
                           S, Rmax, ldb, ba, nb, func, dr, dc, oa, fa, da);
    };
    auto tiled = [&]() {
        hipLaunchKernelGGL(k_scenario_tiled, dim3((unsigned)Q), dim3(kScnBlock), lds, 0, T, dims,
                           B, S, Rmax, ldb, ba, nb, func, dr, dc, ob, fb2, db);
    };
    plain();
    tiled();
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    std::vector<double> ha(Q * blk), hb(Q * blk);
    CK(hipMemcpy(ha.data(), oa, Q * blk * 8, hipMemcpyDeviceToHost));
    CK(hipMemcpy(hb.data(), ob, Q * blk * 8, hipMemcpyDeviceToHost));
    const bool same = memcmp(ha.data(), hb.data(), Q * blk * 8) == 0;
    printf("{\"what\": \"scenario_kernel_shape\", \"n\": %d, \"m\": %d, \"lps\": %d, \"scenarios\": %d, "
           "\"outputs_equal\": %s, \"tiled_lds_bytes\": %zu", n, m, B, S, same ? "true" : "false", lds);
    if (!same) {
        printf("}\n");
        return 2;
    }
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    for (int which = 0; which < 2; ++which) {
        printf(", \"%s_ms\": [", which ? "tiled" : "plain");
        for (int round = 0; round < 3; ++round) {
            CK(hipEventRecord(e0, 0));
            for (int r = 0; r < reps; ++r) which ? tiled() : plain();
            CK(hipEventRecord(e1, 0));
            CK(hipEventSynchronize(e1));
            float ms = 0;
            CK(hipEventElapsedTime(&ms, e0, e1));
            printf("%s%.5f", round ? ", " : "", ms / reps);
        }
        printf("]");
    }
    printf(", \"copy_bytes\": %zu}\n", 2 * Q * blk * 8);
    return 0;
}
