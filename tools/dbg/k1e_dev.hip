// k1e_dev.hip -- development harness (scratch, not product): K1e' (k_coarse_gmin16_dma) against K1e'' (k_coarse_gmin16_grp) on
// synthetic operands: Gaussian-mixture centroids and queries near them, bf16 head / tail and norms as k_split_bf16 makes them,
// the padding centroids' norms +inf.  Compares gpair of the two kernels bit for bit (20 launches per shape, a second stream
// copying memory under varying load; exits 1 at the first difference and prints its position) and times both, alternating.
// build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I../../include -o k1e_dev k1e_dev.hip
//        -DG16_TIMING: K1e'' also sums cycles per phase (wave 0 of each group: products, barrier, minima, barrier)
// run:   k1e_dev                 the small shapes and the headline shape: compare, then time the headline shape
//        k1e_dev time NQ C       time one shape only (for a profiler's pass)   k1e_dev time NQ C new|old   one kernel only
#include "../../multimedia-indexing_amd/csrc/mmidx_kernels.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#define CHECK(x)                                                                          \
    do {                                                                                  \
        hipError_t e_ = (x);                                                              \
        if (e_ != hipSuccess) {                                                           \
            printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); \
            exit(2);                                                                      \
        }                                                                                 \
    } while (0)

struct Shape {
    int nq, C, D;
};

struct Dev {
    __bf16 *Qh, *Ql, *Ch, *Cl;
    double *qn, *cn;
    float2 *g_old, *g_new;
    int nq, C, Cp, D, G;
};

static int g_cus = 256;

static void launch_old(const Dev &d, float2 *out, hipStream_t st) {
    const int ntiles = d.Cp / G16_BC, qblocks = (d.nq + G16_BQ - 1) / G16_BQ;
    const int csplit = std::max(1, std::min(ntiles, (512 + qblocks - 1) / qblocks));
    hipLaunchKernelGGL(k_coarse_gmin16_dma, dim3(qblocks, csplit), dim3(MMIDX_BLOCK), 0, st, d.Qh, d.Ql, d.Ch, d.Cl, d.cn, d.qn, out, d.Cp, d.nq, d.G);
}

static void launch_new(const Dev &d, float2 *out, hipStream_t st) {
    const int ntiles = d.Cp / G16_BC, qblocks = (d.nq + G16G_BQ - 1) / G16G_BQ;
    const int csplit = std::max({1, std::min(ntiles, (g_cus + qblocks - 1) / qblocks), (ntiles + G16G_NORM_TILES - 1) / G16G_NORM_TILES});
    hipLaunchKernelGGL(k_coarse_gmin16_grp, dim3(qblocks, csplit), dim3(G16G_BLOCK), 0, st, d.Qh, d.Ql, d.Ch, d.Cl, d.cn, d.qn, out, d.Cp, d.nq, d.G);
}

static Dev make(const Shape &s, unsigned seed) {
    Dev d{};
    d.nq = s.nq, d.C = s.C, d.D = s.D, d.Cp = (s.C + G16_BC - 1) / G16_BC * G16_BC, d.G = d.Cp / 8;
    const int Dp = G16_KC;
    std::mt19937_64 rng(seed);
    std::normal_distribution<double> N01(0.0, 1.0);
    const int ncen = s.C / 40 + 2;
    std::vector<double> cen((size_t)ncen * s.D), coarse((size_t)s.C * s.D), Q((size_t)s.nq * s.D);
    for (auto &v : cen) v = 4.0 * N01(rng);
    for (int c = 0; c < s.C; c++) {
        const int k = (int)(rng() % ncen);
        for (int j = 0; j < s.D; j++) coarse[(size_t)c * s.D + j] = cen[(size_t)k * s.D + j] + 0.7 * N01(rng);
    }
    for (int c = 0; c < std::min(20, s.C / 2); c++)  // duplicates: ties
        memcpy(&coarse[(size_t)(s.C / 2 + c) * s.D], &coarse[(size_t)c * s.D], (size_t)s.D * 8);
    for (int q = 0; q < s.nq; q++) {
        const int c = (int)(rng() % s.C);
        const double sig = q % 7 == 3 ? 0.0 : 0.05;
        for (int j = 0; j < s.D; j++) Q[(size_t)q * s.D + j] = q % 11 == 5 ? 5.0 * N01(rng) : coarse[(size_t)c * s.D + j] + sig * N01(rng);
    }
    double *dC, *dQ;
    CHECK(hipMalloc((void **)&dC, coarse.size() * 8));
    CHECK(hipMalloc((void **)&dQ, Q.size() * 8));
    CHECK(hipMemcpy(dC, coarse.data(), coarse.size() * 8, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dQ, Q.data(), Q.size() * 8, hipMemcpyHostToDevice));
    CHECK(hipMalloc((void **)&d.Qh, (size_t)s.nq * Dp * 2));
    CHECK(hipMalloc((void **)&d.Ql, (size_t)s.nq * Dp * 2));
    CHECK(hipMalloc((void **)&d.Ch, (size_t)d.Cp * Dp * 2));
    CHECK(hipMalloc((void **)&d.Cl, (size_t)d.Cp * Dp * 2));
    CHECK(hipMalloc((void **)&d.qn, (size_t)s.nq * 8));
    CHECK(hipMalloc((void **)&d.cn, (size_t)d.Cp * 8));
    CHECK(hipMalloc((void **)&d.g_old, (size_t)s.nq * d.G * 8));
    CHECK(hipMalloc((void **)&d.g_new, (size_t)s.nq * d.G * 8));
    CHECK(hipMemset(d.Ch, 0, (size_t)d.Cp * Dp * 2));
    CHECK(hipMemset(d.Cl, 0, (size_t)d.Cp * Dp * 2));
    std::vector<double> inf((size_t)d.Cp, std::numeric_limits<double>::infinity());
    CHECK(hipMemcpy(d.cn, inf.data(), inf.size() * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_split_bf16, dim3((s.C + 3) / 4), dim3(MMIDX_BLOCK), 0, 0, dC, d.Ch, d.Cl, (float *)nullptr, d.cn, s.D, Dp, (long long)s.C, (u32 *)nullptr);
    hipLaunchKernelGGL(k_split_bf16, dim3((s.nq + 3) / 4), dim3(MMIDX_BLOCK), 0, 0, dQ, d.Qh, d.Ql, (float *)nullptr, d.qn, s.D, Dp, (long long)s.nq, (u32 *)nullptr);
    CHECK(hipDeviceSynchronize());
    CHECK(hipFree(dC));
    CHECK(hipFree(dQ));
    return d;
}

static void drop(Dev &d) {
    hipFree(d.Qh), hipFree(d.Ql), hipFree(d.Ch), hipFree(d.Cl), hipFree(d.qn), hipFree(d.cn), hipFree(d.g_old), hipFree(d.g_new);
}

// 20 launches of the new kernel against one of the old, a second stream copying 0 .. 19 x 16 MiB meanwhile
static int compare(const Shape &s, hipStream_t st, hipStream_t st2, unsigned char *cp_a, unsigned char *cp_b) {
    Dev d = make(s, 1000u + (unsigned)(s.nq * 31 + s.C));
    const size_t words = (size_t)s.nq * d.G * 2;
    std::vector<unsigned> a(words), b(words);
    CHECK(hipMemsetAsync(d.g_old, 0xff, words * 4, st));
    launch_old(d, d.g_old, st);
    CHECK(hipGetLastError());
    CHECK(hipStreamSynchronize(st));
    CHECK(hipMemcpy(a.data(), d.g_old, words * 4, hipMemcpyDeviceToHost));
    for (int it = 0; it < 20; it++) {
        CHECK(hipMemsetAsync(d.g_new, 0xff, words * 4, st));
        for (int k = 0; k < it; k++) CHECK(hipMemcpyAsync(cp_b, cp_a, (size_t)16 << 20, hipMemcpyDeviceToDevice, st2));
        launch_new(d, d.g_new, st);
        CHECK(hipGetLastError());
        CHECK(hipStreamSynchronize(st));
        CHECK(hipStreamSynchronize(st2));
        CHECK(hipMemcpy(b.data(), d.g_new, words * 4, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < words; i++)
            if (a[i] != b[i]) {
                const size_t pair = i / 2;
                printf("DIFF nq %d C %d D %d launch %d: query %zu group %zu word %zu: old %08x new %08x\n", s.nq, s.C, s.D, it, pair / d.G, pair % d.G, i & 1, a[i], b[i]);
                return 1;
            }
    }
    printf("same  nq %6d C %5d D %3d: 20 launches, %zu words each\n", s.nq, s.C, s.D, words);
    drop(d);
    return 0;
}

static void time_shape(const Shape &s, hipStream_t st, int which) {
    Dev d = make(s, 77u);
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    const int reps = 20, rounds = 5;
    for (int w = 0; w < 3; w++) {
        if (which != 1) launch_old(d, d.g_old, st);
        if (which != 0) launch_new(d, d.g_new, st);
    }
    CHECK(hipStreamSynchronize(st));
#ifdef G16_TIMING
    unsigned long long zero[2][8] = {};
    CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g16g_cycles), zero, sizeof(zero)));
#endif
    for (int r = 0; r < rounds; r++) {
        float ms_old = 0.f, ms_new = 0.f;
        if (which != 1) {
            CHECK(hipEventRecord(e0, st));
            for (int i = 0; i < reps; i++) launch_old(d, d.g_old, st);
            CHECK(hipEventRecord(e1, st));
            CHECK(hipEventSynchronize(e1));
            CHECK(hipEventElapsedTime(&ms_old, e0, e1));
        }
        if (which != 0) {
            CHECK(hipEventRecord(e0, st));
            for (int i = 0; i < reps; i++) launch_new(d, d.g_new, st);
            CHECK(hipEventRecord(e1, st));
            CHECK(hipEventSynchronize(e1));
            CHECK(hipEventElapsedTime(&ms_new, e0, e1));
        }
        printf("time  nq %6d C %5d round %d: K1e' %8.2f us   K1e'' %8.2f us per launch\n", s.nq, s.C, r, ms_old * 1000.f / reps, ms_new * 1000.f / reps);
    }
#ifdef G16_TIMING
    if (which != 0) {
        unsigned long long cyc[2][8];
        CHECK(hipMemcpyFromSymbol(cyc, HIP_SYMBOL(g16g_cycles), sizeof(cyc)));
        static const char *nm[4] = {"products", "barrier", "minima", "barrier"};
        for (int g = 0; g < 2; g++) {
            printf("phase nq %6d C %5d group %d (memtime ticks per tile, wave %d):", s.nq, s.C, g, 4 * g);
            for (int i = 0; i < 4; i++) printf(" %s %.0f", nm[i], (double)cyc[g][i] / (double)std::max(1ull, cyc[g][7]));
            printf("\n");
        }
    }
#endif
    CHECK(hipEventDestroy(e0));
    CHECK(hipEventDestroy(e1));
    drop(d);
}

int main(int argc, char **argv) {
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    g_cus = prop.multiProcessorCount;
    printf("device %s, %d CUs\n", prop.name, g_cus);
    hipStream_t st, st2;
    CHECK(hipStreamCreate(&st));
    CHECK(hipStreamCreate(&st2));
    if (argc >= 4 && !strcmp(argv[1], "time")) {
        const int which = argc > 4 ? (!strcmp(argv[4], "old") ? 0 : 1) : 2;
        time_shape(Shape{atoi(argv[2]), atoi(argv[3]), 128}, st, which);
        return 0;
    }
    unsigned char *cp_a, *cp_b;
    CHECK(hipMalloc((void **)&cp_a, (size_t)16 << 20));
    CHECK(hipMalloc((void **)&cp_b, (size_t)16 << 20));
    CHECK(hipMemset(cp_a, 1, (size_t)16 << 20));
    const int Cs[] = {128, 384, 1000, 2049, 8192}, nqs[] = {1, 129, 256, 257, 600}, Ds[] = {128, 100};
    for (int D : Ds)
        for (int C : Cs)
            for (int nq : nqs)
                if (compare(Shape{nq, C, D}, st, st2, cp_a, cp_b)) return 1;
    // (the small shapes give every block ONE tile; these give 2, 3 and 1, 4, and at the headline shape 16 tiles a block)
    for (int nq : {1300, 2049, 4096})
        if (compare(Shape{nq, 8192, 128}, st, st2, cp_a, cp_b)) return 1;
    if (compare(Shape{16384, 8192, 128}, st, st2, cp_a, cp_b)) return 1;
    for (int nq : {256, 1024, 4096, 16384}) time_shape(Shape{nq, 8192, 128}, st, 2);
    return 0;
}
