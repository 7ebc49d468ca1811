// mmidx_learn.hip -- k-means codebook learning on the GPU (coarse and product quantizers).
//
// The reference learns its quantizers offline with Weka's SimpleKMeans
// (J/visual/quantization/AbstractQuantizerLearning.java:39-81, CoarseQuantizerLearning.java:39-72,
// ProductQuantizationLearning.java:247-305).  Weka 3.7.6 is a third-party dependency that is not in the
// reference tree (pom.xml), so this file restates the published algorithm -- Lloyd iterations with random or
// k-means++ seeding, optional min-max attribute normalisation (the default of Weka's EuclideanDistance), empty
// clusters dropped, stop when no assignment changes or at maxIterations -- and NOT Weka's exact random stream or
// floating-point order: learned codebooks are equivalent in kind, not bit-identical ("parity unpinned" for this
// row; tests pin the GPU path against a numpy restatement of the same algorithm from identical seeds instead).
//
// Arithmetic is deterministic: the assignment is the library's exact fp64 argmin (first index wins ties), and a
// centroid is the sum of its members in ascending index order divided by their number (stable radix sort by
// cluster, one block per cluster), so a CPU restatement reproduces the iterations bit for bit.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <set>
#include <vector>

#include "mmidx_host.h"
#include "mmidx_learn_kernels.h"

namespace {

typedef unsigned long long u64;

// java.util.Random (the generator Weka seeds with setSeed): 48-bit LCG, JDK javadoc
struct JavaRandom {
    u64 s;
    explicit JavaRandom(long long seed) : s(((u64)seed ^ 0x5DEECE66DULL) & ((1ULL << 48) - 1)) {}
    int next(int bits) {
        s = (s * 0x5DEECE66DULL + 0xBULL) & ((1ULL << 48) - 1);
        return (int)((long long)s >> (48 - bits));
    }
    int nextInt(int bound) {
        int r = next(31);
        const int m = bound - 1;
        if ((bound & m) == 0) return (int)(((long long)bound * (long long)r) >> 31);
        // Java's `u - r + m < 0` relies on int wrap-around (undefined in C++): the same test without overflow
        for (int u = r; (long long)u - (r = u % bound) + m >= (1LL << 31); u = next(31)) {
        }
        return r;
    }
    double nextDouble() { return (double)(((long long)next(26) << 27) + next(27)) * 0x1.0p-53; }
};

// per column minimum / maximum: one block per column
__global__ void k_col_minmax(const double *__restrict__ X, long long n, int d, double *__restrict__ mn, double *__restrict__ mx) {
    const int c = blockIdx.x;
    double lo = __longlong_as_double(0x7FF0000000000000ll), hi = -lo;
    for (long long i = threadIdx.x; i < n; i += blockDim.x) {
        const double v = X[(size_t)i * d + c];
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
    }
    __shared__ double s_lo[256], s_hi[256];
    s_lo[threadIdx.x] = lo;
    s_hi[threadIdx.x] = hi;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            s_lo[threadIdx.x] = s_lo[threadIdx.x + off] < s_lo[threadIdx.x] ? s_lo[threadIdx.x + off] : s_lo[threadIdx.x];
            s_hi[threadIdx.x] = s_hi[threadIdx.x + off] > s_hi[threadIdx.x] ? s_hi[threadIdx.x + off] : s_hi[threadIdx.x];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        mn[c] = s_lo[0];
        mx[c] = s_hi[0];
    }
}

// (x - min) / (max - min), 0 for a constant attribute (weka.core.NormalizableDistance.norm)
__global__ void k_normalize(const double *__restrict__ X, double *__restrict__ Y, const double *__restrict__ mn,
                            const double *__restrict__ mx, long long total, int d) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int c = (int)(e % d);
    const double r = mx[c] - mn[c];
    Y[e] = r > 0.0 ? (X[e] - mn[c]) / r : 0.0;
}

// k-means++: mind2[i] = min(mind2[i], |x_i - c|^2), sequential sum over the dimensions (one thread per row)
__global__ void k_pp_update(const double *__restrict__ X, const double *__restrict__ c, double *__restrict__ mind2, long long n, int d,
                            int first) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double acc = 0.0;
    for (int j = 0; j < d; j++) {
        const double df = X[(size_t)i * d + j] - c[j];
        acc += df * df;
    }
    mind2[i] = (first || acc < mind2[i]) ? acc : mind2[i];
}

// first index whose inclusive cumulative sum exceeds r (cum is non-decreasing); n - 1 if none
__global__ void k_pp_pick(const double *__restrict__ cum, long long n, double r, long long *__restrict__ out) {
    long long lo = 0, hi = n - 1;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (cum[mid] > r) hi = mid;
        else lo = mid + 1;
    }
    *out = lo;
}

// rows idx[0 .. m) of X[][d] -> out[m][d] (candidate seeds, compared on the host)
__global__ void k_gather_rows_ll(const double *__restrict__ X, const long long *__restrict__ idx, double *__restrict__ out, long long m, int d) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= m * d) return;
    const long long r = e / d;
    out[e] = X[(size_t)idx[r] * d + (size_t)(e - r * d)];
}

__global__ void k_iota(int32_t *__restrict__ v, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] = (int32_t)i;
}

// number of changed assignments and members per cluster
__global__ void k_changed_counts(const int32_t *__restrict__ a_old, const int32_t *__restrict__ a_new, long long n, u64 *__restrict__ changed,
                                 int32_t *__restrict__ counts) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int c = a_new[i];
    atomicAdd(counts + c, 1);
    if (a_old[i] != c) atomicAdd(changed, 1ULL);
}

// centroid c = (sum of its members in ascending index order) / count; one block per cluster, thread <-> dimension
__global__ __launch_bounds__(256) void k_centroid_mean(const double *__restrict__ X, const int32_t *__restrict__ sorted_idx,
                                                        const long long *__restrict__ off, double *__restrict__ C, int d) {
    const int c = blockIdx.x;
    const long long a = off[c], b = off[c + 1];
    if (b <= a) return;  // empty: the host drops the cluster
    for (int j = threadIdx.x; j < d; j += blockDim.x) {
        double acc = 0.0;
        for (long long m = a; m < b; m++) acc += X[(size_t)sorted_idx[m] * d + j];
        C[(size_t)c * d + j] = acc / (double)(b - a);
    }
}

// squared error: |x_i - C[a_i]|^2, sequential over dimensions; per-point values (summed in index order on the host)
__global__ void k_point_sqerr(const double *__restrict__ X, const double *__restrict__ C, const int32_t *__restrict__ a, double *__restrict__ out,
                              long long n, int d) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double *c = C + (size_t)a[i] * d;
    double acc = 0.0;
    for (int j = 0; j < d; j++) {
        const double df = X[(size_t)i * d + j] - c[j];
        acc += df * df;
    }
    out[i] = acc;
}

}  // namespace

extern "C" {

int mmidx_kmeans_device(int device, int64_t n, int d, int k, int max_iter, int64_t seed, int flags, const double *dX,
                        const double *init_centroids, double *centroids_out, int32_t *d_assign_out, double *sse_out, int32_t *iters_out,
                        int32_t *k_out, void *stream) {
    if (n < 1 || d < 1 || k < 1 || max_iter < 1 || !dX || !centroids_out)
        return mmidx_fail(MMIDX_ERR_INVALID_ARG, "k-means: n, d, k and max_iter must be positive, data and centroids_out non-null");
    if (n > (int64_t)INT32_MAX) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "k-means: more than 2^31 - 1 points");  // point indices, hipcub's item counts and the JDK draws are 32-bit
    if ((int64_t)k > n) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "k-means: k = %d exceeds the %lld points", k, (long long)n);  // Weka would stop seeding at n centroids; a codebook needs k <= n
    if (mmidx_device_count() < 1) return mmidx_fail(MMIDX_ERR_NO_DEVICE, "no HIP device: libmmidx_hip has no CPU fallback");
    HIPCK(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    const bool plus_plus = (flags & MMIDX_KMEANS_PLUS_PLUS) != 0, normalize = (flags & MMIDX_KMEANS_NORMALIZE) != 0;
    const size_t nd = (size_t)n * d;

    // ---- working copy of the data (normalised attributes: Weka's default distance) --------------------
    DevPtr<double> Xn, mn, mx;
    const double *W = dX;
    std::vector<double> h_mn((size_t)d, 0.0), h_mx((size_t)d, 1.0);
    if (normalize) {
        HIPCK(Xn.alloc(nd));
        HIPCK(mn.alloc((size_t)d));
        HIPCK(mx.alloc((size_t)d));
        hipLaunchKernelGGL(k_col_minmax, dim3((unsigned)d), dim3(256), 0, st, dX, (long long)n, d, mn.p, mx.p);
        hipLaunchKernelGGL(k_normalize, dim3((unsigned)((nd + 255) / 256)), dim3(256), 0, st, dX, Xn.p, mn.p, mx.p, (long long)nd, d);
        HIPCK(hipGetLastError());
        HIPCK(hipMemcpyAsync(h_mn.data(), mn.p, (size_t)d * 8, hipMemcpyDeviceToHost, st));
        HIPCK(hipMemcpyAsync(h_mx.data(), mx.p, (size_t)d * 8, hipMemcpyDeviceToHost, st));
        HIPCK(hipStreamSynchronize(st));
        W = Xn.p;
    }

    // ---- seeding ----------------------------------------------------------------------------------------
    std::vector<double> Ch((size_t)k * d);
    int k_seed = k;  // centres seeded: fewer than k when default seeding runs out of distinct rows
    DevPtr<double> dC;
    HIPCK(dC.alloc((size_t)k * d));
    if (init_centroids) {
        for (int c = 0; c < k; c++)
            for (int j = 0; j < d; j++) {
                const double v = init_centroids[(size_t)c * d + j], r = h_mx[(size_t)j] - h_mn[(size_t)j];
                Ch[(size_t)c * d + j] = normalize ? (r > 0.0 ? (v - h_mn[(size_t)j]) / r : 0.0) : v;
            }
    } else {
        JavaRandom rnd(seed);
        std::vector<long long> pick;
        pick.reserve((size_t)k);
        if (!plus_plus) {
            // SimpleKMeans' default seeding: walk j = n-1 .. 0, draw nextInt(j + 1), take that instance unless its (original,
            // un-normalised) row equals a centre already taken, swap it out of range either way; stop at k centres or when
            // the walk ends.  The draws do not depend on what is taken, so they are made in batches and the batch's rows
            // fetched in one gather to be compared here.
            std::vector<int32_t> perm((size_t)n);
            for (int64_t i = 0; i < n; i++) perm[(size_t)i] = (int32_t)i;
            const int64_t B = std::min<int64_t>(n, std::max<int64_t>(2 * (int64_t)k, 64));
            DevPtr<long long> didx;
            DevPtr<double> drows;
            HIPCK(didx.alloc((size_t)B));
            HIPCK(drows.alloc((size_t)B * d));
            std::vector<long long> cand;
            std::vector<double> rows;
            std::set<std::vector<double>> taken;  // (operator< on the values: -0.0 and 0.0 are one row, as in a == comparison)
            for (int64_t j = n - 1; j >= 0 && (int)pick.size() < k;) {
                const int64_t nb = std::min<int64_t>(j + 1, std::max<int64_t>(2 * (k - (int64_t)pick.size()), 64));
                cand.clear();
                for (int64_t t = 0; t < nb; t++, j--) {
                    const int r = rnd.nextInt((int)(j + 1));
                    cand.push_back(perm[(size_t)r]);
                    std::swap(perm[(size_t)j], perm[(size_t)r]);
                }
                rows.resize((size_t)nb * d);
                HIPCK(hipMemcpyAsync(didx.p, cand.data(), (size_t)nb * sizeof(long long), hipMemcpyHostToDevice, st));
                hipLaunchKernelGGL(k_gather_rows_ll, dim3((unsigned)((nb * d + 255) / 256)), dim3(256), 0, st, dX, didx.p, drows.p, (long long)nb, d);
                HIPCK(hipGetLastError());
                HIPCK(hipMemcpyAsync(rows.data(), drows.p, (size_t)nb * d * 8, hipMemcpyDeviceToHost, st));
                HIPCK(hipStreamSynchronize(st));
                for (int64_t t = 0; t < nb && (int)pick.size() < k; t++)
                    if (taken.emplace(rows.begin() + t * d, rows.begin() + (t + 1) * d).second) pick.push_back(cand[(size_t)t]);
            }
        } else {
            // k-means++ (Arthur & Vassilvitskii): first centre uniform, the others with probability ~ D^2
            DevPtr<double> mind2, cum;
            DevPtr<long long> dpick;
            DevPtr<unsigned char> tmp;
            HIPCK(mind2.alloc((size_t)n));
            HIPCK(cum.alloc((size_t)n));
            HIPCK(dpick.alloc(1));
            size_t tb = 0;
            HIPCK(hipcub::DeviceScan::InclusiveSum(nullptr, tb, mind2.p, cum.p, (int)n, st));
            HIPCK(tmp.alloc(tb));
            pick.push_back(rnd.nextInt((int)n));
            for (int c = 1; c < k; c++) {
                hipLaunchKernelGGL(k_pp_update, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, W, W + (size_t)pick.back() * d, mind2.p,
                                   (long long)n, d, c == 1 ? 1 : 0);
                HIPCK(hipcub::DeviceScan::InclusiveSum(tmp.p, tb, mind2.p, cum.p, (int)n, st));
                double total = 0.0;
                HIPCK(hipMemcpyAsync(&total, cum.p + (n - 1), 8, hipMemcpyDeviceToHost, st));
                HIPCK(hipStreamSynchronize(st));
                const double prob = rnd.nextDouble();
                long long idx = 0;
                hipLaunchKernelGGL(k_pp_pick, dim3(1), dim3(1), 0, st, cum.p, (long long)n, prob * total, dpick.p);
                HIPCK(hipMemcpyAsync(&idx, dpick.p, 8, hipMemcpyDeviceToHost, st));
                HIPCK(hipStreamSynchronize(st));
                pick.push_back(idx);
            }
        }
        // gather the picked rows
        for (size_t c = 0; c < pick.size(); c++)
            HIPCK(hipMemcpyAsync(Ch.data() + c * d, W + (size_t)pick[c] * d, (size_t)d * 8, hipMemcpyDeviceToHost, st));
        HIPCK(hipStreamSynchronize(st));
        k_seed = (int)pick.size();
    }

    // ---- Lloyd iterations -------------------------------------------------------------------------------
    DevPtr<int32_t> a_old, a_new, iota, sorted_idx, keys_out, counts;
    DevPtr<long long> off;
    DevPtr<u64> changed;
    DevPtr<unsigned char> stmp;
    HIPCK(a_old.alloc((size_t)n));
    HIPCK(a_new.alloc((size_t)n));
    HIPCK(iota.alloc((size_t)n));
    HIPCK(sorted_idx.alloc((size_t)n));
    HIPCK(keys_out.alloc((size_t)n));
    HIPCK(counts.alloc((size_t)k));
    HIPCK(off.alloc((size_t)k + 1));
    HIPCK(changed.alloc(1));
    HIPCK(hipMemsetAsync(a_old.p, 0xFF, (size_t)n * 4, st));
    hipLaunchKernelGGL(k_iota, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, iota.p, (long long)n);
    int kbits = 1;
    while ((1 << kbits) < k) kbits++;
    size_t sb = 0;
    HIPCK(hipcub::DeviceRadixSort::SortPairs(nullptr, sb, a_new.p, keys_out.p, iota.p, sorted_idx.p, (int)n, 0, kbits, st));
    HIPCK(stmp.alloc(sb));

    int k_eff = k_seed, iters = 0;
    std::vector<int32_t> h_counts((size_t)k);
    std::vector<long long> h_off((size_t)k + 1);
    mmidx_index *h = nullptr;
    int rc = MMIDX_OK;
    auto sort_and_mean = [&](const double *data, double *d_out) -> int {
        HIPCK(hipcub::DeviceRadixSort::SortPairs(stmp.p, sb, a_new.p, keys_out.p, iota.p, sorted_idx.p, (int)n, 0, kbits, st));
        hipLaunchKernelGGL(k_centroid_mean, dim3((unsigned)k_eff), dim3(256), 0, st, data, sorted_idx.p, off.p, d_out, d);
        HIPCK(hipGetLastError());
        return MMIDX_OK;
    };
    for (;;) {
        iters++;
        if (h) mmidx_destroy(h);
        h = nullptr;
        rc = mmidx_create(MMIDX_KIND_IVFPQ, d, 1, 2, k_eff, MMIDX_TR_NONE, nullptr, nullptr, device, &h);
        if (rc) break;
        rc = mmidx_set_coarse(h, Ch.data());
        if (rc) break;
        rc = mmidx_assign_device(h, n, W, a_new.p, st);
        if (rc) break;
        HIPCK(hipMemsetAsync(changed.p, 0, 8, st));
        HIPCK(hipMemsetAsync(counts.p, 0, (size_t)k_eff * 4, st));
        hipLaunchKernelGGL(k_changed_counts, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a_old.p, a_new.p, (long long)n, changed.p, counts.p);
        u64 nchanged = 0;
        HIPCK(hipMemcpyAsync(&nchanged, changed.p, 8, hipMemcpyDeviceToHost, st));
        HIPCK(hipMemcpyAsync(h_counts.data(), counts.p, (size_t)k_eff * 4, hipMemcpyDeviceToHost, st));
        HIPCK(hipStreamSynchronize(st));
        h_off[0] = 0;
        for (int c = 0; c < k_eff; c++) h_off[(size_t)c + 1] = h_off[(size_t)c] + h_counts[(size_t)c];
        HIPCK(hipMemcpyAsync(off.p, h_off.data(), ((size_t)k_eff + 1) * 8, hipMemcpyHostToDevice, st));
        rc = sort_and_mean(W, dC.p);
        if (rc) break;
        HIPCK(hipMemcpyAsync(Ch.data(), dC.p, (size_t)k_eff * d * 8, hipMemcpyDeviceToHost, st));
        HIPCK(hipStreamSynchronize(st));
        const bool done = nchanged == 0 || iters >= max_iter;
        // empty clusters are dropped (SimpleKMeans: m_NumClusters -= emptyClusterCount); the survivors keep their order
        int kept = 0;
        for (int c = 0; c < k_eff; c++) {
            if (h_counts[(size_t)c] > 0) {
                if (kept != c) memcpy(Ch.data() + (size_t)kept * d, Ch.data() + (size_t)c * d, (size_t)d * 8);
                kept++;
            }
        }
        const bool dropped = kept != k_eff;
        if (done) {
            if (dropped) {
                // renumber the final assignment to the compacted codebook
                std::vector<int32_t> remap((size_t)k_eff, -1);
                int t = 0;
                for (int c = 0; c < k_eff; c++)
                    if (h_counts[(size_t)c] > 0) remap[(size_t)c] = t++;
                std::vector<int32_t> ha((size_t)n);
                HIPCK(hipMemcpyAsync(ha.data(), a_new.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
                HIPCK(hipStreamSynchronize(st));
                for (int64_t i = 0; i < n; i++) ha[(size_t)i] = remap[(size_t)ha[(size_t)i]];
                HIPCK(hipMemcpyAsync(a_new.p, ha.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
                HIPCK(hipStreamSynchronize(st));  // (ha is freed at the end of this block)
                // offsets of the compacted numbering
                int t2 = 0;
                h_off[0] = 0;
                for (int c = 0; c < k_eff; c++)
                    if (h_counts[(size_t)c] > 0) {
                        h_off[(size_t)t2 + 1] = h_off[(size_t)t2] + h_counts[(size_t)c];
                        t2++;
                    }
                HIPCK(hipMemcpyAsync(off.p, h_off.data(), ((size_t)kept + 1) * 8, hipMemcpyHostToDevice, st));
            }
            k_eff = kept;
            break;
        }
        k_eff = kept;
        std::swap(a_old.p, a_new.p);
        if (dropped) HIPCK(hipMemsetAsync(a_old.p, 0xFF, (size_t)n * 4, st));  // numbering changed: everything counts as moved
    }
    if (h) mmidx_destroy(h);
    if (rc) return rc;

    // ---- outputs ------------------------------------------------------------------------------------------
    // squared error in the space the clustering ran in (what SimpleKMeans.getSquaredError reports)
    if (sse_out) {
        DevPtr<double> perr;
        HIPCK(perr.alloc((size_t)n));
        HIPCK(hipMemcpyAsync(dC.p, Ch.data(), (size_t)k_eff * d * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_point_sqerr, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, W, dC.p, a_new.p, perr.p, (long long)n, d);
        std::vector<double> he((size_t)n);
        HIPCK(hipMemcpyAsync(he.data(), perr.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
        HIPCK(hipStreamSynchronize(st));
        double s = 0.0;
        for (int64_t i = 0; i < n; i++) s += he[(size_t)i];
        *sse_out = s;
    }
    if (normalize) {
        // centroids in the original space = means of the original vectors over the final assignment
        // (SimpleKMeans.moveCentroid averages the un-normalised instances)
        int rc2 = sort_and_mean(dX, dC.p);
        if (rc2) return rc2;
        HIPCK(hipMemcpyAsync(Ch.data(), dC.p, (size_t)k_eff * d * 8, hipMemcpyDeviceToHost, st));
        HIPCK(hipStreamSynchronize(st));
    }
    memcpy(centroids_out, Ch.data(), (size_t)k_eff * d * 8);
    if (d_assign_out) HIPCK(hipMemcpyAsync(d_assign_out, a_new.p, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
    HIPCK(hipStreamSynchronize(st));
    if (iters_out) *iters_out = iters;
    if (k_out) *k_out = k_eff;
    return MMIDX_OK;
}

int mmidx_kmeans(int device, int64_t n, int d, int k, int max_iter, int64_t seed, int flags, const double *X, const double *init_centroids,
                 double *centroids_out, int32_t *assign_out, double *sse_out, int32_t *iters_out, int32_t *k_out) {
    if (n < 1 || d < 1 || !X || n > (int64_t)INT32_MAX) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "k-means: n and d must be positive (n < 2^31), data non-null");
    if (mmidx_device_count() < 1) return mmidx_fail(MMIDX_ERR_NO_DEVICE, "no HIP device: libmmidx_hip has no CPU fallback");
    HIPCK(hipSetDevice(device));
    DevPtr<double> dX;
    DevPtr<int32_t> dA;
    HIPCK(dX.alloc((size_t)n * d));
    HIPCK(dA.alloc((size_t)n));
    HIPCK(hipMemcpy(dX.p, X, (size_t)n * d * 8, hipMemcpyHostToDevice));
    int rc = mmidx_kmeans_device(device, n, d, k, max_iter, seed, flags, dX.p, init_centroids, centroids_out, dA.p, sse_out, iters_out, k_out,
                                 nullptr);
    if (rc) return rc;
    if (assign_out) HIPCK(hipMemcpy(assign_out, dA.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return MMIDX_OK;
}

}  // extern "C"

// ---- the product quantizer in one device-resident call ------------------------------------------------------
namespace {

struct PlJobResult {
    std::vector<double> cent;  // [k_eff][dsub]
    double sse = 0.0;
    int k_eff = 0, iters = 0;
};

// everything the groups of one call share
struct PlCtx {
    hipStream_t st = nullptr;
    long long n = 0, ntl = 0;
    int m = 0, ks = 0, dsub = 0, DS = 0, max_iter = 0, repeats = 0, G = 0;
    bool normalize = false;
    const double *Y = nullptr, *W = nullptr;  // [m][n][dsub]: the data, and the space the clustering runs in (the normalised copy, or Y itself)
    DevPtr<int32_t> assign, iota, sorted, pick, cnt, ctlB;
    DevPtr<uint32_t> keys_in, keys_out;
    DevPtr<double> mind2, tsum, tinc, prob, Ctab, Cfin, sse;
    DevPtr<PlSlot> slots;
    DevPtr<unsigned char> stmp;
    size_t stmp_bytes = 0;
    PinBuf<PlSlot> h_slots;
    PinBuf<int32_t> h_pick0, h_cnt, h_ctlB;
    PinBuf<double> h_prob, h_sse, h_cent;
};

template <int DS>
void pl_launch_assign(const PlCtx &c, int nact, size_t lds) {
    hipLaunchKernelGGL(k_pl_assign<DS>, dim3((unsigned)((c.n + PL_APTS - 1) / PL_APTS), (unsigned)nact), dim3(PL_BLOCK), lds, c.st, c.W, c.slots.p,
                       c.Ctab.p, c.assign.p, c.keys_in.p, c.cnt.p, (uint32_t *)(c.cnt.p + (size_t)nact * c.ks), c.n, c.dsub, c.ks);
}

// jobs g0 .. g0 + Gc of the call, start to finish: seeding, Lloyd iterations, squared error, reported centroids
int pl_run_group(PlCtx &c, int g0, int Gc, std::vector<PlJobResult> &res) {
    const long long n = c.n;
    const int ks = c.ks, dsub = c.dsub, G = c.G;
    hipStream_t st = c.st;
    // ---- seeding: every draw comes from the job's own JavaRandom(seed) and none depends on the data, so all are made up front
    for (int jl = 0; jl < Gc; jl++) {
        const int g = g0 + jl;
        JavaRandom rnd((long long)(g % c.repeats) + 1);
        c.h_pick0.p[(size_t)jl * ks] = rnd.nextInt((int)n);  // (the rest of the row is written by the pick kernel)
        for (int t = 0; t + 1 < ks; t++) c.h_prob.p[(size_t)jl * (ks - 1) + t] = rnd.nextDouble();
        c.h_slots.p[jl] = PlSlot{jl, g / c.repeats, ks, 1};
    }
    HIPCK(hipMemcpyAsync(c.pick.p, c.h_pick0.p, (size_t)Gc * ks * 4, hipMemcpyHostToDevice, st));
    HIPCK(hipMemcpyAsync(c.prob.p, c.h_prob.p, (size_t)Gc * (ks - 1) * 8, hipMemcpyHostToDevice, st));
    HIPCK(hipMemcpyAsync(c.slots.p, c.h_slots.p, (size_t)Gc * sizeof(PlSlot), hipMemcpyHostToDevice, st));
    for (int t = 1; t < ks; t++) {
        hipLaunchKernelGGL(k_pl_pp_update, dim3((unsigned)c.ntl, (unsigned)Gc), dim3(PL_BLOCK), 0, st, c.W, c.slots.p, c.pick.p, c.mind2.p,
                           c.tsum.p, n, dsub, ks, t, c.ntl);
        hipLaunchKernelGGL(k_pl_pp_pick, dim3((unsigned)Gc), dim3(PL_BLOCK), 0, st, c.mind2.p, c.tsum.p, c.tinc.p, c.prob.p, c.slots.p, c.pick.p,
                           n, ks, t, c.ntl);
    }
    hipLaunchKernelGGL(k_pl_gather_seeds, dim3((unsigned)((ks * dsub + PL_BLOCK - 1) / PL_BLOCK), (unsigned)Gc), dim3(PL_BLOCK), 0, st, c.W,
                       c.slots.p, c.pick.p, c.Ctab.p, n, dsub, ks);
    HIPCK(hipGetLastError());

    // ---- Lloyd iterations: one wait per iteration for all jobs together ---------------------------------------------------------
    std::vector<int> k_eff((size_t)Gc, ks), iters((size_t)Gc, 0), force((size_t)Gc, 1), act((size_t)Gc);
    for (int jl = 0; jl < Gc; jl++) act[(size_t)jl] = jl;
    // ctlB: kept [G] | done list [G] | rng_a [G][ks] | rng_b [G][ks] | remap [G][ks]
    int32_t *hb_kept = c.h_ctlB.p, *hb_done = hb_kept + G, *hb_a = hb_done + G, *hb_b = hb_a + (size_t)G * ks, *hb_remap = hb_b + (size_t)G * ks;
    const int32_t *db_kept = c.ctlB.p, *db_done = db_kept + G, *db_a = db_done + G, *db_b = db_a + (size_t)G * ks, *db_remap = db_b + (size_t)G * ks;
    const size_t ctlB_ints = 2 * (size_t)G + 3 * (size_t)G * ks;
    const unsigned cgrid = (unsigned)((ks * dsub + PL_BLOCK - 1) / PL_BLOCK);
    std::vector<int> next_act;
    next_act.reserve((size_t)Gc);
    while (!act.empty()) {
        const int nact = (int)act.size();
        const size_t cnt_ints = (size_t)nact * ks + (size_t)nact;  // the live slots only: counts [slot][ks], then changed [slot]
        int kmax = 0;
        for (int s = 0; s < nact; s++) {
            const int jl = act[(size_t)s];
            iters[(size_t)jl]++;
            c.h_slots.p[s] = PlSlot{jl, (g0 + jl) / c.repeats, k_eff[(size_t)jl], force[(size_t)jl]};
            kmax = std::max(kmax, k_eff[(size_t)jl]);
        }
        HIPCK(hipMemcpyAsync(c.slots.p, c.h_slots.p, (size_t)nact * sizeof(PlSlot), hipMemcpyHostToDevice, st));
        HIPCK(hipMemsetAsync(c.cnt.p, 0, cnt_ints * 4, st));
        const size_t lds = (size_t)kmax * dsub * 8 + (size_t)kmax * 4;
        if (c.DS == 4) pl_launch_assign<4>(c, nact, lds);
        else if (c.DS == 8) pl_launch_assign<8>(c, nact, lds);
        else pl_launch_assign<16>(c, nact, lds);
        HIPCK(hipGetLastError());
        HIPCK(hipMemcpyAsync(c.h_cnt.p, c.cnt.p, cnt_ints * 4, hipMemcpyDeviceToHost, st));
        // stable grouping of all active jobs' points by (slot, cluster)
        int bits = 1;
        while ((1ll << bits) < (long long)nact * ks) bits++;
        const int items = (int)((long long)nact * n);
        size_t need = 0;
        HIPCK(hipcub::DeviceRadixSort::SortPairs(nullptr, need, c.keys_in.p, c.keys_out.p, c.iota.p, c.sorted.p, items, 0, bits, st));
        if (need > c.stmp_bytes) {  // (sized for the largest sort; fewer items are not expected to ask for more)
            HIPCK(hipStreamSynchronize(st));
            HIPCK(c.stmp.alloc(need));
            c.stmp_bytes = need;
        }
        HIPCK(hipcub::DeviceRadixSort::SortPairs(c.stmp.p, c.stmp_bytes, c.keys_in.p, c.keys_out.p, c.iota.p, c.sorted.p, items, 0, bits, st));
        HIPCK(hipStreamSynchronize(st));

        // host: who is done, which clusters emptied (SimpleKMeans: m_NumClusters -= emptyClusterCount; the survivors keep their order)
        int ndone = 0;
        next_act.clear();
        for (int s = 0; s < nact; s++) {
            const int jl = act[(size_t)s], ke = k_eff[(size_t)jl];
            const int32_t *cn = c.h_cnt.p + (size_t)s * ks;
            const uint32_t moved = (uint32_t)c.h_cnt.p[(size_t)nact * ks + s];
            long long off = (long long)s * n;
            int kept = 0;
            for (int k = 0; k < ke; k++) {
                hb_remap[(size_t)s * ks + k] = cn[k] > 0 ? kept : -1;
                if (cn[k] > 0) {
                    hb_a[(size_t)s * ks + kept] = (int32_t)off;
                    hb_b[(size_t)s * ks + kept] = (int32_t)(off + cn[k]);
                    kept++;
                }
                off += cn[k];
            }
            hb_kept[s] = kept;
            const bool done = moved == 0 || iters[(size_t)jl] >= c.max_iter;
            force[(size_t)jl] = kept != ke;  // numbering changed: everything counts as moved, for this job only
            k_eff[(size_t)jl] = kept;
            if (done) hb_done[ndone++] = s;
            else next_act.push_back(jl);
        }
        HIPCK(hipMemcpyAsync(c.ctlB.p, c.h_ctlB.p, ctlB_ints * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_pl_means, dim3(cgrid, (unsigned)nact), dim3(PL_BLOCK), 0, st, c.W, c.slots.p, (const int32_t *)nullptr, c.sorted.p, db_a,
                           db_b, db_kept, c.Ctab.p, n, dsub, ks);
        if (ndone) {
            // the squared error in the space the clustering ran in, summed in index order; with normalisation the reported
            // centroids are the means of the original members (SimpleKMeans.moveCentroid)
            hipLaunchKernelGGL(k_pl_sqerr, dim3((unsigned)((n + PL_BLOCK - 1) / PL_BLOCK), (unsigned)ndone), dim3(PL_BLOCK), 0, st, c.W, c.slots.p,
                               db_done, c.Ctab.p, c.assign.p, db_remap, c.mind2.p, n, dsub, ks);
            hipLaunchKernelGGL(k_pl_seqsum, dim3((unsigned)ndone), dim3(PL_BLOCK), 0, st, c.mind2.p, c.slots.p, db_done, c.sse.p, n);
            if (c.normalize)
                hipLaunchKernelGGL(k_pl_means, dim3(cgrid, (unsigned)ndone), dim3(PL_BLOCK), 0, st, c.Y, c.slots.p, db_done, c.sorted.p, db_a, db_b,
                                   db_kept, c.Cfin.p, n, dsub, ks);
        }
        HIPCK(hipGetLastError());
        act.swap(next_act);
    }
    HIPCK(hipMemcpyAsync(c.h_sse.p, c.sse.p, (size_t)Gc * 8, hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(c.h_cent.p, c.normalize ? c.Cfin.p : c.Ctab.p, (size_t)Gc * ks * dsub * 8, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    for (int jl = 0; jl < Gc; jl++) {
        PlJobResult &r = res[(size_t)(g0 + jl)];
        r.k_eff = k_eff[(size_t)jl];
        r.iters = iters[(size_t)jl];
        r.sse = c.h_sse.p[jl];
        r.cent.assign(c.h_cent.p + (size_t)jl * ks * dsub, c.h_cent.p + ((size_t)jl * ks + r.k_eff) * dsub);
    }
    return MMIDX_OK;
}

// the refusals that need no device, shared by the host and the device entry
int pl_check_args(int64_t n, int D, int m, int ks, int max_iter, int repeats, int flags, const void *X, int C, const double *coarse, int transform,
                  const int32_t *perm, const double *rot, const double *pq_out) {
    if (!X || !pq_out) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "pq learn: null argument (the vectors and pq_out are required)");
    if (n < 1 || D < 1 || m < 1 || ks < 1 || max_iter < 1 || repeats < 1)
        return mmidx_fail(MMIDX_ERR_INVALID_ARG, "pq learn: n, D, m, ks, max_iter and repeats must be positive");
    if ((int64_t)ks > n) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "pq learn: ks = %d exceeds the %lld vectors", ks, (long long)n);
    if (flags & ~MMIDX_KMEANS_NORMALIZE) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "pq learn: flags accepts MMIDX_KMEANS_NORMALIZE only (the seeding is always k-means++)");
    if (C < 0 || (C > 0 && !coarse) || (C == 0 && coarse))
        return mmidx_fail(MMIDX_ERR_INVALID_ARG, "pq learn: C coarse centroids need a coarse array, and none (flat PQ) is C = 0 with NULL");
    if (D % m) return mmidx_fail(MMIDX_ERR_INVALID_SUBVECTORS, "The given number of subvectors is not valid!");
    if (transform != MMIDX_TR_NONE && transform != MMIDX_TR_ROTATION && transform != MMIDX_TR_PERMUTATION)
        return mmidx_fail(MMIDX_ERR_INVALID_ARG, "pq learn: unknown transformation %d", transform);
    if (transform == MMIDX_TR_PERMUTATION && !perm) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "pq learn: a permutation needs perm[D]");
    if (transform == MMIDX_TR_ROTATION && !rot) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "pq learn: a rotation needs rot[D][D]");
    if (n > (int64_t)INT32_MAX) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "pq learn: more than 2^31 - 1 vectors");  // point indices, the JDK draws
    const int dsub = D / m;
    if (dsub > PL_MAX_DSUB)
        return mmidx_fail(MMIDX_ERR_UNSUPPORTED, "pq learn: dsub = %d exceeds the limit dsub <= %d of the batched learner (use mmidx_kmeans per sub-space)", dsub,
                          PL_MAX_DSUB);
    if ((int64_t)ks * dsub * 8 > 65536)
        return mmidx_fail(MMIDX_ERR_UNSUPPORTED, "pq learn: a table of ks x dsub = %d x %d doubles exceeds the limit ks * dsub * 8 <= 64 KiB of LDS", ks, dsub);
    if ((int64_t)m * repeats > (int64_t)INT32_MAX) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "pq learn: m * repeats exceeds 2^31 - 1");
    return MMIDX_OK;
}

}  // namespace

extern "C" {

int mmidx_pq_learn_device(int device, int64_t n, int D, int m, int ks, int max_iter, int repeats, int flags, const double *dX, int C,
                          const double *coarse, int transform, const int32_t *perm, const double *rot, double *pq_out, double *sse_out,
                          int32_t *seed_out, int32_t *k_out, int32_t *iters_out, void *stream) {
    int rc = pl_check_args(n, D, m, ks, max_iter, repeats, flags, dX, C, coarse, transform, perm, rot, pq_out);
    if (rc) return rc;
    if (mmidx_device_count() < 1) return mmidx_fail(MMIDX_ERR_NO_DEVICE, "no HIP device: libmmidx_hip has no CPU fallback");
    HIPCK(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    const int dsub = D / m, J = m * repeats;
    const size_t nd = (size_t)n * D;
    PlCtx c;
    c.st = st;
    c.n = n;
    c.ntl = (n + PL_TILE - 1) / PL_TILE;
    c.m = m;
    c.ks = ks;
    c.dsub = dsub;
    c.DS = dsub <= 4 ? 4 : dsub <= 8 ? 8 : 16;
    c.max_iter = max_iter;
    c.repeats = repeats;
    c.normalize = (flags & MMIDX_KMEANS_NORMALIZE) != 0;

    // ---- prep: nearest coarse centroid, residual, transform, sub-space-major; the normalised copy -------------------------------
    DevPtr<double> Y, Yn, mn, mx, d_coarse, d_rot;
    DevPtr<int32_t> d_cell, d_perm;
    HIPCK(Y.alloc(nd));
    if (C > 0) {
        HIPCK(d_cell.alloc((size_t)n));
        HIPCK(d_coarse.alloc((size_t)C * D));
        HIPCK(hipMemcpyAsync(d_coarse.p, coarse, (size_t)C * D * 8, hipMemcpyHostToDevice, st));
        mmidx_index *h = nullptr;  // one scratch handle for the whole call
        rc = mmidx_create(MMIDX_KIND_IVFPQ, D, 1, 2, C, MMIDX_TR_NONE, nullptr, nullptr, device, &h);
        if (!rc) rc = mmidx_set_coarse(h, coarse);
        if (!rc) rc = mmidx_assign_device(h, n, dX, d_cell.p, st);
        if (!rc && hipStreamSynchronize(st) != hipSuccess) rc = mmidx_fail(MMIDX_ERR_HIP, "pq learn: the coarse assignment failed");
        if (h) mmidx_destroy(h);
        if (rc) return rc;
    }
    if (transform == MMIDX_TR_PERMUTATION) {
        HIPCK(d_perm.alloc((size_t)D));
        HIPCK(hipMemcpyAsync(d_perm.p, perm, (size_t)D * 4, hipMemcpyHostToDevice, st));
    } else if (transform == MMIDX_TR_ROTATION) {
        HIPCK(d_rot.alloc((size_t)D * D));
        HIPCK(hipMemcpyAsync(d_rot.p, rot, (size_t)D * D * 8, hipMemcpyHostToDevice, st));
    }
    hipLaunchKernelGGL(k_pl_prep, dim3((unsigned)((nd + PL_BLOCK - 1) / PL_BLOCK)), dim3(PL_BLOCK), 0, st, dX, d_cell.p, d_coarse.p, d_perm.p, d_rot.p,
                       Y.p, (long long)n, D, dsub, transform, C > 0 ? 1 : 0);
    c.Y = c.W = Y.p;
    if (c.normalize) {
        HIPCK(Yn.alloc(nd));
        HIPCK(mn.alloc((size_t)D));
        HIPCK(mx.alloc((size_t)D));
        hipLaunchKernelGGL(k_pl_minmax, dim3((unsigned)D), dim3(PL_BLOCK), 0, st, Y.p, (long long)n, dsub, mn.p, mx.p);
        hipLaunchKernelGGL(k_pl_normalize, dim3((unsigned)((nd + PL_BLOCK - 1) / PL_BLOCK)), dim3(PL_BLOCK), 0, st, Y.p, Yn.p, mn.p, mx.p, (long long)n,
                           dsub, (long long)nd);
        c.W = Yn.p;
    }
    HIPCK(hipGetLastError());
    HIPCK(hipStreamSynchronize(st));  // (perm / rot / coarse are the caller's: their copies are done)

    // ---- jobs per group: the sort's 32-bit item count, the memory that is free, and the test switch ---------------------------------
    size_t free_b = 0, total_b = 0;
    HIPCK(hipMemGetInfo(&free_b, &total_b));
    const size_t per_job = (size_t)n * 48 + (size_t)ks * dsub * 16 + 4096;  // five int32 / uint32 arrays, mind2, the sort's workspace
    long long G = std::min<long long>(std::min<long long>(J, 65535), (long long)INT32_MAX / n);  // (a grid's y extent walks the jobs)
    G = std::min<long long>(G, (long long)(free_b / 10 * 8 / per_job));
    if (const char *e = getenv("MMIDX_PQ_LEARN_GROUP")) {
        const long long v = atoll(e);
        if (v >= 1) G = std::min<long long>(G, v);
    }
    if (G < 1) G = 1;
    c.G = (int)G;
    const size_t Gn = (size_t)G * n;
    HIPCK(c.assign.alloc(Gn));
    HIPCK(c.iota.alloc(Gn));
    HIPCK(c.sorted.alloc(Gn));
    HIPCK(c.keys_in.alloc(Gn));
    HIPCK(c.keys_out.alloc(Gn));
    HIPCK(c.mind2.alloc(Gn));
    HIPCK(c.tsum.alloc((size_t)G * c.ntl));
    HIPCK(c.tinc.alloc((size_t)G * c.ntl));
    HIPCK(c.pick.alloc((size_t)G * ks));
    HIPCK(c.prob.alloc((size_t)G * ks));
    HIPCK(c.Ctab.alloc((size_t)G * ks * dsub));
    if (c.normalize) HIPCK(c.Cfin.alloc((size_t)G * ks * dsub));
    HIPCK(c.sse.alloc((size_t)G));
    HIPCK(c.slots.alloc((size_t)G));
    HIPCK(c.cnt.alloc((size_t)G * ks + (size_t)G));
    HIPCK(c.ctlB.alloc(2 * (size_t)G + 3 * (size_t)G * ks));
    HIPCK(c.h_slots.alloc((size_t)G));
    HIPCK(c.h_pick0.alloc((size_t)G * ks));
    memset(c.h_pick0.p, 0, (size_t)G * ks * 4);
    HIPCK(c.h_prob.alloc((size_t)G * ks));
    HIPCK(c.h_cnt.alloc((size_t)G * ks + (size_t)G));
    HIPCK(c.h_ctlB.alloc(2 * (size_t)G + 3 * (size_t)G * ks));
    HIPCK(c.h_sse.alloc((size_t)G));
    HIPCK(c.h_cent.alloc((size_t)G * ks * dsub));
    {
        int bits = 1;
        while ((1ll << bits) < (long long)G * ks) bits++;
        HIPCK(hipcub::DeviceRadixSort::SortPairs(nullptr, c.stmp_bytes, c.keys_in.p, c.keys_out.p, c.iota.p, c.sorted.p, (int)Gn, 0, bits, st));
        HIPCK(c.stmp.alloc(c.stmp_bytes));
    }
    hipLaunchKernelGGL(k_pl_iota_mod, dim3((unsigned)((Gn + PL_BLOCK - 1) / PL_BLOCK)), dim3(PL_BLOCK), 0, st, c.iota.p, (long long)n, (long long)Gn);
    // the assignment's LDS: a table of at most 64 KiB and its histogram of at most 32 KiB
    HIPCK(hipFuncSetAttribute((const void *)k_pl_assign<4>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
    HIPCK(hipFuncSetAttribute((const void *)k_pl_assign<8>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
    HIPCK(hipFuncSetAttribute((const void *)k_pl_assign<16>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
    HIPCK(hipGetLastError());

    std::vector<PlJobResult> res((size_t)J);
    for (int g0 = 0; g0 < J; g0 += (int)G) {
        rc = pl_run_group(c, g0, std::min<int>((int)G, J - g0), res);
        if (rc) return rc;
    }

    // ---- the kept repeat of every sub-space: seeds 1..repeats in order, replaced only on sse < best (ProductQuantizationLearning.java:252-269)
    for (int s = 0; s < m; s++) {
        int best = 0;
        for (int r = 1; r < repeats; r++)
            if (res[(size_t)s * repeats + r].sse < res[(size_t)s * repeats + best].sse) best = r;
        const PlJobResult &b = res[(size_t)s * repeats + best];
        double *out = pq_out + (size_t)s * ks * dsub;
        std::copy(b.cent.begin(), b.cent.end(), out);
        std::fill(out + (size_t)b.k_eff * dsub, out + (size_t)ks * dsub, 1000.0);  // missing centres: far-away fakes (:285-302)
        if (sse_out) sse_out[s] = b.sse;
        if (seed_out) seed_out[s] = best + 1;
        if (k_out) k_out[s] = b.k_eff;
        if (iters_out) iters_out[s] = b.iters;
    }
    return MMIDX_OK;
}

int mmidx_pq_learn(int device, int64_t n, int D, int m, int ks, int max_iter, int repeats, int flags, const double *X, int C, const double *coarse,
                   int transform, const int32_t *perm, const double *rot, double *pq_out, double *sse_out, int32_t *seed_out, int32_t *k_out,
                   int32_t *iters_out) {
    int rc = pl_check_args(n, D, m, ks, max_iter, repeats, flags, X, C, coarse, transform, perm, rot, pq_out);
    if (rc) return rc;
    if (mmidx_device_count() < 1) return mmidx_fail(MMIDX_ERR_NO_DEVICE, "no HIP device: libmmidx_hip has no CPU fallback");
    HIPCK(hipSetDevice(device));
    DevPtr<double> dX;
    HIPCK(dX.alloc((size_t)n * D));
    HIPCK(hipMemcpy(dX.p, X, (size_t)n * D * 8, hipMemcpyHostToDevice));
    return mmidx_pq_learn_device(device, n, D, m, ks, max_iter, repeats, flags, dX.p, C, coarse, transform, perm, rot, pq_out, sse_out, seed_out, k_out,
                                 iters_out, nullptr);
}

}  // extern "C"
