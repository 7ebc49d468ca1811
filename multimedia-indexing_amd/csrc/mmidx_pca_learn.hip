// mmidx_pca_learn.hip -- learning the PCA basis on the GPU: PCA.addSample / computeBasis (J/dimreduction/PCA.java:120-177).
//
// The reference keeps the samples in A[numSamples][sampleSize], computes the column means with a sequential loop, centres A and
// takes V_t and W from EJML's dense SVD, sorted descending, first numComponents rows.  Here:
//   means       k_pca_colsum: a thread per column adds the rows in arrival order into a running fp64 sum (the reference's loop,
//               :142-153, continued across add calls), one division by numSamples on the host -- BIT-EXACT.
//   Gram        k_pca_gram: G = (A - mu)^T (A - mu) on v_mfma_f64_16x16x4_f64, lower-triangle tiles, mirrored.
//   eigenpairs  top-nc of G by blocked subspace iteration with Rayleigh-Ritz, block width b = min(ss, nc + 32): Z = G Q (K7,
//               k_pca_project with a zero mean), T = Q^T Z (k_pca_gram with two operands), eigen-solve of the b x b matrix T on the
//               host, V = Q W, residuals ||G v_i - lambda_i v_i|| = ||Z w_i - lambda_i v_i||, Q <- CholeskyQR2(Z W).
//   finish      k_pca_finish: sv = sqrt(max(lambda, 0)), the sign rule (largest-magnitude entry of a row positive, lowest index on
//               a tie), transpose to Vt[nc][ss].
// EJML is absent from the reference tree and its SVD cannot be reproduced bit for bit (assumption A2): components and singular
// values are right singular vectors / values of A - mu in the mathematical sense, row signs by the rule above (EJML's are
// arbitrary).  sv are the singular values of the CENTRED SAMPLE MATRIX, not divided by n or n - 1: what PCA.savePCAToFile writes on
// line 2 (W.get(i, i), :234-237) and the loader whitens with value^-0.5 (:283-285).
// Everything is deterministic: fixed start block, no atomics, no split reductions whose order depends on scheduling.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "mmidx_host.h"
#include "mmidx_small_solve.h"
#include "mmidx_dense_solve.h"

namespace {

typedef __attribute__((ext_vector_type(4))) double f64x4;

// ------------------------------------------------------------------------------------------------
// column sums: sum[c] += X[r][c], r = 0 .. n-1 in order (PCA.java:144-149).  A thread per column, a wave reads 512 contiguous
// bytes of a row; eight rows are requested together and added one after the other (the additions stay sequential).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_pca_colsum(const double *__restrict__ X, long long n, int ss, double *__restrict__ sum) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= ss) return;
    double s = sum[c];
    const double *x = X + c;
    long long r = 0;
    for (; r + 8 <= n; r += 8) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = x[(size_t)(r + u) * ss];
#pragma unroll
        for (int u = 0; u < 8; u++) s += v[u];
    }
    for (; r < n; r++) s += x[(size_t)r * ss];
    sum[c] = s;
}

// ------------------------------------------------------------------------------------------------
// Gram: C[sa][sb] = (A[n][sa] - muA)^T (B[n][sb] - muB), the contraction runs over the n ROWS.  The transposed-operand
// counterpart of K7: both operands are read along their rows (contiguous) for GR_BK consecutive samples, the mean is subtracted
// while staging, tiles go through LDS as [k][column] with a row stride of 16 doubles past a multiple of 32 -- a fragment read is
// 16 consecutive doubles per k (lane & 15) for four k (lane >> 4), and with that stride the two k of a 32-lane half fall on
// disjoint halves of the 64 banks (ds_read_b64: bank = (addr / 4) mod 64).  Block = 4 waves, tile 64 x 128: wave w owns rows
// 16w .. 16w+15 of the tile and its 8 column tiles, as K7 (64 accumulator registers, four waves per SIMD).
// A operand: one f64 per lane, A[i = lane & 15][k = lane >> 4]; B[k = lane >> 4][j = lane & 15]; C/D: col = lane & 15,
// row = (lane >> 4) + 4 * reg.
// SYM (A == B): only tiles that touch the lower triangle run; an element (i >= j) is written to C[i][j] and C[j][i] by the one
// tile that owns it, so the matrix is exactly symmetric and no element is written twice.
// ------------------------------------------------------------------------------------------------
#define GR_BM 64
#define GR_BN 128
#ifndef GR_BK
#define GR_BK 8
#endif
#define GR_NT 256
#define GR_LDA (GR_BM + 16)
#define GR_LDB (GR_BN + 16)
#define GR_NA (GR_BK * GR_BM / 2 / GR_NT)  // pairs of doubles per thread: A tile
#define GR_NB (GR_BK * GR_BN / 2 / GR_NT)  // ... B tile

// ACC (the streaming learner's fold, SYM only): a tile starts from the stored values of the elements it owns instead of from zero,
// C += (A - muA)^T (B - muB); the mirrored copy is rewritten with the same value.  Ownership is what it is without ACC, so no element
// is read or written by two tiles and the sum of a fold does not depend on scheduling.
template <bool SYM, bool ACC = false>
__global__ __launch_bounds__(GR_NT, 4) void k_pca_gram(const double *__restrict__ A, const double *__restrict__ B, const double *__restrict__ muA,
                                                       const double *__restrict__ muB, double *__restrict__ Cm, long long n, int sa, int sb) {
    __shared__ __attribute__((aligned(16))) double As[GR_BK * GR_LDA];
    __shared__ __attribute__((aligned(16))) double Bs[GR_BK * GR_LDB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i0 = blockIdx.y * GR_BM, j0 = blockIdx.x * GR_BN;
    if (SYM && i0 + GR_BM - 1 < j0) return;  // strictly above the diagonal (block-uniform)
    f64x4 acc[8];
#pragma unroll
    for (int t = 0; t < 8; t++) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
    if constexpr (ACC) {
        static_assert(SYM, "the accumulating form exists for the symmetric Gram matrix only");
#pragma unroll
        for (int t = 0; t < 8; t++) {
            const int j = j0 + t * 16 + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int i = i0 + wave * 16 + (lane >> 4) + 4 * r;
                if (i < sa && j < sb && i >= j) acc[t][r] = Cm[(size_t)i * sb + j];
            }
        }
    }
    // staging: thread <-> (k, pair of columns); the means of its columns stay in registers
    double2 ra[GR_NA], rb[GR_NB], ma[GR_NA], mb[GR_NB];
#pragma unroll
    for (int u = 0; u < GR_NA; u++) {
        const int c = i0 + ((tid + u * GR_NT) % (GR_BM / 2)) * 2;
        ma[u] = make_double2(c < sa ? muA[c] : 0.0, c + 1 < sa ? muA[c + 1] : 0.0);
    }
#pragma unroll
    for (int u = 0; u < GR_NB; u++) {
        const int c = j0 + ((tid + u * GR_NT) % (GR_BN / 2)) * 2;
        mb[u] = make_double2(c < sb ? muB[c] : 0.0, c + 1 < sb ? muB[c + 1] : 0.0);
    }
    auto load_tiles = [&](long long k0) {
#pragma unroll
        for (int u = 0; u < GR_NA; u++) {
            const int p = tid + u * GR_NT, k = p / (GR_BM / 2), c = i0 + (p % (GR_BM / 2)) * 2;
            const long long gr = k0 + k;
            double2 v = make_double2(0.0, 0.0);  // rows past n and columns past sa contribute nothing
            if (gr < n) {
                const double *src = A + (size_t)gr * sa + c;
                if (c < sa) v.x = src[0] - ma[u].x;
                if (c + 1 < sa) v.y = src[1] - ma[u].y;
            }
            ra[u] = v;
        }
#pragma unroll
        for (int u = 0; u < GR_NB; u++) {
            const int p = tid + u * GR_NT, k = p / (GR_BN / 2), c = j0 + (p % (GR_BN / 2)) * 2;
            const long long gr = k0 + k;
            double2 v = make_double2(0.0, 0.0);
            if (gr < n) {
                const double *src = B + (size_t)gr * sb + c;
                if (c < sb) v.x = src[0] - mb[u].x;
                if (c + 1 < sb) v.y = src[1] - mb[u].y;
            }
            rb[u] = v;
        }
    };
    auto store_tiles = [&]() {
#pragma unroll
        for (int u = 0; u < GR_NA; u++) {
            const int p = tid + u * GR_NT, k = p / (GR_BM / 2), c = (p % (GR_BM / 2)) * 2;
            *(double2 *)(As + k * GR_LDA + c) = ra[u];
        }
#pragma unroll
        for (int u = 0; u < GR_NB; u++) {
            const int p = tid + u * GR_NT, k = p / (GR_BN / 2), c = (p % (GR_BN / 2)) * 2;
            *(double2 *)(Bs + k * GR_LDB + c) = rb[u];
        }
    };
    const int fr = lane & 15, fk = lane >> 4;
    load_tiles(0);
    for (long long k0 = 0; k0 < n; k0 += GR_BK) {
        __syncthreads();
        store_tiles();
        __syncthreads();
        if (k0 + GR_BK < n) load_tiles(k0 + GR_BK);
#pragma unroll
        for (int kk = 0; kk < GR_BK / 4; kk++) {
            const double a = As[(kk * 4 + fk) * GR_LDA + wave * 16 + fr];
#pragma unroll
            for (int t = 0; t < 8; t++) {
                const double b = Bs[(kk * 4 + fk) * GR_LDB + t * 16 + fr];
                acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[t], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 8; t++) {
        const int j = j0 + t * 16 + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int i = i0 + wave * 16 + (lane >> 4) + 4 * r;
            if (i < sa && j < sb) {
                if (SYM) {
                    if (i >= j) {
                        Cm[(size_t)i * sb + j] = acc[t][r];
                        Cm[(size_t)j * sb + i] = acc[t][r];
                    }
                } else {
                    Cm[(size_t)i * sb + j] = acc[t][r];
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// small kernels of the iteration
// ------------------------------------------------------------------------------------------------
__device__ inline double unit_hash(unsigned long long x) {  // splitmix64 -> [-1, 1)
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    x ^= x >> 31;
    return (double)(long long)(x >> 11) * 0x1p-52 - 1.0;
}
// the fixed start block Q[ss][b] (col < 0: all columns), or one fresh column for a deficient direction
__global__ void k_pca_fill(double *__restrict__ Q, int ss, int b, int col, unsigned long long salt) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (col < 0) {
        if (e < (long long)ss * b) Q[e] = unit_hash((unsigned long long)e);
    } else if (e < ss) {
        Q[(size_t)e * b + col] = unit_hash(salt * 0x100000000ull + (unsigned long long)e * 4099ull + (unsigned long long)col);
    }
}
// out[c][r] = in[r][c]
__global__ __launch_bounds__(256) void k_pca_transpose(const double *__restrict__ in, double *__restrict__ out, int rows, int cols) {
    __shared__ double tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
    for (int y = ty; y < 32; y += 8)
        if (r0 + y < rows && c0 + tx < cols) tile[y][tx] = in[(size_t)(r0 + y) * cols + c0 + tx];
    __syncthreads();
    for (int y = ty; y < 32; y += 8)
        if (c0 + y < cols && r0 + tx < rows) out[(size_t)(c0 + y) * rows + r0 + tx] = tile[tx][y];
}
// res[i] = || ZW[:, i] - lam[i] V[:, i] ||_2 : a block per column, fixed tree
__global__ __launch_bounds__(256) void k_pca_resid(const double *__restrict__ ZW, const double *__restrict__ V, const double *__restrict__ lam, int ss,
                                                   int b, double *__restrict__ res) {
    __shared__ double red[256];
    const int i = blockIdx.x;
    const double l = lam[i];
    double s = 0.0;
    for (int k = threadIdx.x; k < ss; k += 256) {
        const double d = ZW[(size_t)k * b + i] - l * V[(size_t)k * b + i];
        s += d * d;
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) res[i] = sqrt(red[0]);
}
// component i: sign rule, transpose, singular value.  renorm (the streaming learner): the row is divided by its 2-norm (fixed tree), so
// that |v| = 1 to an ulp instead of to the few eps the last orthonormalisation and V = Q W leave; 0 = the row as it is.
__global__ __launch_bounds__(256) void k_pca_finish(const double *__restrict__ V, const double *__restrict__ lam, int ss, int b, double *__restrict__ Vt,
                                                    double *__restrict__ sv, int renorm) {
    __shared__ double bv[256];
    __shared__ int bi[256];
    const int i = blockIdx.x;
    double best = -1.0;
    int idx = (int)threadIdx.x < ss ? (int)threadIdx.x : 0;  // always a valid row, whatever the values (a NaN compares false)
    for (int k = threadIdx.x; k < ss; k += 256) {
        const double a = fabs(V[(size_t)k * b + i]);
        if (a > best) {  // ascending k inside a thread: the first maximum stays
            best = a;
            idx = k;
        }
    }
    bv[threadIdx.x] = best;
    bi[threadIdx.x] = idx;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            const double ov = bv[threadIdx.x + off];
            const int oi = bi[threadIdx.x + off];
            if (ov > bv[threadIdx.x] || (ov == bv[threadIdx.x] && oi < bi[threadIdx.x])) {
                bv[threadIdx.x] = ov;
                bi[threadIdx.x] = oi;
            }
        }
        __syncthreads();
    }
    const double sgn = V[(size_t)bi[0] * b + i] < 0.0 ? -1.0 : 1.0;
    if (renorm) {
        __syncthreads();  // (bi[0] has been read by every thread)
        double s = 0.0;
        for (int k = threadIdx.x; k < ss; k += 256) {
            const double v = V[(size_t)k * b + i];
            s += v * v;
        }
        bv[threadIdx.x] = s;
        __syncthreads();
        for (int off = 128; off > 0; off >>= 1) {
            if ((int)threadIdx.x < off) bv[threadIdx.x] += bv[threadIdx.x + off];
            __syncthreads();
        }
        const double nrm = sqrt(bv[0]);
        if (nrm > 0.0 && nrm <= 1.79769313486231570815e308) {  // (a zero or non-finite column stays as it is)
            for (int k = threadIdx.x; k < ss; k += 256) Vt[(size_t)i * ss + k] = sgn * V[(size_t)k * b + i] / nrm;
            if (threadIdx.x == 0) sv[i] = sqrt(lam[i] > 0.0 ? lam[i] : 0.0);
            return;
        }
    }
    for (int k = threadIdx.x; k < ss; k += 256) Vt[(size_t)i * ss + k] = sgn * V[(size_t)k * b + i];
    if (threadIdx.x == 0) sv[i] = sqrt(lam[i] > 0.0 ? lam[i] : 0.0);
}

const char *const NONFINITE = "PCA learning: the samples hold non-finite values, or their Gram matrix overflows";

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int launch_gram(bool sym, const double *A, const double *B, const double *muA, const double *muB, double *Cm, long long n, int sa, int sb,
                hipStream_t st) {
    dim3 grid((unsigned)((sb + GR_BN - 1) / GR_BN), (unsigned)((sa + GR_BM - 1) / GR_BM));
    if (sym)
        hipLaunchKernelGGL(k_pca_gram<true>, grid, dim3(GR_NT), 0, st, A, B, muA, muB, Cm, n, sa, sb);
    else
        hipLaunchKernelGGL(k_pca_gram<false>, grid, dim3(GR_NT), 0, st, A, B, muA, muB, Cm, n, sa, sb);
    HIPCK(hipGetLastError());
    return MMIDX_OK;
}

// ------------------------------------------------------------------------------------------------
// the streaming learner's running quantities (mmidx_pca_stream_*): with the shift m0 = the first row,
//   fold      Gt += (X - m0)^T (X - m0) over a staging block (k_pca_gram<true, true>), st[c] += sum_r (X[r][c] - m0[c]) in row order
//   finalise  G = Gt - st st^T / n: the Gram matrix centred by the exact mean; s_i * s_j commutes, so G is exactly symmetric
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_pca_shiftsum(const double *__restrict__ X, long long n, int ss, const double *__restrict__ m0,
                                                     double *__restrict__ sum) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= ss) return;
    double s = sum[c];
    const double m = m0[c];
    const double *x = X + c;
    for (long long r = 0; r < n; r++) s += x[(size_t)r * ss] - m;
    sum[c] = s;
}
__global__ __launch_bounds__(256) void k_pca_finalise(double *__restrict__ G, const double *__restrict__ s, int ss, double n) {
    const int i = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j < ss) G[(size_t)i * ss + j] -= s[i] * s[j] / n;
}

int launch_fold(const double *X, const double *m0, double *G, double *ssum, long long n, int ss, hipStream_t st) {
    dim3 grid((unsigned)((ss + GR_BN - 1) / GR_BN), (unsigned)((ss + GR_BM - 1) / GR_BM));
    hipLaunchKernelGGL((k_pca_gram<true, true>), grid, dim3(GR_NT), 0, st, X, X, m0, m0, G, n, ss, ss);
    hipLaunchKernelGGL(k_pca_shiftsum, dim3((unsigned)((ss + 63) / 64)), dim3(64), 0, st, X, n, ss, m0, ssum);
    HIPCK(hipGetLastError());
    return MMIDX_OK;
}

// The device eigen-solver as the learners and the probe use it: cyclic Jacobi (mmidx_dense_solve.h), then one Newton-Schulz step
// Wt <- Wt (3 I - Wt^T Wt) / 2 on the kernels of this file, which takes the orthonormality of the eigenvectors from the ~100 eps the
// rotations' rounding leaves to the few eps of one b-long product (the components' own orthonormality is held to 16 x LAPACK's).
struct DeviceEig {
    dense_solve::DenseSolver solver;
    DevPtr<double> M, Wraw, zero;
    int cap = 0;
    int sym_eig(const double *dS, int b, double *d_lam, double *d_Wt, hipStream_t st, int *sweeps_out, const char *what, const char *nonfinite) {
        if (b > cap) {
            HIPCK(M.alloc((size_t)b * b));
            HIPCK(Wraw.alloc((size_t)b * b));
            HIPCK(zero.alloc((size_t)b));
            HIPCK(hipMemsetAsync(zero.p, 0, (size_t)b * 8, st));
            cap = b;
        }
        int rc = solver.sym_eig(dS, b, d_lam, Wraw.p, st, sweeps_out, what, nonfinite);
        if (rc) return rc;
        rc = launch_gram(true, Wraw.p, Wraw.p, zero.p, zero.p, M.p, b, b, b, st);
        if (rc) return rc;
        hipLaunchKernelGGL(dense_solve::k_ds_newton, dim3((unsigned)((b + DS_NT - 1) / DS_NT), (unsigned)b), dim3(DS_NT), 0, st, M.p, b);
        HIPCK(hipGetLastError());
        return mmidx_internal_gemm_nt(Wraw.p, zero.p, M.p, d_Wt, b, b, b, st);  // (M is symmetric: Wraw M^T = Wraw M)
    }
};

// what both learners hand to the eigenpair loop: the centred Gram matrix on the device and what the trace line reports of its making
struct EigArgs {
    const double *G;       // [ss][ss], exactly symmetric
    const double *d_zero;  // [ss] zeros (the mean operand of K7 and k_pca_gram)
    int ss, nc;
    long long n;
    double tol;
    int max_iter;
    hipStream_t st;
    const char *who;  // "pca_learn" / "pca_stream"
    bool renorm;      // k_pca_finish divides every component by its norm (the streaming learner)
    float gram_ms;    // the resident learner's k_pca_gram; < 0: not measured here
    double t_begin;
    double *sv_out, *Vt_out;
    int32_t *iters_out;
    double *residual_out;
};
int pca_eigenpairs(const EigArgs &a);

}  // namespace

struct MMIDX_HIDDEN mmidx_pca_learner {
    std::mutex mu;
    int nc = 0, ss = 0, device = 0;
    int64_t num = 0, count = 0;
    Stream stream;  // (before what is used on it: members are destroyed in reverse order)
    DevPtr<double> dA, dsum;
    Event ev_own, ev_ext;  // order the library's stream and a caller's stream (add_device) on the running sums
};

namespace {

// rows [count, count + n) <- src (host or device), then the running sums; `st` = the stream the copy and the sums run on
int add_rows(mmidx_pca_learner *l, int64_t n, const double *src, hipMemcpyKind kind, hipStream_t st) {
    if (n == 0) return MMIDX_OK;
    HIPCK(hipSetDevice(l->device));
    double *dst = l->dA + (size_t)l->count * l->ss;
    if (st != l->stream) HIPCK(hipStreamWaitEvent(st, l->ev_own, 0));
    HIPCK(hipMemcpyAsync(dst, src, (size_t)n * l->ss * 8, kind, st));
    hipLaunchKernelGGL(k_pca_colsum, dim3((unsigned)((l->ss + 63) / 64)), dim3(64), 0, st, dst, (long long)n, l->ss, l->dsum);
    HIPCK(hipGetLastError());
    if (st != l->stream) {
        HIPCK(hipEventRecord(l->ev_ext, st));
        HIPCK(hipStreamWaitEvent(l->stream, l->ev_ext, 0));
    } else {
        HIPCK(hipStreamSynchronize(st));  // host rows: the caller may reuse its buffer
    }
    HIPCK(hipEventRecord(l->ev_own, l->stream));
    l->count += n;
    return MMIDX_OK;
}

}  // namespace

extern "C" {

int mmidx_pca_learn_create(int nc, int64_t num_samples, int ss, int device, mmidx_pca_learner **out) {
    if (!out) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null out pointer");
    *out = nullptr;
    if (nc < 1 || ss < 1 || num_samples < 0) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "bad PCA shape");
    if (nc > ss) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "More components requested than the data's length.");  // PCA.java:102-104
    if (ss > 16384 || nc > 1024 || num_samples > (int64_t)INT32_MAX)
        return mmidx_fail(MMIDX_ERR_UNSUPPORTED, "PCA learning: sampleSize <= 16384, numComponents <= 1024, numSamples < 2^31");
    const int ndev = mmidx_device_count();
    if (ndev < 1) return mmidx_fail(MMIDX_ERR_NO_DEVICE, "no HIP device: libmmidx_hip has no CPU fallback");
    if (device < 0 || device >= ndev) return mmidx_fail(MMIDX_ERR_NO_DEVICE, "device outside the visible range");
    HIPCK(hipSetDevice(device));
    std::unique_ptr<mmidx_pca_learner, int (*)(mmidx_pca_learner *)> l(new mmidx_pca_learner(), mmidx_pca_learn_destroy);  // (destroy: it waits for the stream)
    l->nc = nc;
    l->ss = ss;
    l->num = num_samples;
    l->device = device;
    hipError_t e = l->stream.create();
    if (e == hipSuccess) e = l->ev_own.create(hipEventDisableTiming);
    if (e == hipSuccess) e = l->ev_ext.create(hipEventDisableTiming);
    if (e == hipSuccess) e = l->dA.alloc((size_t)num_samples * ss);  // the samples stay resident (A, :109)
    if (e == hipSuccess) e = l->dsum.alloc((size_t)ss);
    if (e == hipSuccess) e = hipMemsetAsync(l->dsum, 0, (size_t)ss * 8, l->stream);
    if (e == hipSuccess) e = hipEventRecord(l->ev_own, l->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(l->stream);
    if (e != hipSuccess)
        return mmidx_fail(MMIDX_ERR_HIP, "PCA learner: allocation of %lld x %d samples failed: %s", (long long)num_samples, ss, hipGetErrorString(e));
    *out = l.release();
    return MMIDX_OK;
}

int mmidx_pca_learn_destroy(mmidx_pca_learner *l) {
    if (!l) return MMIDX_OK;
    (void)hipSetDevice(l->device);
    if (l->stream) (void)hipStreamSynchronize(l->stream);
    delete l;
    return MMIDX_OK;
}

int mmidx_pca_learn_add(mmidx_pca_learner *l, int64_t n, const double *X) {
    if (!l) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null handle");
    if (n < 0 || (n > 0 && !X)) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null argument");
    std::lock_guard<std::mutex> lk(l->mu);
    if (l->count + n > l->num) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "Too many samples");  // PCA.java:121-122
    return add_rows(l, n, X, hipMemcpyHostToDevice, l->stream);
}

int mmidx_pca_learn_add_device(mmidx_pca_learner *l, int64_t n, const double *dX, void *stream) {
    if (!l) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null handle");
    if (n < 0 || (n > 0 && !dX)) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null argument");
    std::lock_guard<std::mutex> lk(l->mu);
    if (l->count + n > l->num) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "Too many samples");
    return add_rows(l, n, dX, hipMemcpyDeviceToDevice, (hipStream_t)stream);
}

int mmidx_pca_learn_compute(mmidx_pca_learner *l, double tol, int max_iter, double *means_out, double *sv_out, double *Vt_out,
                            int32_t *iters_out, double *residual_out) {
    if (!l) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null handle");
    std::lock_guard<std::mutex> lk(l->mu);
    if (l->count != l->num) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "Not all the data has been added");  // PCA.java:136-137
    if ((int64_t)l->nc > l->num)
        return mmidx_fail(MMIDX_ERR_INVALID_ARG, "More data needed to compute the desired number of components");  // :138-140
    if (!(tol >= 0.0) || max_iter < 1) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "tol must be >= 0 and max_iter >= 1");
    HIPCK(hipSetDevice(l->device));
    hipStream_t st = l->stream;
    const int ss = l->ss, nc = l->nc;
    const long long n = (long long)l->num;
    const double t_begin = now_s();

    // ---- means (PCA.java:150-153) ----
    std::vector<double> h_mu((size_t)ss);
    HIPCK(hipMemcpyAsync(h_mu.data(), l->dsum, (size_t)ss * 8, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    for (int j = 0; j < ss; j++) h_mu[(size_t)j] = h_mu[(size_t)j] / (double)n;
    if (means_out) memcpy(means_out, h_mu.data(), (size_t)ss * 8);

    DevPtr<double> d_mu, d_zero, G;
    HIPCK(d_mu.alloc((size_t)ss));
    HIPCK(d_zero.alloc((size_t)ss));
    HIPCK(G.alloc((size_t)ss * ss));
    HIPCK(hipMemcpyAsync(d_mu.p, h_mu.data(), (size_t)ss * 8, hipMemcpyHostToDevice, st));
    HIPCK(hipMemsetAsync(d_zero.p, 0, (size_t)ss * 8, st));

    // ---- Gram matrix of the centred samples ----
    Event e0, e1;
    HIPCK(e0.create());
    HIPCK(e1.create());
    HIPCK(hipEventRecord(e0, st));
    int rc = launch_gram(true, l->dA, l->dA, d_mu.p, d_mu.p, G.p, n, ss, ss, st);
    if (rc) return rc;
    HIPCK(hipEventRecord(e1, st));
    HIPCK(hipStreamSynchronize(st));
    float gram_ms = 0.f;
    HIPCK(hipEventElapsedTime(&gram_ms, e0, e1));
    const EigArgs ea = {G.p, d_zero.p, ss, nc, n, tol, max_iter, st, "pca_learn", false, gram_ms, t_begin, sv_out, Vt_out, iters_out, residual_out};
    return pca_eigenpairs(ea);
}

}  // extern "C"

namespace {

// which of the two b x b solvers an iteration uses: mmidx_small_solve.h on the host, or mmidx_dense_solve.h on the device.  The
// device serves PCA_DEVICE_SOLVE_ABOVE < b <= PCA_DEVICE_SOLVE_UPTO by default.  Below (never below 256) every shape runs the host
// code it always ran.  The upper end is where the measurements end: the device won at b = 288, and no run of
// the learner with device solves has been measured to converge and win at b = 544 or 1056, so there the default stays the parent's.
// MMIDX_PCA_LEARN_SOLVE=host|device forces either at any b, for both learners.
#ifndef PCA_DEVICE_SOLVE_ABOVE
#define PCA_DEVICE_SOLVE_ABOVE 256
#endif
#ifndef PCA_DEVICE_SOLVE_UPTO
#define PCA_DEVICE_SOLVE_UPTO DS_FUSED_MAX
#endif
static_assert(PCA_DEVICE_SOLVE_ABOVE >= 256, "the host solves stay for b <= 256");

// The top-nc eigenpairs of G by blocked subspace iteration with Rayleigh-Ritz (the header of this file), sv and Vt from them.
int pca_eigenpairs(const EigArgs &a) {
    const int ss = a.ss, nc = a.nc, b = std::min(ss, nc + 32);
    hipStream_t st = a.st;
    const bool trace = getenv("MMIDX_PCA_LEARN_TRACE") != nullptr;
    bool dev = b > PCA_DEVICE_SOLVE_ABOVE && b <= PCA_DEVICE_SOLVE_UPTO;
    if (const char *e = getenv("MMIDX_PCA_LEARN_SOLVE")) {
        if (!strcmp(e, "device")) dev = true;
        else if (!strcmp(e, "host")) dev = false;
        else return mmidx_fail(MMIDX_ERR_INVALID_ARG, "MMIDX_PCA_LEARN_SOLVE must be host or device");
    }
    DeviceEig deig;
    dense_solve::DenseSolver &solver = deig.solver;
    int rc = MMIDX_OK;

    DevPtr<double> Q, Z, V, ZW, Qt, S, Wd, d_lam, d_res, d_Vt, d_sv, d_scale;
    DevPtr<unsigned long long> d_defect;
    const size_t sb = (size_t)ss * b, bb = (size_t)b * b;
    if (dev) {  // (what the device solves alone use; DeviceEig allocates its own blocks at its first solve)
        HIPCK(d_scale.alloc((size_t)b));
        HIPCK(d_defect.alloc(1));
    }
    HIPCK(Q.alloc(sb));
    HIPCK(Z.alloc(sb));
    HIPCK(V.alloc(sb));
    HIPCK(ZW.alloc(sb));
    HIPCK(Qt.alloc(sb));
    HIPCK(S.alloc(bb));
    HIPCK(Wd.alloc(bb));
    HIPCK(d_lam.alloc((size_t)b));
    HIPCK(d_res.alloc((size_t)b));
    HIPCK(d_Vt.alloc((size_t)nc * ss));
    HIPCK(d_sv.alloc((size_t)nc));

    double t_small = 0.0;  // host time in the b x b solves
    std::vector<double> hS(bb), Linv, lam, Wt, h_scale((size_t)b);
    std::vector<int> deficient;
    unsigned long long salt = 1;
    // the device form of one orthonormalisation pass: S = U L U^T, Wd <- rows u_j / sqrt(l_j) (tmp = src Wd^T = src U L^-1/2); a
    // direction with l_j <= b 2^-52 l_max is deficient, as a pivot at that level is for the host's Cholesky factor
    int near_identity = 0;  // passes served by the Newton-Schulz factor
    auto orth_factor_device = [&]() -> int {
        // S within 2^-26 of I (the repeat pass of a block that is orthonormal already): X (3 I - S) / 2 is orthonormal to 3/8 of the
        // defect squared, below eps -- no eigen-solve, and no Jacobi on a spectrum that is one cluster at rounding level
        unsigned long long bits = 0;
        HIPCK(hipMemsetAsync(d_defect.p, 0, 8, st));
        hipLaunchKernelGGL(dense_solve::k_ds_ident_defect, dim3((unsigned)b), dim3(DS_NT), 0, st, S.p, b, d_defect.p);
        HIPCK(hipGetLastError());
        HIPCK(hipMemcpyAsync(&bits, d_defect.p, 8, hipMemcpyDeviceToHost, st));
        HIPCK(hipStreamSynchronize(st));
        double defect;
        memcpy(&defect, &bits, 8);
        if (defect <= 0x1p-26) {
            HIPCK(hipMemcpyAsync(Wd.p, S.p, bb * 8, hipMemcpyDeviceToDevice, st));
            hipLaunchKernelGGL(dense_solve::k_ds_newton, dim3((unsigned)((b + DS_NT - 1) / DS_NT), (unsigned)b), dim3(DS_NT), 0, st, Wd.p, b);
            HIPCK(hipGetLastError());
            deficient.clear();
            near_identity++;
            return MMIDX_OK;
        }
        int r = deig.sym_eig(S.p, b, d_lam.p, Wd.p, st, nullptr, "PCA learning, orthonormalisation", NONFINITE);
        if (r) return r;
        lam.resize((size_t)b);
        HIPCK(hipMemcpyAsync(lam.data(), d_lam.p, (size_t)b * 8, hipMemcpyDeviceToHost, st));
        HIPCK(hipStreamSynchronize(st));
        const double thr = (double)b * 0x1p-52 * lam[0];
        deficient.clear();
        for (int j = 0; j < b; j++) {
            const bool ok = lam[(size_t)j] > thr;
            if (!ok) deficient.push_back(j);
            h_scale[(size_t)j] = ok ? 1.0 / std::sqrt(lam[(size_t)j]) : 0.0;
        }
        HIPCK(hipMemcpyAsync(d_scale.p, h_scale.data(), (size_t)b * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(dense_solve::k_ds_scale_rows, dim3((unsigned)((b + DS_NT - 1) / DS_NT), (unsigned)b), dim3(DS_NT), 0, st, Wd.p, d_scale.p, b);
        HIPCK(hipGetLastError());
        return MMIDX_OK;
    };
    // CholeskyQR until two passes in a row met no deficient direction (normally the first two): *src <- orthonormal basis of span(*src)
    auto orth = [&](double *&src, double *&tmp) -> int {
        for (int pass = 0, clean = 0; pass < 6; pass++) {
            int r = launch_gram(true, src, src, a.d_zero, a.d_zero, S.p, ss, b, b, st);
            if (r) return r;
            if (dev) {
                r = orth_factor_device();
                if (r) return r;
            } else {
                HIPCK(hipMemcpyAsync(hS.data(), S.p, bb * 8, hipMemcpyDeviceToHost, st));
                HIPCK(hipStreamSynchronize(st));
                const double t0 = now_s();
                if (!mmidx_small::chol_inverse(hS.data(), b, (double)b * 0x1p-52, Linv, deficient))
                    return mmidx_fail(MMIDX_ERR_INVALID_ARG, "%s", NONFINITE);
                t_small += now_s() - t0;
                HIPCK(hipMemcpyAsync(Wd.p, Linv.data(), bb * 8, hipMemcpyHostToDevice, st));
            }
            r = mmidx_internal_gemm_nt(src, a.d_zero, Wd.p, tmp, ss, b, b, st);  // tmp = src L^-T (device solves: src U L^-1/2)
            if (r) return r;
            for (int j : deficient)
                hipLaunchKernelGGL(k_pca_fill, dim3((unsigned)((ss + 255) / 256)), dim3(256), 0, st, tmp, ss, b, j, salt++);
            HIPCK(hipGetLastError());
            HIPCK(hipStreamSynchronize(st));  // (Linv is rewritten by the next pass)
            std::swap(src, tmp);
            clean = deficient.empty() ? clean + 1 : 0;
            if (clean >= 2) return MMIDX_OK;
        }
        return mmidx_fail(MMIDX_ERR_UNSUPPORTED, "PCA learning: the block could not be orthonormalised in 6 CholeskyQR passes");
    };

    double *q = Q.p, *z = Z.p, *zw = ZW.p;
    hipLaunchKernelGGL(k_pca_fill, dim3((unsigned)((sb + 255) / 256)), dim3(256), 0, st, q, ss, b, -1, 0ull);
    HIPCK(hipGetLastError());
    rc = orth(q, z);
    if (rc) return rc;

    const double t_iter0 = now_s();
    int iters = 0;
    double residual = 0.0;
    bool converged = false;
    std::vector<double> h_res((size_t)b);
    for (;;) {
        iters++;
        hipLaunchKernelGGL(k_pca_transpose, dim3((unsigned)((b + 31) / 32), (unsigned)((ss + 31) / 32)), dim3(256), 0, st, q, Qt.p, ss, b);
        HIPCK(hipGetLastError());
        rc = mmidx_internal_gemm_nt(a.G, a.d_zero, Qt.p, z, ss, b, ss, st);  // Z = G Q
        if (rc) return rc;
        rc = launch_gram(false, q, z, a.d_zero, a.d_zero, S.p, ss, b, b, st);  // T = Q^T Z
        if (rc) return rc;
        if (dev) {
            rc = deig.sym_eig(S.p, b, d_lam.p, Wd.p, st, nullptr, "PCA learning, Rayleigh-Ritz", NONFINITE);
            if (rc) return rc;
            lam.resize((size_t)b);
            HIPCK(hipMemcpyAsync(lam.data(), d_lam.p, (size_t)b * 8, hipMemcpyDeviceToHost, st));
            HIPCK(hipStreamSynchronize(st));
        } else {
            HIPCK(hipMemcpyAsync(hS.data(), S.p, bb * 8, hipMemcpyDeviceToHost, st));
            HIPCK(hipStreamSynchronize(st));
            const double t0 = now_s();
            for (int i = 0; i < b; i++)
                for (int j = 0; j < i; j++) {
                    const double m = 0.5 * (hS[(size_t)i * b + j] + hS[(size_t)j * b + i]);
                    hS[(size_t)i * b + j] = m;
                    hS[(size_t)j * b + i] = m;
                }
            if (!mmidx_small::sym_eig(hS.data(), b, lam, Wt)) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "%s", NONFINITE);
            t_small += now_s() - t0;
            HIPCK(hipMemcpyAsync(Wd.p, Wt.data(), bb * 8, hipMemcpyHostToDevice, st));
            HIPCK(hipMemcpyAsync(d_lam.p, lam.data(), (size_t)b * 8, hipMemcpyHostToDevice, st));
        }
        rc = mmidx_internal_gemm_nt(q, a.d_zero, Wd.p, V.p, ss, b, b, st);  // V = Q W (Ritz vectors)
        if (rc) return rc;
        rc = mmidx_internal_gemm_nt(z, a.d_zero, Wd.p, zw, ss, b, b, st);  // Z W = G V
        if (rc) return rc;
        hipLaunchKernelGGL(k_pca_resid, dim3((unsigned)nc), dim3(256), 0, st, zw, V.p, d_lam.p, ss, b, d_res.p);
        HIPCK(hipGetLastError());
        HIPCK(hipMemcpyAsync(h_res.data(), d_res.p, (size_t)nc * 8, hipMemcpyDeviceToHost, st));
        HIPCK(hipStreamSynchronize(st));
        double mr = 0.0;
        for (int i = 0; i < nc; i++) mr = std::max(mr, h_res[(size_t)i]);
        residual = lam[0] > 0.0 ? mr / lam[0] : (mr == 0.0 ? 0.0 : HUGE_VAL);
        if (!(mr == mr)) residual = HUGE_VAL;  // NaN
        if (trace) fprintf(stderr, "[mmidx] %s: iteration %d residual %.3e\n", a.who, iters, residual);
        if (residual <= a.tol) {
            converged = true;
            break;
        }
        if (iters >= a.max_iter) break;
        std::swap(q, zw);  // next block: an orthonormal basis of span(Z W)
        rc = orth(q, z);
        if (rc) return rc;
    }
    const double t_iter1 = now_s();

    // ---- singular values, sign rule, transpose ----
    hipLaunchKernelGGL(k_pca_finish, dim3((unsigned)nc), dim3(256), 0, st, V.p, d_lam.p, ss, b, d_Vt.p, d_sv.p, a.renorm ? 1 : 0);
    HIPCK(hipGetLastError());
    if (a.Vt_out) HIPCK(hipMemcpyAsync(a.Vt_out, d_Vt.p, (size_t)nc * ss * 8, hipMemcpyDeviceToHost, st));
    if (a.sv_out) HIPCK(hipMemcpyAsync(a.sv_out, d_sv.p, (size_t)nc * 8, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    if (a.iters_out) *a.iters_out = iters;
    if (a.residual_out) *a.residual_out = residual;
    if (trace) {
        long long tiles = 0;  // tiles k_pca_gram ran (lower triangle + the diagonal's): the TF/s figure counts what was executed
        for (int i0 = 0; i0 < ss; i0 += GR_BM)
            for (int j0 = 0; j0 < ss; j0 += GR_BN) tiles += i0 + GR_BM - 1 >= j0;
        char gram[96] = "";
        if (a.gram_ms >= 0.f)
            snprintf(gram, sizeof gram, " gram %.3f ms (%.2f TF/s executed),", a.gram_ms, 2.0 * (double)a.n * (double)tiles * GR_BM * GR_BN / (a.gram_ms * 1e-3) * 1e-12);
        fprintf(stderr, "[mmidx] %s: n %lld ss %d nc %d b %d:%s %d iterations %.3f s, solver %s, host solves %.3f s (start block included), device solves %d in %.3f s, %.2f sweeps per solve, %d near-identity passes, total %.3f s\n",
                a.who, a.n, ss, nc, b, gram, iters, t_iter1 - t_iter0, dev ? "device" : "host", t_small, solver.solves, solver.seconds,
                solver.solves ? (double)solver.sweeps_total / solver.solves : 0.0, near_identity, now_s() - a.t_begin);
    }
    if (!converged)
        return mmidx_fail(MMIDX_ERR_NOT_CONVERGED, "PCA basis not converged: residual %.3e > a.tol %.3e after %d iterations", residual, a.tol, iters);
    return MMIDX_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// the streaming learner: rows are folded into the Gram matrix as they arrive and are not kept
// ------------------------------------------------------------------------------------------------
struct MMIDX_HIDDEN mmidx_pca_stream {
    std::mutex mu;
    int nc = 0, ss = 0, device = 0;
    int R = 0;             // rows of the staging block: a fold runs whenever it is full, whatever the add calls were
    int fill = 0;          // rows waiting in it
    int64_t count = 0;
    bool finalised = false;  // compute has turned Gt into the centred G: no row can be folded any more
    bool broken = false;     // a device call failed in the middle of an add or of the finalisation: the running sums are not to be trusted
    Stream stream;
    DevPtr<double> dG, dstage, dsum, dm0, dssum, dzero;
    Event ev_own, ev_ext;
};

namespace {

int stream_add_rows(mmidx_pca_stream *s, int64_t n, const double *src, hipMemcpyKind kind, hipStream_t st) {
    if (n == 0) return MMIDX_OK;
    HIPCK(hipSetDevice(s->device));
    const int ss = s->ss;
    if (st != s->stream) HIPCK(hipStreamWaitEvent(st, s->ev_own, 0));
    while (n > 0) {
        const int64_t chunk = std::min<int64_t>(n, (int64_t)(s->R - s->fill));
        double *dst = s->dstage + (size_t)s->fill * ss;
        HIPCK(hipMemcpyAsync(dst, src, (size_t)chunk * ss * 8, kind, st));
        if (s->count == 0) HIPCK(hipMemcpyAsync(s->dm0.p, dst, (size_t)ss * 8, hipMemcpyDeviceToDevice, st));  // the shift: the first row
        hipLaunchKernelGGL(k_pca_colsum, dim3((unsigned)((ss + 63) / 64)), dim3(64), 0, st, dst, (long long)chunk, ss, s->dsum);
        HIPCK(hipGetLastError());
        s->fill += (int)chunk;
        s->count += chunk;
        src += (size_t)chunk * ss;
        n -= chunk;
        if (s->fill == s->R) {
            int rc = launch_fold(s->dstage, s->dm0, s->dG, s->dssum, s->R, ss, st);
            if (rc) return rc;
            s->fill = 0;
        }
    }
    if (st != s->stream) {
        HIPCK(hipEventRecord(s->ev_ext, st));
        HIPCK(hipStreamWaitEvent(s->stream, s->ev_ext, 0));
    } else {
        HIPCK(hipStreamSynchronize(st));  // host rows: the caller may reuse its buffer
    }
    HIPCK(hipEventRecord(s->ev_own, s->stream));
    return MMIDX_OK;
}

const char *const STREAM_BROKEN = "PCA stream: an earlier device call on this handle failed part-way; destroy it";

// the state checks of both add forms, then the rows on `st` (already resolved: the handle's own stream for host rows)
int stream_add_checked(mmidx_pca_stream *s, int64_t n, const double *X, hipMemcpyKind kind, hipStream_t st) {
    if (s->broken) return mmidx_fail(MMIDX_ERR_HIP, "%s", STREAM_BROKEN);
    if (s->finalised) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "PCA stream: the basis has been computed and the Gram matrix finalised: no more samples");
    if (s->count + n > (int64_t)INT32_MAX) return mmidx_fail(MMIDX_ERR_UNSUPPORTED, "PCA stream: fewer than 2^31 samples in all");
    const int rc = stream_add_rows(s, n, X, kind, st);
    if (rc) s->broken = true;  // (fill and count may have advanced past rows that never arrived)
    return rc;
}

}  // namespace

extern "C" {

int mmidx_pca_stream_create(int nc, int ss, int device, mmidx_pca_stream **out) {
    if (!out) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null out pointer");
    *out = nullptr;
    if (nc < 1 || ss < 1) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "bad PCA shape");
    if (nc > ss) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "More components requested than the data's length.");  // PCA.java:102-104
    if (ss > 32768 || nc > 1024) return mmidx_fail(MMIDX_ERR_UNSUPPORTED, "PCA stream: sampleSize <= 32768, numComponents <= 1024");
    int R = std::min(4096, std::max(64, ((1 << 25) / ss) & ~63));
    if (const char *e = getenv("MMIDX_PCA_STREAM_ROWS")) {  // tests: a staging block of their choice
        char *end = nullptr;
        const long v = strtol(e, &end, 10);
        if (end == e || *end || v < 8 || v % 8 || v > 65536)
            return mmidx_fail(MMIDX_ERR_INVALID_ARG, "MMIDX_PCA_STREAM_ROWS must be a multiple of 8 in 8 .. 65536");
        R = (int)v;
    }
    const int ndev = mmidx_device_count();
    if (ndev < 1) return mmidx_fail(MMIDX_ERR_NO_DEVICE, "no HIP device: libmmidx_hip has no CPU fallback");
    if (device < 0 || device >= ndev) return mmidx_fail(MMIDX_ERR_NO_DEVICE, "device outside the visible range");
    HIPCK(hipSetDevice(device));
    std::unique_ptr<mmidx_pca_stream, int (*)(mmidx_pca_stream *)> s(new mmidx_pca_stream(), mmidx_pca_stream_destroy);
    s->nc = nc;
    s->ss = ss;
    s->R = R;
    s->device = device;
    hipError_t e = s->stream.create();
    if (e == hipSuccess) e = s->ev_own.create(hipEventDisableTiming);
    if (e == hipSuccess) e = s->ev_ext.create(hipEventDisableTiming);
    if (e == hipSuccess) e = s->dG.alloc((size_t)ss * ss);
    if (e == hipSuccess) e = s->dstage.alloc((size_t)R * ss);
    if (e == hipSuccess) e = s->dsum.alloc((size_t)ss);
    if (e == hipSuccess) e = s->dm0.alloc((size_t)ss);
    if (e == hipSuccess) e = s->dssum.alloc((size_t)ss);
    if (e == hipSuccess) e = s->dzero.alloc((size_t)ss);
    if (e == hipSuccess) e = hipMemsetAsync(s->dG, 0, (size_t)ss * ss * 8, s->stream);
    if (e == hipSuccess) e = hipMemsetAsync(s->dsum, 0, (size_t)ss * 8, s->stream);
    if (e == hipSuccess) e = hipMemsetAsync(s->dm0, 0, (size_t)ss * 8, s->stream);
    if (e == hipSuccess) e = hipMemsetAsync(s->dssum, 0, (size_t)ss * 8, s->stream);
    if (e == hipSuccess) e = hipMemsetAsync(s->dzero, 0, (size_t)ss * 8, s->stream);
    if (e == hipSuccess) e = hipEventRecord(s->ev_own, s->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    if (e != hipSuccess)
        return mmidx_fail(MMIDX_ERR_HIP, "PCA stream: allocation of the %d x %d Gram matrix and %d staging rows failed: %s", ss, ss, R, hipGetErrorString(e));
    *out = s.release();
    return MMIDX_OK;
}

int mmidx_pca_stream_destroy(mmidx_pca_stream *s) {
    if (!s) return MMIDX_OK;
    (void)hipSetDevice(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);  // (work of an add_device on another stream is ordered before it)
    delete s;
    return MMIDX_OK;
}

int mmidx_pca_stream_add(mmidx_pca_stream *s, int64_t n, const double *X) {
    if (!s) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null handle");
    if (n < 0 || (n > 0 && !X)) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null argument");
    std::lock_guard<std::mutex> lk(s->mu);
    return stream_add_checked(s, n, X, hipMemcpyHostToDevice, s->stream);
}

int mmidx_pca_stream_add_device(mmidx_pca_stream *s, int64_t n, const double *dX, void *stream) {
    if (!s) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null handle");
    if (n < 0 || (n > 0 && !dX)) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null argument");
    std::lock_guard<std::mutex> lk(s->mu);
    // (as mmidx_pca_learn_add_device: a null stream is the device's default stream, not the handle's)
    return stream_add_checked(s, n, dX, hipMemcpyDeviceToDevice, (hipStream_t)stream);
}

int mmidx_pca_stream_count(const mmidx_pca_stream *s, int64_t *n_out) {
    if (!s || !n_out) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null argument");
    std::lock_guard<std::mutex> lk(const_cast<mmidx_pca_stream *>(s)->mu);
    *n_out = s->count;
    return MMIDX_OK;
}

int mmidx_pca_stream_compute(mmidx_pca_stream *s, double tol, int max_iter, double *means_out, double *sv_out, double *Vt_out,
                             int32_t *iters_out, double *residual_out) {
    if (!s) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null handle");
    std::lock_guard<std::mutex> lk(s->mu);
    if (s->broken) return mmidx_fail(MMIDX_ERR_HIP, "%s", STREAM_BROKEN);
    if ((int64_t)s->nc > s->count)
        return mmidx_fail(MMIDX_ERR_INVALID_ARG, "More data needed to compute the desired number of components");  // PCA.java:138-140
    if (!(tol >= 0.0) || max_iter < 1) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "tol must be >= 0 and max_iter >= 1");
    HIPCK(hipSetDevice(s->device));
    hipStream_t st = s->stream;
    const int ss = s->ss;
    const double t_begin = now_s();
    if (!s->finalised) {
        // the tail's fold and the finalisation change Gt in place: the handle counts as finalised only once the stream has run them,
        // and a device failure on the way leaves it unusable
        auto finalise = [&]() -> int {
            if (s->fill > 0) {
                int rc = launch_fold(s->dstage, s->dm0, s->dG, s->dssum, s->fill, ss, st);
                if (rc) return rc;
            }
            hipLaunchKernelGGL(k_pca_finalise, dim3((unsigned)((ss + 255) / 256), (unsigned)ss), dim3(256), 0, st, s->dG.p, s->dssum.p, ss, (double)s->count);
            HIPCK(hipGetLastError());
            HIPCK(hipStreamSynchronize(st));
            return MMIDX_OK;
        };
        const int rc = finalise();
        if (rc) {
            s->broken = true;
            return rc;
        }
        s->fill = 0;
        s->finalised = true;
    }
    // ---- means (PCA.java:150-153) ----
    std::vector<double> h_mu((size_t)ss);
    HIPCK(hipMemcpyAsync(h_mu.data(), s->dsum, (size_t)ss * 8, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    for (int j = 0; j < ss; j++) h_mu[(size_t)j] = h_mu[(size_t)j] / (double)s->count;
    if (means_out) memcpy(means_out, h_mu.data(), (size_t)ss * 8);
    const EigArgs ea = {s->dG.p, s->dzero.p, ss, s->nc, (long long)s->count, tol, max_iter, st, "pca_stream", true, -1.f, t_begin, sv_out, Vt_out, iters_out, residual_out};
    return pca_eigenpairs(ea);
}

int mmidx_probe_sym_eig(int device, int b, const double *T, double *lam_out, double *Wt_out, int32_t *sweeps_out) {
    if (!T) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null argument");
    if (b < 1 || b > 1056) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "mmidx_probe_sym_eig: 1 <= b <= 1056");
    const int ndev = mmidx_device_count();
    if (ndev < 1) return mmidx_fail(MMIDX_ERR_NO_DEVICE, "no HIP device: libmmidx_hip has no CPU fallback");
    if (device < 0 || device >= ndev) return mmidx_fail(MMIDX_ERR_NO_DEVICE, "device outside the visible range");
    HIPCK(hipSetDevice(device));
    const size_t bb = (size_t)b * b;
    Stream st;
    DevPtr<double> dS, d_lam, d_Wt;
    DeviceEig deig;
    HIPCK(st.create());
    HIPCK(dS.alloc(bb));
    HIPCK(d_lam.alloc((size_t)b));
    HIPCK(d_Wt.alloc(bb));
    HIPCK(hipMemcpyAsync(dS.p, T, bb * 8, hipMemcpyHostToDevice, st));
    int sweeps = 0;
    int rc = deig.sym_eig(dS.p, b, d_lam.p, d_Wt.p, st, &sweeps, "mmidx_probe_sym_eig", "mmidx_probe_sym_eig: the matrix holds a non-finite entry");
    if (rc) {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    if (lam_out) HIPCK(hipMemcpyAsync(lam_out, d_lam.p, (size_t)b * 8, hipMemcpyDeviceToHost, st));
    if (Wt_out) HIPCK(hipMemcpyAsync(Wt_out, d_Wt.p, bb * 8, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    if (sweeps_out) *sweeps_out = sweeps;
    return MMIDX_OK;
}

}  // extern "C"
