// mmidx_dense_solve.h -- the dense b x b solves of the PCA learners' subspace iteration on the device (b = numComponents + 32 <= 1056).
// A kernel header: included by mmidx_pca_learn.hip alone.
//
//   DenseSolver::sym_eig   all eigenpairs of a symmetric matrix by cyclic Jacobi in fp64, two-sided, under the round-robin ordering
//                          of mmidx_jacobi.h: a sweep is n - 1 steps, a step rotates n / 2 disjoint pairs at once, T <- J^T T J and
//                          Wt <- J^T Wt.  Eigenvalues descending, eigenvectors as the ROWS of Wt: what mmidx_small::sym_eig returns.
//   The orthonormalisation of a tall block reuses it (S = X^T X = U L U^T, X <- X U L^-1/2): see orth in mmidx_pca_learn.hip.
//
// One launch per step (b <= DS_FUSED_MAX: every thread works out the rotations it needs itself) or two (k_ds_rot writes the step's
// rotations, k_ds_step applies them).  Nothing waits inside a kernel for another workgroup: the order between steps is the stream's.
// A step reads one copy of T and Wt and writes the other, so no element is read after it was overwritten.
//   k_ds_step, T part: thread (I, J) owns the 2 x 2 block rows {p, q} of pair I x columns {P, Q} of pair J and writes rows p and q
//     only (coalesced).  Block (J, I) is its transpose; both threads apply the two rotations in the same order -- first the one of
//     the larger pair index -- to bitwise-equal inputs, so T stays EXACTLY symmetric without mirrored (strided) stores.
//     On the pair's own block the new diagonal is a_pp - t a_pq, a_qq + t a_pq and the off-diagonal is set to 0.
//   k_ds_off: max |t_ij|, i != j, over the entries themselves, by atomicMax on the bit pattern of a non-negative double (ordered as
//     the values are, so the result does not depend on scheduling); read back once per sweep.  The same kernel reports max |t_ij|
//     over all entries and whether any entry is non-finite: the first call is the non-finite check, before any rotation.
//   Stop: off <= sqrt(b) eps max|t_ij| of the input (max|t_ij| <= ||T||_2, so this is below b eps ||T||), or off <= b eps max|t_ij|
//     after a sweep that no longer halved it (the rounding floor of a clustered spectrum, below); 30 sweeps without either is
//     MMIDX_ERR_NOT_CONVERGED.  The level cannot be a plain eps ||T||: the diagonal is stored to eps ||T||, a rotation
//     rounds two of its entries, and a cluster of eigenvalues tighter than that (S = X^T X of a nearly orthonormal block: every
//     eigenvalue within 1e-13 of 1) keeps regenerating off-diagonal entries of a few eps -- measured 3.2 eps at b = 320, for 30 sweeps.
//     The residual of an eigenvector is then at most sqrt(b) off <= b eps ||T||, a thirtieth of the 30 b eps the tests hold it to.
//   The rounding of about sweeps x b rotations per row leaves Wt orthonormal to about 100 eps at b = 160; the caller polishes it with
//     one Newton-Schulz step (DeviceEig in mmidx_pca_learn.hip, on the product kernels that file already has).
// Cost: about n launches per sweep (2n above DS_FUSED_MAX) and 7-10 sweeps from a dense start; the launch overhead is the floor.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstring>

#include "mmidx_host.h"
#include "mmidx_jacobi.h"

#define DS_NT 256
#define DS_FUSED_MAX 512   // up to this b a step is one launch
#define DS_MAX_SWEEPS 30

namespace dense_solve {

namespace J = mmidx_jacobi;

// flags[0] = bits of max |t_ij| i != j, flags[1] = bits of max |t_ij|, flags[2] = 1 iff an entry is non-finite
__global__ __launch_bounds__(DS_NT) void k_ds_off(const double *__restrict__ T, int b, unsigned long long *__restrict__ flags) {
    __shared__ double r_off[DS_NT], r_all[DS_NT];
    __shared__ int r_bad[DS_NT];
    const int i = blockIdx.x;
    double off = 0.0, all = 0.0;
    int bad = 0;
    for (int j = threadIdx.x; j < b; j += DS_NT) {
        const double v = fabs(T[(size_t)i * b + j]);
        if (!(v <= 1.79769313486231570815e308)) bad = 1;  // NaN or Inf
        else {
            all = v > all ? v : all;
            if (j != i) off = v > off ? v : off;
        }
    }
    r_off[threadIdx.x] = off;
    r_all[threadIdx.x] = all;
    r_bad[threadIdx.x] = bad;
    __syncthreads();
    for (int o = DS_NT / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            r_off[threadIdx.x] = fmax(r_off[threadIdx.x], r_off[threadIdx.x + o]);
            r_all[threadIdx.x] = fmax(r_all[threadIdx.x], r_all[threadIdx.x + o]);
            r_bad[threadIdx.x] |= r_bad[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        atomicMax(flags + 0, (unsigned long long)__double_as_longlong(r_off[0]));
        atomicMax(flags + 1, (unsigned long long)__double_as_longlong(r_all[0]));
        if (r_bad[0]) atomicMax(flags + 2, 1ull);
    }
}

// T[i][j] = (S[i][j] + S[j][i]) / 2 (what the host path does before mmidx_small::sym_eig), Wt = I
__global__ __launch_bounds__(DS_NT) void k_ds_prepare(const double *__restrict__ S, int b, double *__restrict__ T, double *__restrict__ Wt) {
    const int i = blockIdx.y, j = blockIdx.x * DS_NT + threadIdx.x;
    if (j >= b) return;
    const double a = S[(size_t)i * b + j], c = S[(size_t)j * b + i];
    T[(size_t)i * b + j] = i == j ? a : (i > j ? 0.5 * (a + c) : 0.5 * (c + a));  // (both triangles add in the same order)
    Wt[(size_t)i * b + j] = i == j ? 1.0 : 0.0;
}

__device__ inline J::Rot pair_rot(const double *__restrict__ T, int b, int p, int q) {
    if (q >= b) return J::rotation(0.0, 0.0, 0.0);  // the idle slot of an odd b
    return J::rotation(T[(size_t)p * b + p], T[(size_t)q * b + q], T[(size_t)p * b + q]);
}

// the rotations of step s: rot[k] = (c, s, t) of pair k
__global__ __launch_bounds__(DS_NT) void k_ds_rot(const double *__restrict__ T, int b, int n, int s, double *__restrict__ rot) {
    const int k = blockIdx.x * DS_NT + threadIdx.x;
    if (k >= n / 2) return;
    int p, q;
    J::pair_of(n, s, k, &p, &q);
    const J::Rot r = pair_rot(T, b, p, q);
    rot[3 * k + 0] = r.c;
    rot[3 * k + 1] = r.s;
    rot[3 * k + 2] = r.t;
}

__device__ inline J::Rot get_rot(const double *__restrict__ T, const double *__restrict__ rot, int b, int k, int p, int q) {
    if (!rot) return pair_rot(T, b, p, q);
    J::Rot r;
    r.c = rot[3 * k + 0];
    r.s = rot[3 * k + 1];
    r.t = rot[3 * k + 2];
    return r;
}

// one step.  grid (ceil(b / DS_NT), n / 2, 2): blockIdx.y = pair I; z = 0 the T part (thread <-> pair J), z = 1 the Wt part
// (thread <-> column).  rot == nullptr: the rotations are worked out here from Tin.
__global__ __launch_bounds__(DS_NT) void k_ds_step(const double *__restrict__ Tin, double *__restrict__ Tout, const double *__restrict__ Win,
                                                   double *__restrict__ Wout, const double *__restrict__ rot, int b, int n, int s) {
    const int I = blockIdx.y, x = blockIdx.x * DS_NT + threadIdx.x;
    int p, q;
    J::pair_of(n, s, I, &p, &q);
    const bool hq = q < b;  // (p < q, so p < b always: n - 1 is the only slot that may be idle)
    const J::Rot rI = get_rot(Tin, rot, b, I, p, q);
    if (blockIdx.z == 1) {
        if (x >= b) return;
        double wp = Win[(size_t)p * b + x], wq = hq ? Win[(size_t)q * b + x] : 0.0;
        J::rotate(rI, &wp, &wq);
        Wout[(size_t)p * b + x] = wp;
        if (hq) Wout[(size_t)q * b + x] = wq;
        return;
    }
    if (x >= n / 2) return;
    int P, Q;
    J::pair_of(n, s, x, &P, &Q);
    const bool hQ = Q < b;
    if (x == I) {
        const double app = Tin[(size_t)p * b + p];
        if (!hq) {
            Tout[(size_t)p * b + p] = app;
            return;
        }
        const double aqq = Tin[(size_t)q * b + q], apq = Tin[(size_t)p * b + q];
        Tout[(size_t)p * b + p] = app - rI.t * apq;
        Tout[(size_t)q * b + q] = aqq + rI.t * apq;
        Tout[(size_t)p * b + q] = 0.0;
        Tout[(size_t)q * b + p] = 0.0;
        return;
    }
    const J::Rot rJ = get_rot(Tin, rot, b, x, P, Q);
    double apP = Tin[(size_t)p * b + P], apQ = hQ ? Tin[(size_t)p * b + Q] : 0.0;
    double aqP = hq ? Tin[(size_t)q * b + P] : 0.0, aqQ = hq && hQ ? Tin[(size_t)q * b + Q] : 0.0;
    if (I > x) {  // the rotation of the larger pair index first, in this block and in its transpose
        J::rotate(rI, &apP, &aqP);
        J::rotate(rI, &apQ, &aqQ);
        J::rotate(rJ, &apP, &apQ);
        J::rotate(rJ, &aqP, &aqQ);
    } else {
        J::rotate(rJ, &apP, &apQ);
        J::rotate(rJ, &aqP, &aqQ);
        J::rotate(rI, &apP, &aqP);
        J::rotate(rI, &apQ, &aqQ);
    }
    Tout[(size_t)p * b + P] = apP;
    if (hQ) Tout[(size_t)p * b + Q] = apQ;
    if (hq) Tout[(size_t)q * b + P] = aqP;
    if (hq && hQ) Tout[(size_t)q * b + Q] = aqQ;
}

// descending order, equal values in index order: row i of Wt goes to row rank(i) of out, lam[rank(i)] = T[i][i]
__global__ __launch_bounds__(DS_NT) void k_ds_sort(const double *__restrict__ T, const double *__restrict__ Wt, int b, double *__restrict__ lam,
                                                   double *__restrict__ out) {
    __shared__ int cnt[DS_NT];
    const int i = blockIdx.x;
    const double di = T[(size_t)i * b + i];
    int c = 0;
    for (int j = threadIdx.x; j < b; j += DS_NT) {
        const double dj = T[(size_t)j * b + j];
        c += (dj > di || (dj == di && j < i)) ? 1 : 0;
    }
    cnt[threadIdx.x] = c;
    __syncthreads();
    for (int o = DS_NT / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) cnt[threadIdx.x] += cnt[threadIdx.x + o];
        __syncthreads();
    }
    const int r = cnt[0];
    if (threadIdx.x == 0) lam[r] = di;
    for (int j = threadIdx.x; j < b; j += DS_NT) out[(size_t)r * b + j] = Wt[(size_t)i * b + j];
}

// M <- 1.5 I - 0.5 M (M = Wt^T Wt): the factor of one Newton-Schulz step Wt <- Wt M towards the nearest orthogonal matrix
__global__ __launch_bounds__(DS_NT) void k_ds_newton(double *__restrict__ M, int b) {
    const int i = blockIdx.y, j = blockIdx.x * DS_NT + threadIdx.x;
    if (j < b) M[(size_t)i * b + j] = (i == j ? 1.5 : 0.0) - 0.5 * M[(size_t)i * b + j];
}

// out[0] = bits of max |S_ij - delta_ij| (+inf for a non-finite entry): how far a Gram matrix is from the identity
__global__ __launch_bounds__(DS_NT) void k_ds_ident_defect(const double *__restrict__ S, int b, unsigned long long *__restrict__ out) {
    __shared__ double red[DS_NT];
    const int i = blockIdx.x;
    double m = 0.0;
    for (int j = threadIdx.x; j < b; j += DS_NT) {
        const double v = fabs(S[(size_t)i * b + j] - (i == j ? 1.0 : 0.0));
        m = !(v <= 1.79769313486231570815e308) ? __longlong_as_double(0x7ff0000000000000ll) : (v > m ? v : m);
    }
    red[threadIdx.x] = m;
    __syncthreads();
    for (int o = DS_NT / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicMax(out, (unsigned long long)__double_as_longlong(red[0]));
}

// row j of Wt times scale[j] (in place): the factor U L^-1/2 of the orthonormalisation, as the B operand of K7
__global__ __launch_bounds__(DS_NT) void k_ds_scale_rows(double *__restrict__ Wt, const double *__restrict__ scale, int b) {
    const int i = blockIdx.y, j = blockIdx.x * DS_NT + threadIdx.x;
    if (j < b) Wt[(size_t)i * b + j] *= scale[i];
}

struct DenseSolver {
    DevPtr<double> T0, T1, W0, W1, rot;
    DevPtr<unsigned long long> flags;
    int cap = 0;
    int sweeps_total = 0, solves = 0;  // since the caller last cleared them
    double seconds = 0.0;              // wall time inside sym_eig, its waits included

    int ensure(int b) {
        if (b <= cap) return MMIDX_OK;
        const size_t bb = (size_t)b * b;
        HIPCK(T0.alloc(bb));
        HIPCK(T1.alloc(bb));
        HIPCK(W0.alloc(bb));
        HIPCK(W1.alloc(bb));
        HIPCK(rot.alloc((size_t)3 * (size_t)(J::slots(b) / 2)));
        HIPCK(flags.alloc(3));
        cap = b;
        return MMIDX_OK;
    }

    // dS[b][b] on the device (symmetrised here) -> d_lam[b] descending, d_Wt[b][b] eigenvectors as rows, *sweeps_out.
    // `what` names the solve in the message of MMIDX_ERR_NOT_CONVERGED; a non-finite entry: MMIDX_ERR_INVALID_ARG with `nonfinite`,
    // nothing written.
    int sym_eig(const double *dS, int b, double *d_lam, double *d_Wt, hipStream_t st, int *sweeps_out, const char *what, const char *nonfinite) {
        const auto t0 = std::chrono::steady_clock::now();
        int rc = ensure(b);
        if (rc) return rc;
        const int n = J::slots(b);
        double *Ti = T0.p, *To = T1.p, *Wi = W0.p, *Wo = W1.p;
        const dim3 g2((unsigned)((b + DS_NT - 1) / DS_NT), (unsigned)b);
        hipLaunchKernelGGL(k_ds_prepare, g2, dim3(DS_NT), 0, st, dS, b, Ti, Wi);
        HIPCK(hipGetLastError());
        unsigned long long h[3];
        double level = 0.0, floor_level = 0.0, prev = 0.0;
        int sweeps = 0;
        for (;; sweeps++) {
            HIPCK(hipMemsetAsync(flags.p, 0, 3 * sizeof(unsigned long long), st));
            hipLaunchKernelGGL(k_ds_off, dim3((unsigned)b), dim3(DS_NT), 0, st, Ti, b, flags.p);
            HIPCK(hipGetLastError());
            HIPCK(hipMemcpyAsync(h, flags.p, sizeof(h), hipMemcpyDeviceToHost, st));
            HIPCK(hipStreamSynchronize(st));
            if (h[2]) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "%s", nonfinite);
            double off, all;
            memcpy(&off, &h[0], 8);
            memcpy(&all, &h[1], 8);
            if (sweeps == 0) {
                level = std::sqrt((double)b) * 0x1p-52 * all;
                floor_level = (double)b * 0x1p-52 * all;
            }
            if (off <= level) break;
            if (sweeps > 0 && off <= floor_level && off > 0.5 * prev) break;  // at the rounding floor: another sweep gains nothing
            prev = off;
            if (sweeps >= DS_MAX_SWEEPS)
                return mmidx_fail(MMIDX_ERR_NOT_CONVERGED, "%s: the Jacobi eigen-solve of the %d x %d matrix left off-diagonal %.3e above %.3e after %d sweeps",
                                  what, b, b, off, level, DS_MAX_SWEEPS);
            const bool fused = b <= DS_FUSED_MAX;
            const dim3 gs((unsigned)((b + DS_NT - 1) / DS_NT), (unsigned)(n / 2), 2);
            for (int s = 0; s < n - 1; s++) {
                if (!fused) hipLaunchKernelGGL(k_ds_rot, dim3((unsigned)((n / 2 + DS_NT - 1) / DS_NT)), dim3(DS_NT), 0, st, Ti, b, n, s, rot.p);
                hipLaunchKernelGGL(k_ds_step, gs, dim3(DS_NT), 0, st, (const double *)Ti, To, (const double *)Wi, Wo, fused ? (const double *)nullptr : (const double *)rot.p, b,
                                   n, s);
                std::swap(Ti, To);
                std::swap(Wi, Wo);
            }
            HIPCK(hipGetLastError());
        }
        hipLaunchKernelGGL(k_ds_sort, dim3((unsigned)b), dim3(DS_NT), 0, st, (const double *)Ti, (const double *)Wi, b, d_lam, d_Wt);
        HIPCK(hipGetLastError());
        HIPCK(hipStreamSynchronize(st));
        if (sweeps_out) *sweeps_out = sweeps;
        sweeps_total += sweeps;
        solves++;
        seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return MMIDX_OK;
    }
};

}  // namespace dense_solve
