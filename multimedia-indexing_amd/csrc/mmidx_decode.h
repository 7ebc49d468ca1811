// mmidx_decode.h -- K10: stored records back to vectors.  Included by mmidx_decode.hip only.
//
// A record is (list, code).  The vector the index holds for it:
//   1. z[s * dsub + t] = pq[s][code[s]][t]                     (the codes on the device hold the index itself, not the stored byte - 128)
//   2. y = z                                                   no transformation
//      y[perm[i]] = z[i]                                       RandomPermutation (the search permutes by tr[i] = r[perm[i]])
//      y[i] = sum_j z[j] * R[i][j], j ascending from 0.0       RandomRotation (the search rotates by tr[j] = sum_i r[i] R[i][j], R orthogonal);
//                                                              every product is rounded before its add (__dmul_rn / __dadd_rn: never fused)
//   3. x[d] = coarse[list][d] - y[d] for IVFPQ (the residual is centroid - vector, IVFPQ.java:645), x = y for PQ
//
// k_decode_records<CodeT, R>: a block takes R consecutive records of the call.
//   - R lanes find the records: position through the iid -> position table, list by bisection of the list offsets (the last
//     list whose start is <= position, as lookup_records does on the host).
//   - lanes walk j = 0 .. D-1 in steps of the block size; the dsub doubles of a codebook row are consecutive lanes' reads.  z lands in
//     LDS, for a permutation already at its place perm[j] (the scatter is an LDS write, never a global one).
//   - rotation: lane i keeps R accumulators, reads rotT[j * D + i] (consecutive lanes, consecutive doubles; one read serves the R
//     records) and takes z[r][j] as an LDS broadcast.  Each output is its own chain over j.
//   - the rows leave with consecutive lanes on consecutive doubles.  A record that does not exist gets a row of zeros, found = 0.
// D is covered by loops, never by the block size (4 .. 2048 and beyond, as far as R * D doubles fit the LDS).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

struct DecodeParams {
    const int32_t *iids;      // [n] internal ids
    const int32_t *inv;       // [inv_size] iid -> position in the list-major arrays, -1 = absent
    const long long *off;     // [nlists + 1] list offsets
    const void *codes;        // [n_csr][m]
    const double *pq;         // [m][ks][dsub]
    const double *coarse;     // [C][D] (IVFPQ)
    const int32_t *perm;      // [D] (RandomPermutation)
    const double *rotT;       // [D][D], rotT[j][i] = R[i][j] (RandomRotation)
    double *X;                // [n][D] out
    int32_t *found;           // [n] out, may be null
    long long n, inv_size, n_csr;
    int nlists, D, m, ks, dsub, transform, ivf;
};

template <typename CodeT, int R>
__global__ __launch_bounds__(256) void k_decode_records(const DecodeParams P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dec_smem[];
    double *z = (double *)dec_smem;            // [R][D]
    int32_t *s_pos = (int32_t *)(z + (size_t)R * P.D);  // [R] position, -1 = no such record, -2 = past the end of the call
    int32_t *s_cell = s_pos + R;               // [R]
    const int tid = threadIdx.x, nt = blockDim.x, D = P.D;
    const long long r0 = (long long)blockIdx.x * R;
    if (tid < R) {
        const long long r = r0 + tid;
        int32_t pos = -2, cell = 0;
        if (r < P.n) {
            const int32_t id = P.iids[r];
            pos = (id >= 0 && id < P.inv_size) ? P.inv[id] : -1;
            if (pos < -1 || pos >= P.n_csr) pos = -1;
            if (pos >= 0 && P.ivf) {
                // first list whose start is > pos, minus one (empty lists share a start: the last of them is the one that holds pos)
                int lo = 0, hi = P.nlists + 1;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (P.off[mid] <= (long long)pos) lo = mid + 1;
                    else hi = mid;
                }
                cell = lo - 1;
                if (cell < 0 || cell >= P.nlists) pos = -1;  // (offsets that do not cover the position: treated as absent, nothing is read)
            }
            if (P.found) P.found[r] = pos >= 0 ? 1 : 0;
        }
        s_pos[tid] = pos;
        s_cell[tid] = cell;
    }
    __syncthreads();
    // 1. the codebook rows the code selects
    const CodeT *codes = (const CodeT *)P.codes;
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int32_t pos = s_pos[r];  // (uniform)
        if (pos == -2) break;
        for (int j = tid; j < D; j += nt) {
            double v = 0.0;
            if (pos >= 0) {
                const int s = j / P.dsub, t = j - s * P.dsub;
                int a = (int)codes[(size_t)pos * P.m + s];
                a = a < P.ks ? a : P.ks - 1;  // (adds validate the codes; an index past the codebook is never formed)
                v = P.pq[((size_t)s * P.ks + a) * P.dsub + t];
            }
            int dst = j;
            if (P.transform == 2) {
                dst = P.perm[j];
                dst = (dst >= 0 && dst < D) ? dst : j;
            }
            z[(size_t)r * D + dst] = v;
        }
    }
    __syncthreads();
    // 2. + 3.
    if (P.transform == 1) {
        for (int i = tid; i < D; i += nt) {
            double acc[R];
#pragma unroll
            for (int r = 0; r < R; r++) acc[r] = 0.0;
#pragma unroll 4
            for (int j = 0; j < D; j++) {
                const double rv = P.rotT[(size_t)j * D + i];
#pragma unroll
                for (int r = 0; r < R; r++) acc[r] = __dadd_rn(acc[r], __dmul_rn(z[(size_t)r * D + j], rv));
            }
#pragma unroll
            for (int r = 0; r < R; r++) {
                const int32_t pos = s_pos[r];
                if (pos == -2) break;
                double x = 0.0;
                if (pos >= 0) x = P.ivf ? P.coarse[(size_t)s_cell[r] * D + i] - acc[r] : acc[r];
                P.X[(size_t)(r0 + r) * D + i] = x;
            }
        }
        return;
    }
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int32_t pos = s_pos[r];
        if (pos == -2) break;
        const size_t crow = (size_t)s_cell[r] * D;
        for (int i = tid; i < D; i += nt) {
            double x = 0.0;
            if (pos >= 0) {
                const double y = z[(size_t)r * D + i];
                x = P.ivf ? P.coarse[crow + i] - y : y;
            }
            P.X[(size_t)(r0 + r) * D + i] = x;
        }
    }
}

// found[i] = 1 where iids[i] is a stored record (the host forms check a whole call before they write anything)
__global__ void k_ids_found(const int32_t *__restrict__ iids, long long n, const int32_t *__restrict__ inv, long long inv_size, long long n_csr,
                            int32_t *__restrict__ found) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t id = iids[i];
    const int32_t pos = (id >= 0 && id < inv_size) ? inv[id] : -1;
    found[i] = (pos >= 0 && pos < n_csr) ? 1 : 0;
}

// dst[j][i] = src[i][j] for a D x D matrix, 32 x 32 tiles through LDS (both sides coalesced); block (32, 8)
__global__ void k_transpose_square(const double *__restrict__ src, double *__restrict__ dst, int D) {
    __shared__ double tile[32][33];
    const int bx = blockIdx.x * 32, by = blockIdx.y * 32;
    for (int r = threadIdx.y; r < 32; r += 8) {
        const int i = by + r, j = bx + threadIdx.x;
        tile[r][threadIdx.x] = (i < D && j < D) ? src[(size_t)i * D + j] : 0.0;
    }
    __syncthreads();
    for (int r = threadIdx.y; r < 32; r += 8) {
        const int j = bx + r, i = by + threadIdx.x;
        if (i < D && j < D) dst[(size_t)j * D + i] = tile[threadIdx.x][r];
    }
}

// the rows of an id query whose id does not exist: count -1, ids -1, distances +inf.  One thread per answer slot.
__global__ void k_mark_unknown_rows(const int32_t *__restrict__ found, long long nq, int k, int32_t *__restrict__ iid, double *__restrict__ dist,
                                    int32_t *__restrict__ cnt) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nq * k) return;
    const long long q = e / k;
    if (found[q]) return;
    iid[e] = -1;
    dist[e] = __longlong_as_double(0x7FF0000000000000ll);
    if (e == q * k) cnt[q] = -1;
}
