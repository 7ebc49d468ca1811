// mmidx_refine.h -- the kernels of the exact re-ranking (mmidx_search_refine*): the R best records of a PQ / IVFPQ
// answer meet their full vectors in a Linear handle's HBM rows and the k best of them by exact distance come back.
// Included by mmidx_refine.hip alone.
//
//   K11g  k_refine_gather_queries  the _ids form: row iids[q] of the Linear rows is query q (Linear.java:181-184); an id outside
//                                 [0, n) gives a row of zeros and valid[q] = 0, and is never dereferenced
//   K11a  k_refine_dist            block = (query, tile of 256 candidates), thread = candidate: d = sum_j (q_j - x_j)^2, j ascending,
//                                 fp64, uncontracted (Linear.java:147-149).  The candidates' rows come 16 dimensions at a time
//                                 through LDS, 128 coalesced bytes of each row per piece.  A record whose internal id is outside
//                                 [0, n) is dropped: its id in the candidate list becomes -1, its row is never read, and the
//                                 block adds its dropped records to `missing` with one atomic.
//   K11b  k_refine_select          block = query: the pairs (distance bits, offer position) of the records that are left, sorted in
//                                 LDS, then the bounded queue of size k in closed form (below); ids, distances, count.
//
// The queue (LingPipe BoundedPriorityQueue as ASS.lookUp drives it): the candidates are offered in the order of the compressed
// answer.  While fewer than k are held every one is accepted; afterwards a candidate equal to the worst held is rejected and a
// better one evicts the earliest-inserted of the equal-worst.  With tau the k-th smallest distance, "better" d < tau, "ties"
// d == tau, and s the offer position of the k-th candidate with d <= tau: p = ties offered up to s, e = better offered after s;
// the queue ends with every better candidate and the ties number e .. p-1 in offer order (exactly k entries).  It empties nearest
// first, and among equal distances the later offer first.  Squared distances are >= 0, so they order as their bits.
#pragma once
#include "mmidx_device_util.h"

#define RF_NT 256
#define RF_CAP 4096                  // most pairs K11b sorts: MMIDX_K_MAX + 1; 32 KiB of keys + 16 KiB of positions in LDS
#define RF_KEY_MAX 0xFFFFFFFFFFFFFFFFull
#define RF_POS_NONE 0xFFFFFFFFu

__global__ void k_refine_gather_queries(const double *__restrict__ X, long long n, int D, const int32_t *__restrict__ ids, double *__restrict__ out,
                                        int32_t *__restrict__ valid, long long nq) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq * D) return;
    const long long q = i / D;
    const int j = (int)(i - q * D);
    const long long id = ids[q];
    const bool ok = id >= 0 && id < n;
    out[i] = ok ? X[(size_t)id * D + j] : 0.0;
    if (j == 0) valid[q] = ok ? 1 : 0;
}

// cand_iid [nq][R] (the compressed answer, -1 beyond cand_cnt[q]) -> cand_dist [nq][R] exact distances; dropped records' ids -> -1
__global__ __launch_bounds__(RF_NT) void k_refine_dist(const double *__restrict__ X, long long n, int D, const double *__restrict__ Q,
                                                       const int32_t *__restrict__ qvalid, int R, int32_t *__restrict__ cand_iid,
                                                       double *__restrict__ cand_dist, const int32_t *__restrict__ cand_cnt,
                                                       unsigned long long *__restrict__ missing) {
    __shared__ double tile[RF_NT][17];
    __shared__ int32_t s_row[RF_NT];
    const int tid = threadIdx.x;
    const long long q = blockIdx.x;
    const int c0 = blockIdx.y * RF_NT;
    int nc = cand_cnt[q];
    nc = nc < R ? nc : R;
    if (c0 >= nc || (qvalid && !qvalid[q])) return;  // (block-uniform) nothing offered in this tile / no such query
    const int c = c0 + tid;
    const size_t slot = (size_t)q * R + c;
    const long long iid = c < nc ? (long long)cand_iid[slot] : -1;
    const bool have = iid >= 0 && iid < n;
    s_row[tid] = have ? (int32_t)iid : -1;
    const int nmiss = __syncthreads_count(c < nc && !have);
    if (c < nc && !have) cand_iid[slot] = -1;
    if (tid == 0 && nmiss > 0 && missing) atomicAdd(missing, (unsigned long long)nmiss);
    const double *qp = Q + (size_t)q * D;
    double acc = 0.0;
    for (int j0 = 0; j0 < D; j0 += 16) {
        const int jw = D - j0 < 16 ? D - j0 : 16;
        if (j0) __syncthreads();
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int e = tid + i * RF_NT, rr = e >> 4, jj = e & 15;
            const int32_t row = s_row[rr];
            tile[rr][jj] = (row >= 0 && jj < jw) ? X[(size_t)row * D + j0 + jj] : 0.0;
        }
        __syncthreads();
        for (int jj = 0; jj < jw; jj++) {
            const double df = qp[j0 + jj] - tile[tid][jj];
            acc += df * df;
        }
    }
    if (have) cand_dist[slot] = acc;
}

__device__ __forceinline__ bool rf_less(u64 ka, u32 pa, u64 kb, u32 pb) { return ka < kb || (ka == kb && pa < pb); }

// One block per query.  Sorted order: distance bits ascending, then offer position DESCENDING (the stored word is RF_CAP - 1 - position),
// which is the order the queue empties in; dropped records and the padding of the power of two sort last.  CAP >= R: the LDS arrays
// are sized by it (512: 6 KiB, 1024: 12 KiB, 4096: 49 KiB), so that small R keeps more queries in flight per CU.
template <int CAP>
__global__ __launch_bounds__(RF_NT) void k_refine_select(int k, int R, const int32_t *__restrict__ qvalid, const int32_t *__restrict__ cand_iid,
                                                         const double *__restrict__ cand_dist, const int32_t *__restrict__ cand_cnt,
                                                         int32_t *__restrict__ iid_out, double *__restrict__ dist_out, int32_t *__restrict__ cnt_out) {
    __shared__ u64 s_key[CAP];
    __shared__ u32 s_rp[CAP];
    __shared__ u32 s_bits[CAP / 32];
    __shared__ int s_sm, s_p;
    const int tid = threadIdx.x;
    const long long q = blockIdx.x;
    const int32_t *ci = cand_iid + (size_t)q * R;
    const double *cd = cand_dist + (size_t)q * R;
    int32_t *io = iid_out + (size_t)q * k;
    double *dd = dist_out + (size_t)q * k;
    int nc = cand_cnt[q];
    nc = nc < 0 ? 0 : (nc < R ? nc : R);
    if (qvalid && !qvalid[q]) nc = 0;
    int P = 2;
    while (P < nc) P <<= 1;
    int mine = 0;
    for (int i = tid; i < P; i += RF_NT) {
        const bool have = i < nc && ci[i] >= 0;
        s_key[i] = have ? (u64)__double_as_longlong(cd[i]) : RF_KEY_MAX;
        s_rp[i] = have ? (u32)(RF_CAP - 1 - i) : RF_POS_NONE;
        mine += have ? 1 : 0;
    }
    for (int i = tid; i < CAP / 32; i += RF_NT) s_bits[i] = 0u;
    if (tid == 0) {
        s_sm = 0;
        s_p = 0;
    }
    // m = records left (a block-wide sum through the barrier's count: one round per entry a thread loaded, 16 at most)
    int m = 0;
    for (int r = 0; r < (P + RF_NT - 1) / RF_NT; r++) m += __syncthreads_count(mine > r);
    for (int k2 = 2; k2 <= P; k2 <<= 1) {
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += RF_NT) {
                const int x = i ^ j;
                if (x > i) {
                    const u64 ka = s_key[i], kb = s_key[x];
                    const u32 pa = s_rp[i], pb = s_rp[x];
                    const bool up = (i & k2) == 0;
                    if (up ? rf_less(kb, pb, ka, pa) : rf_less(ka, pa, kb, pb)) {
                        s_key[i] = kb;
                        s_key[x] = ka;
                        s_rp[i] = pb;
                        s_rp[x] = pa;
                    }
                }
            }
            __syncthreads();
        }
    }
    const int cnt = m < k ? m : k;
    int nb = cnt, shift = 0;  // slot t of the answer is sorted entry t (t < nb) or t + shift
    if (m > k) {
        const u64 tau = s_key[k - 1];
        int lo = 0, hi = k - 1;  // nb = first entry with key == tau
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_key[mid] < tau) lo = mid + 1;
            else hi = mid;
        }
        nb = lo;
        lo = k;
        hi = m;  // first entry with key > tau
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_key[mid] <= tau) lo = mid + 1;
            else hi = mid;
        }
        const int nj = lo, nt = nj - nb;  // candidates with d <= tau, ties
        if (nj > k) {                     // (nj == k: the k-th and (k + 1)-th distances differ, the first k sorted entries are the answer)
            for (int i = tid; i < nj; i += RF_NT) {
                const u32 pos = (u32)(RF_CAP - 1) - s_rp[i];
                atomicOr(&s_bits[pos >> 5], 1u << (pos & 31));
            }
            __syncthreads();
            if (tid == 0) {  // s = offer position of the k-th candidate with d <= tau
                int seen = 0, w = 0;
                while (seen + __popc(s_bits[w]) < k) seen += __popc(s_bits[w++]);
                u32 word = s_bits[w];
                for (int r = k - seen; r > 1; r--) word &= word - 1;
                s_sm = w * 32 + (__ffs((int)word) - 1);
            }
            __syncthreads();
            const int sm = s_sm;
            int p = 0;  // ties offered up to s (e = nb + p - k follows: the queue holds k)
            for (int i = nb + tid; i < nj; i += RF_NT) p += (RF_CAP - 1) - (int)s_rp[i] <= sm ? 1 : 0;
            if (p) atomicAdd(&s_p, p);
            __syncthreads();
            // ties in offer order e .. p-1 = sorted entries nb + nt - p .. nb + nt - 1 - e (the positions descend)
            shift = nt - s_p;
        }
    }
    for (int t = tid; t < k; t += RF_NT) {
        if (t < cnt) {
            const int i = t < nb ? t : t + shift;
            io[t] = ci[(RF_CAP - 1) - (int)s_rp[i]];
            dd[t] = __longlong_as_double((long long)s_key[i]);
        } else {
            io[t] = -1;
            dd[t] = __longlong_as_double(0x7ff0000000000000ll);
        }
    }
    if (tid == 0) cnt_out[q] = cnt;
}
