// mmidx_linear_scan.h -- the kernels of Linear (J/datastructures/Linear.java): append-time side data, the certified scan
// over HBM-resident rows, and the exact path it hands queries back to.  Included by mmidx_linear.hip alone.
//
// The scan of one round of queries (host side: linear_scan_round in mmidx_linear.hip):
//   seed     k_lin_seed      exact fp64 distances to the first S = max(k + 1, 1024) rows -> every query's pool
//            k_lin_reduce    pool -> its k + 1 smallest by (distance bits, row), T[q] = the (k + 1)-th
//   segment  k_lin_qprep     a[q] = T[q] + eps(q) - |q|^2 (-inf for a query that is handed back); zeroes the record counter
//            k_lin_sweep     S(q, x) on v_mfma_f32_16x16x32_bf16 (three products of the bf16 split); record (q, row)
//                            wherever |x|^2 - 2 S <= a[q], i.e. d~ - eps <= T[q]
//            k_lin_verify    exact sequential fp64 distance of every record; into the pool where its key <= T[q]
//            k_lin_reduce    as above: thresholds only fall
//   answer   k_lin_answer    the first k pool entries (nearest first, equal distances later arrival first, as the queue
//                            empties); a query whose k-th and (k + 1)-th distances tie, whose norms fail the guard or that
//                            lost a record to a full list goes to the redo list
//   redo     k_lin_exact     exact distances of the listed queries to all n rows, then K1b (mmidx_internal_select_topw)
// Host synchronisation: ONE per search call -- the number of handed-back queries is read back after k_lin_answer, because
// it sizes the exact path's distance matrix.  Nothing is read back inside the segment loop: the record list is sized from
// the call (or by the option "mfma_qcap"), and a record that does not fit hands its query back.
//
// Certificate: |d~ - d| <= eps(q) = filter_eps_split16(Dp, 2^-21, |q|, |q|^2, max|x|, max|x|^2), max over
// every stored row (kept on the device, raised by k_lin_split at append time); d~ = |x|^2 + |q|^2 - 2 S is evaluated in fp64
// from the rounded-up fp64 norms, so the epilogue's roundings are far inside the 2^-21 the siblings' fp32 epilogues need.
// A row is dropped only where d~ - eps > T[q], hence d > T[q] >= the final threshold: it is neither among the k + 1
// smallest nor tied with the (k + 1)-th.  Queries with (max|x| + |q|)^2 outside filter_norms_usable() are not certified.
#pragma once
#include "mmidx_device_util.h"
#include "mmidx_split16.h"

#define LIN_NT 256
#define LIN_KEY_MAX 0xFFFFFFFFFFFFFFFFull
#define LIN_REDO_TIE 1u
#define LIN_REDO_GUARD 2u
#define LIN_REDO_OVERFLOW 4u

__device__ __forceinline__ u64 lin_key(double d) { return (u64)__double_as_longlong(d); }
__device__ __forceinline__ double lin_keyd(u64 k) { return __longlong_as_double((long long)k); }

// the reference's distance, Linear.java:147-149: sum_j (q_j - x_j)^2, j ascending, no contraction (-ffp-contract=off)
__device__ __forceinline__ double lin_exact_dist(const double *__restrict__ q, const double *__restrict__ x, int D) {
    double s = 0.0;
    for (int j = 0; j < D; j++) {
        const double df = q[j] - x[j];
        s += df * df;
    }
    return s;
}

// one wave per row: X (fp64) -> bf16 head / tail, zero padded to Dp; |x|^2 rounded up; the running maximum of |x|^2
// (as bits: squared norms are >= 0 or NaN, and a NaN's bits exceed every number's, so a NaN row poisons the maximum and
// with it the guard, as it must).  nmax == nullptr: queries.
__global__ __launch_bounds__(LIN_NT) void k_lin_split(const double *__restrict__ X, __bf16 *__restrict__ H, __bf16 *__restrict__ L,
                                                      double *__restrict__ nrm2, u64 *__restrict__ nmax, int D, int Dp, long long n) {
    const long long r = (long long)blockIdx.x * (LIN_NT / 64) + (threadIdx.x >> 6);
    if (r >= n) return;
    const int lane = threadIdx.x & 63;
    double s = 0.0;
    for (int j = lane; j < Dp; j += 64) {
        const double v = j < D ? X[(size_t)r * D + j] : 0.0;
        split16_head_tail((float)v, H[(size_t)r * Dp + j], L[(size_t)r * Dp + j]);
        s += v * v;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) {
        s *= 1.0 + 1e-12;  // only ever used inside the bound and in d~: round up
        nrm2[r] = s;
        if (nmax) atomicMax((unsigned long long *)nmax, (unsigned long long)lin_key(s));
    }
}

__global__ void k_lin_fill(int32_t *__restrict__ iid, double *__restrict__ dist, int32_t *__restrict__ cnt, long long nq, int k) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nq * k) {
        iid[i] = -1;
        dist[i] = __longlong_as_double(0x7ff0000000000000ll);
    }
    if (i < nq) cnt[i] = 0;
}

__global__ void k_lin_gather_rows(const double *__restrict__ X, const int32_t *__restrict__ ids, double *__restrict__ out, int D, long long nq) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq * D) return;
    const long long q = i / D;
    out[i] = X[(size_t)ids[q] * D + (i - q * D)];
}

// pool <- (exact distance, row) of the first S rows; thread = row, blockIdx.y = query (its values are block-uniform)
__global__ __launch_bounds__(LIN_NT) void k_lin_seed(const double *__restrict__ X, const double *__restrict__ Q, u64 *__restrict__ pool_key,
                                                     u32 *__restrict__ pool_row, u32 *__restrict__ pcnt, u32 *__restrict__ pkept,
                                                     u64 *__restrict__ T, u32 *__restrict__ redo, int PC, int D, int S) {
    const int r = blockIdx.x * LIN_NT + threadIdx.x, q = blockIdx.y;
    if (r == 0) {
        pcnt[q] = (u32)S;
        pkept[q] = 0;
        T[q] = LIN_KEY_MAX;
        redo[q] = 0;
    }
    if (r >= S) return;
    pool_key[(size_t)q * PC + r] = lin_key(lin_exact_dist(Q + (size_t)q * D, X + (size_t)r * D, D));
    pool_row[(size_t)q * PC + r] = (u32)r;
}

// one block per query: the pool's entries sorted by (key, row) in LDS, the k1 smallest kept, T lowered to the k1-th
__global__ __launch_bounds__(LIN_NT) void k_lin_reduce(u64 *__restrict__ pool_key, u32 *__restrict__ pool_row, u32 *__restrict__ pcnt,
                                                       u32 *__restrict__ pkept, u64 *__restrict__ T, u32 *__restrict__ redo, int PC, int k1) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lin_smem[];
    u64 *sk = (u64 *)lin_smem;      // [PC]
    u32 *si = (u32 *)(sk + PC);     // [PC]
    const int q = blockIdx.x, tid = threadIdx.x;
    const u32 cnt = pcnt[q], kept = pkept[q];
    __syncthreads();  // (every thread has read the counters before thread 0 rewrites them)
    if (cnt > (u32)PC) {  // entries were lost: the exact path serves this query
        if (tid == 0) {
            redo[q] |= LIN_REDO_OVERFLOW;
            pcnt[q] = kept;
        }
        return;
    }
    if (cnt == kept) return;  // nothing new since the last reduction
    int Pn = 2;
    while (Pn < (int)cnt) Pn <<= 1;
    u64 *gk = pool_key + (size_t)q * PC;
    u32 *gi = pool_row + (size_t)q * PC;
    for (int i = tid; i < Pn; i += LIN_NT) {
        sk[i] = i < (int)cnt ? gk[i] : LIN_KEY_MAX;
        si[i] = i < (int)cnt ? gi[i] : 0xFFFFFFFFu;
    }
    for (int size = 2; size <= Pn; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int i = tid; i < (Pn >> 1); i += LIN_NT) {
                const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                const bool asc = (lo & size) == 0;
                const u64 ka = sk[lo], kb = sk[hi];
                const u32 ia = si[lo], ib = si[hi];
                const bool gt = ka > kb || (ka == kb && ia > ib);
                if (gt == asc) {
                    sk[lo] = kb;
                    sk[hi] = ka;
                    si[lo] = ib;
                    si[hi] = ia;
                }
            }
        }
    }
    __syncthreads();
    const int m = (int)cnt < k1 ? (int)cnt : k1;
    for (int i = tid; i < m; i += LIN_NT) {
        gk[i] = sk[i];
        gi[i] = si[i];
    }
    if (tid == 0) {
        pcnt[q] = (u32)m;
        pkept[q] = (u32)m;
        if (m == k1) T[q] = sk[k1 - 1];
    }
}

// a[q] = T[q] + eps(q) - |q|^2: the sweep passes a row where |x|^2 - 2 S <= a[q].  -inf where the query is handed back.
__global__ void k_lin_qprep(const double *__restrict__ qn, const u64 *__restrict__ nmax, const u64 *__restrict__ T, u32 *__restrict__ redo,
                            double *__restrict__ a, u32 *__restrict__ rec_cnt, int Dp, int nq) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q == 0) *rec_cnt = 0;
    if (q >= nq) return;
    const double ninf = __longlong_as_double((long long)0xfff0000000000000ull);
    const double cn2 = lin_keyd(*nmax), qn2 = qn[q];
    const double cnorm = sqrt(cn2) * (1.0 + 1e-15), qnorm = sqrt(qn2) * (1.0 + 1e-15);
    const double t = lin_keyd(T[q]);
    u32 rd = redo[q];
    if (!filter_norms_usable(cnorm + qnorm) || !(t < __longlong_as_double(0x7ff0000000000000ll))) {
        rd |= LIN_REDO_GUARD;
        redo[q] = rd;
    }
    if (rd) {
        a[q] = ninf;
        return;
    }
    const double eps = filter_eps_split16(Dp, 0x1p-21, qnorm, qn2, cnorm, cn2);
    a[q] = (t + eps) * (1.0 + 1e-15) - qn2 * (1.0 - 1e-12);  // (rounded towards keeping a row)
}

// The sweep.  grid = (ceil(nq / 128), row groups); block = 4 waves, wave w owns queries [32 w, 32 w + 32) of the block's 128
// as two 16-row A tiles; a row group = 64 stored rows = four 16-column B tiles, read straight from global memory (the four
// waves of a block read the same rows: L1).  Fragments of v_mfma_f32_16x16x32_bf16: lane l holds A[row l & 15][k = 8 (l >> 4) ..]
// and B[k = 8 (l >> 4) ..][col l & 15]; result register r of lane l is (row 4 (l >> 4) + r, col l & 15).
// Rows past r1 and queries past nq are clamped for the loads (in bounds) and never recorded.
__global__ __launch_bounds__(LIN_NT, 2) void k_lin_sweep(const __bf16 *__restrict__ Qh, const __bf16 *__restrict__ Ql,
                                                         const __bf16 *__restrict__ Xh, const __bf16 *__restrict__ Xl,
                                                         const double *__restrict__ xn, const double *__restrict__ a, u64 *__restrict__ rec,
                                                         u32 *__restrict__ rec_cnt, u32 rec_cap, u32 *__restrict__ redo, int Dp, int nq,
                                                         long long r0, long long r1) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fg = lane >> 4;
    const int q0 = blockIdx.x * 128 + wave * 32;
    if (q0 >= nq) return;  // (wave-uniform; no barrier in this kernel)
    const int nkc = (Dp + 127) / 128;
    const double ninf = __longlong_as_double((long long)0xfff0000000000000ull);
    double aq[2][4];
    bool any_q = false;
#pragma unroll
    for (int rt = 0; rt < 2; rt++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int q = q0 + rt * 16 + 4 * fg + r;
            aq[rt][r] = q < nq ? a[q] : ninf;
            any_q |= aq[rt][r] > ninf;
        }
    if (!__any(any_q)) return;  // every query of the wave is handed back already
    bf16x8 ah[2][4], al[2][4];
    auto load_a = [&](int kc) { split16_load_a<true>(ah, al, Qh, Ql, q0, nq, Dp, kc * 128, fr, fg); };
    if (nkc == 1) load_a(0);
    const long long ngroups = (r1 - r0 + 63) / 64;
    const u64 lane_lt = (1ull << lane) - 1ull;
    for (long long g = blockIdx.y; g < ngroups; g += gridDim.y) {
        const long long c0 = r0 + g * 64;
        long long rowc[4];
#pragma unroll
        for (int ct = 0; ct < 4; ct++) {
            const long long row = c0 + ct * 16 + fr;
            rowc[ct] = row < r1 ? row : r1 - 1;
        }
        f32x4 acc[2][4];
#pragma unroll
        for (int rt = 0; rt < 2; rt++)
#pragma unroll
            for (int ct = 0; ct < 4; ct++) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int kc = 0; kc < nkc; kc++) {
            if (nkc > 1) load_a(kc);
#pragma unroll
            for (int ks = 0; ks < 4; ks++) {
                const int k = kc * 128 + ks * 32 + fg * 8;
                if (kc * 128 + ks * 32 < Dp) {  // wave-uniform
                    bf16x8 bh[4], bl[4];
#pragma unroll
                    for (int ct = 0; ct < 4; ct++) {
                        bh[ct] = *(const bf16x8 *)(Xh + (size_t)rowc[ct] * Dp + k);
                        bl[ct] = *(const bf16x8 *)(Xl + (size_t)rowc[ct] * Dp + k);
                    }
                    split16_mma_step<4>(acc, 0, ah, al, ks, bh, bl);
                }
            }
        }
        // epilogue: |x|^2 - 2 S <= a[q] in fp64; survivors are appended with one atomic per wave and test
#pragma unroll
        for (int ct = 0; ct < 4; ct++) {
            const long long row = c0 + ct * 16 + fr;
            const bool rvalid = row < r1;
            const double xn_c = xn[rowc[ct]];
#pragma unroll
            for (int rt = 0; rt < 2; rt++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const double t = xn_c - 2.0 * (double)acc[rt][ct][r];
                    const bool pass = rvalid && t <= aq[rt][r];
                    const u64 mask = __ballot(pass);
                    if (mask) {
                        u32 base = 0;
                        const int leader = __ffsll((long long)mask) - 1;
                        if (lane == leader) base = atomicAdd(rec_cnt, (u32)__popcll(mask));
                        base = wave_read_u32(base, leader);
                        if (pass) {
                            const u32 slot = base + (u32)__popcll(mask & lane_lt);
                            const int q = q0 + rt * 16 + 4 * fg + r;
                            if (slot < rec_cap)
                                rec[slot] = ((u64)(u32)q << 32) | (u64)(u32)row;
                            else
                                atomicOr(&redo[q], LIN_REDO_OVERFLOW);
                        }
                    }
                }
        }
    }
}

// exact distance of every record; into its query's pool where the key does not exceed the threshold
__global__ __launch_bounds__(LIN_NT) void k_lin_verify(const double *__restrict__ X, const double *__restrict__ Q, const u64 *__restrict__ rec,
                                                       const u32 *__restrict__ rec_cnt, u32 rec_cap, const u64 *__restrict__ T,
                                                       u64 *__restrict__ pool_key, u32 *__restrict__ pool_row, u32 *__restrict__ pcnt,
                                                       u64 *__restrict__ surv_total, int PC, int D) {
    const u32 have = *rec_cnt;
    const u32 nrec = have < rec_cap ? have : rec_cap;
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd((unsigned long long *)surv_total, (unsigned long long)nrec);
    for (u32 i = blockIdx.x * LIN_NT + threadIdx.x; i < nrec; i += gridDim.x * LIN_NT) {
        const u64 rc = rec[i];
        const u32 q = (u32)(rc >> 32), row = (u32)rc;
        const u64 key = lin_key(lin_exact_dist(Q + (size_t)q * D, X + (size_t)row * D, D));
        if (key <= T[q]) {
            const u32 slot = atomicAdd(&pcnt[q], 1u);  // (past PC: counted, not stored -- k_lin_reduce sees the overflow)
            if (slot < (u32)PC) {
                pool_key[(size_t)q * PC + slot] = key;
                pool_row[(size_t)q * PC + slot] = row;
            }
        }
    }
}

// thread per query: the answer, or the query's index appended to the redo list
__global__ void k_lin_answer(const u64 *__restrict__ pool_key, const u32 *__restrict__ pool_row, const u32 *__restrict__ pcnt,
                             u32 *__restrict__ redo, int PC, int k, int32_t *__restrict__ iid_out, double *__restrict__ dist_out,
                             int32_t *__restrict__ cnt_out, int32_t *__restrict__ redo_list, u32 *__restrict__ redo_cnt, int nq) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    const u64 *pk = pool_key + (size_t)q * PC;
    const u32 *pr = pool_row + (size_t)q * PC;
    const int m = (int)pcnt[q];
    u32 rd = redo[q];
    if (!rd && m >= k + 1 && pk[k - 1] == pk[k]) {  // the kept entries cannot tell which of the tied rows the queue keeps
        rd = LIN_REDO_TIE;
        redo[q] = rd;
    }
    if (rd) {
        redo_list[atomicAdd(redo_cnt, 1u)] = q;
        return;
    }
    const int n = m < k ? m : k;
    int32_t *io = iid_out + (size_t)q * k;
    double *dd = dist_out + (size_t)q * k;
    int s = 0;
    while (s < n) {  // nearest first; inside a run of equal distances the later arrival (larger row) first
        int e = s;
        while (e + 1 < n && pk[e + 1] == pk[s]) e++;
        for (int t = s; t <= e; t++) {
            io[t] = (int32_t)pr[e - (t - s)];
            dd[t] = lin_keyd(pk[s]);
        }
        s = e + 1;
    }
    cnt_out[q] = n;
}

// The exact path: out[r][row] = distance of query qidx[r] (r itself where qidx is null) to every stored row.  A block takes
// 256 rows, 16 dimensions at a time through LDS (coalesced 128-byte reads of each row; thread = row sums in dimension order).
template <int QT>
__global__ __launch_bounds__(LIN_NT) void k_lin_exact(const double *__restrict__ X, const double *__restrict__ Q, const int32_t *__restrict__ qidx,
                                                      double *__restrict__ out, int D, long long n, int nr) {
    __shared__ double tile[LIN_NT][17];
    const int tid = threadIdx.x;
    const long long row0 = (long long)blockIdx.x * LIN_NT;
    const int r0 = blockIdx.y * QT;
    const double *qp[QT];
    double acc[QT];
#pragma unroll
    for (int t = 0; t < QT; t++) {
        const int r = r0 + t < nr ? r0 + t : nr - 1;
        qp[t] = Q + (size_t)(qidx ? qidx[r] : r) * D;
        acc[t] = 0.0;
    }
    for (int j0 = 0; j0 < D; j0 += 16) {
        const int jw = D - j0 < 16 ? D - j0 : 16;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int e = tid + i * LIN_NT, rr = e >> 4, jj = e & 15;
            long long row = row0 + rr;
            row = row < n ? row : n - 1;
            tile[rr][jj] = jj < jw ? X[(size_t)row * D + j0 + jj] : 0.0;
        }
        __syncthreads();
        for (int jj = 0; jj < jw; jj++) {
            const double x = tile[tid][jj];
#pragma unroll
            for (int t = 0; t < QT; t++) {
                const double df = qp[t][j0 + jj] - x;
                acc[t] += df * df;
            }
        }
    }
    const long long row = row0 + tid;
    if (row < n) {
#pragma unroll
        for (int t = 0; t < QT; t++)
            if (r0 + t < nr) out[(size_t)(r0 + t) * n + row] = acc[t];
    }
}

// cells [nr][w] (K1b's order) -> the answer rows of the queries qidx[r] (r where null); the distance comes from the selected
// list dsel [nr][w] or from the exact matrix dmat [nr][n]
__global__ void k_lin_place(const int32_t *__restrict__ cells, const double *__restrict__ dsel, const double *__restrict__ dmat,
                            const int32_t *__restrict__ qidx, long long n, int w, int k, int32_t *__restrict__ iid_out,
                            double *__restrict__ dist_out, int32_t *__restrict__ cnt_out, long long nr) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nr * w) return;
    const long long r = i / w;
    const int t = (int)(i - r * w);
    const long long q = qidx ? qidx[r] : r;
    const int32_t c = cells[i];
    iid_out[(size_t)q * k + t] = c;
    dist_out[(size_t)q * k + t] = dsel ? dsel[i] : dmat[(size_t)r * n + c];
    if (t == 0) cnt_out[q] = w;
}
