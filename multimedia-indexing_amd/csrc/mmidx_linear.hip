// mmidx_linear.hip -- Linear: exhaustive exact search (J/datastructures/Linear.java).  The indexed vectors live in HBM in arrival
// order with the side data of the scan (bf16 head / tail, squared norms), produced at append time for the new rows only.
// A search is served by one of three paths (mmidx_linear_stats.path):
//   1  n <= 16384 and w + 1 <= 256: the vectors are the "centroids" of a hidden index handle and the search is that handle's
//      certified coarse stage (mmidx_internal_coarse_topw); a host mirror of the rows exists only while the index is this small
//   3  beyond that: the certified scan of mmidx_linear_scan.h (seed, matrix-core sweep, exact verification, falling thresholds)
//   2  the exact path: fp64 distances to every row for the queries concerned, then K1b (mmidx_internal_select_topw) -- for the
//      queries the scan hands back, for shapes outside its envelope, and for everything with the option "exact"
#include "mmidx_host.h"
#include "mmidx_linear_scan.h"

#include <algorithm>
#include <cstring>
#include <limits>
#include <mutex>
#include <vector>

// ---- Linear (exhaustive exact search, J/datastructures/Linear.java) -----------------------------------------------
// computeNearestNeighborsInternal (Linear.java:138-163) offers (i, sum_j (q_j - x_ij)^2) for every vector in index order
// to a bounded queue of size k: exactly what computeNearestCoarseIndices does with the coarse centroids and w; (q - x)^2 and
// (x - q)^2 are the same bits.

#define LIN_SMALL_N (64 * 256)        // largest index the hidden handle's certified coarse stage serves (coarse_certified)
#define LIN_SMALL_W1 256              // ... and the largest w + 1
#define LIN_MAX_D 4096                // envelope of the scan: vector length ...
#define LIN_MAX_K 4095                // ... and k (a pool of 2 (k + 1) entries is sorted in LDS)
#define LIN_SEED_ROWS 1024
#define LIN_POOL_MAX 8192
#define LIN_REC_MAX (32ll << 20)      // records of one round of queries (8 bytes each)

namespace {

struct LinStatsAcc {
    int path = 0, segments = 0;
    int64_t rows_scanned = 0, survivors = 0, redo_queries = 0, uploaded_rows = 0;
    double scan_ms = 0, verify_ms = 0;
};

}  // namespace

extern "C" {

struct MMIDX_HIDDEN mmidx_linear {
    Stream stream;  // first: members are destroyed in reverse order, and everything below was used on it
    mutable std::mutex mu;
    int D = 0, Dp = 0, device = 0;
    int64_t capacity = 0;
    int64_t n = 0, cap = 0;           // rows stored / rows the device arrays have room for
    DevPtr<double> dX;                // [cap][D], arrival order (TDoubleArrayList, Linear.java:45)
    DevPtr<__bf16> dXh, dXl;          // [cap][Dp]
    DevPtr<double> dxn;               // [cap] |x|^2, rounded up
    DevPtr<u64> d_nmax;               // bits of the largest |x|^2 so far
    std::vector<double> X;            // host mirror for the hidden handle, kept only while n <= LIN_SMALL_N
    bool mirror = true;
    mmidx_index *inner = nullptr;
    int64_t inner_n = -1;   // number of vectors the inner handle was built for
    hipStream_t last_stream = nullptr;  // a _device call is asynchronous on its caller's stream: the next call on another waits
    bool last_stream_valid = false;
    int opt_exact = 0, opt_qcap = 0, opt_prof = 0;
    LinStatsAcc st;
    DevBuf<double> ws_Q, ws_d, ws_cd, ws_qn, ws_a, ws_dmat;
    DevBuf<int32_t> ws_i, ws_c, ws_cells, ws_redo, ws_ids;
    DevBuf<unsigned short> ws_Qh, ws_Ql;
    DevBuf<u64> ws_T, ws_pk, ws_rec, ws_ctr;
    DevBuf<u32> ws_u32, ws_pr;
    Combiner comb;              // concurrent one-query callers are served together, as in mmidx_search
    std::vector<double> cat_Q;  // their queries, concatenated
};

}  // extern "C"

namespace {

void lin_wait_other_stream(mmidx_linear *l, hipStream_t st) {
    if (l->last_stream_valid && l->last_stream != st) {
        if (hipStreamSynchronize(l->last_stream) != hipSuccess) {  // (the caller may have destroyed that stream)
            (void)hipGetLastError();
            (void)hipDeviceSynchronize();
        }
    }
    l->last_stream = st;
    l->last_stream_valid = true;
}

// room for `need` rows; on failure nothing has changed.  Growth by half: an append copies earlier rows only when the arrays
// are full, O(1) amortised per row.
int lin_grow(mmidx_linear *l, int64_t need) {
    if (!l->d_nmax) {
        HIPCK(l->d_nmax.alloc(1));
        HIPCK(hipMemset(l->d_nmax, 0, 8));
    }
    if (need <= l->cap) return MMIDX_OK;
    int64_t cap = std::max<int64_t>(std::max<int64_t>(need, l->cap + l->cap / 2), 4096);
    if (l->capacity > 0) cap = std::max<int64_t>(need, std::min<int64_t>(cap, l->capacity));
    DevPtr<double> nX, nN;
    DevPtr<__bf16> nH, nL;
    hipError_t e = nX.alloc((size_t)cap * l->D);
    if (e == hipSuccess) e = nH.alloc((size_t)cap * l->Dp);
    if (e == hipSuccess) e = nL.alloc((size_t)cap * l->Dp);
    if (e == hipSuccess) e = nN.alloc((size_t)cap);
    if (e == hipSuccess && l->n > 0) {
        hipStream_t st = l->stream;
        lin_wait_other_stream(l, st);
        e = hipMemcpyAsync(nX, l->dX, (size_t)l->n * l->D * 8, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(nH, l->dXh, (size_t)l->n * l->Dp * 2, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(nL, l->dXl, (size_t)l->n * l->Dp * 2, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(nN, l->dxn, (size_t)l->n * 8, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return mmidx_fail(MMIDX_ERR_HIP, "Linear: no room for %lld vectors on device %d: %s", (long long)need, l->device, hipGetErrorString(e));
    }
    l->dX = std::move(nX);
    l->dXh = std::move(nH);
    l->dXl = std::move(nL);
    l->dxn = std::move(nN);
    l->cap = cap;
    return MMIDX_OK;
}

// indexVectorInternal, Linear.java:111-122, for n rows at once: only the new rows are moved and split.  The caller holds l->mu.
int lin_append(mmidx_linear *l, int64_t n, const double *src, bool on_device, hipStream_t st) {
    const int64_t have = l->n;
    if (l->capacity > 0 && have + n > l->capacity) return mmidx_fail(MMIDX_ERR_CAPACITY, "Maximum index capacity reached, no more vectors can be indexed!");
    if (have + n > 0x7fffffff) return mmidx_fail(MMIDX_ERR_CAPACITY, "internal ids are 32-bit, as in the reference");
    l->st.uploaded_rows = 0;
    if (n == 0) return MMIDX_OK;
    HIPCK(hipSetDevice(l->device));
    int rc = lin_grow(l, have + n);
    if (rc) return rc;
    lin_wait_other_stream(l, st);
    HIPCK(hipMemcpyAsync(l->dX + (size_t)have * l->D, src, (size_t)n * l->D * 8, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_lin_split, dim3((unsigned)((n + LIN_NT / 64 - 1) / (LIN_NT / 64))), dim3(LIN_NT), 0, st, l->dX + (size_t)have * l->D,
                       l->dXh + (size_t)have * l->Dp, l->dXl + (size_t)have * l->Dp, l->dxn + have, l->d_nmax, l->D, l->Dp, (long long)n);
    HIPCK(hipGetLastError());
    if (l->mirror && have + n <= LIN_SMALL_N) {
        l->X.resize((size_t)(have + n) * l->D);
        double *dst = l->X.data() + (size_t)have * l->D;
        if (on_device) {
            const hipError_t e = hipMemcpyAsync(dst, src, (size_t)n * l->D * 8, hipMemcpyDeviceToHost, st);
            if (e != hipSuccess) {
                l->X.resize((size_t)have * l->D);
                HIPCK(e);
            }
        } else
            memcpy(dst, src, (size_t)n * l->D * 8);
    } else if (l->mirror) {  // past the small path for good: the mirror and the hidden handle are released
        l->mirror = false;
        std::vector<double>().swap(l->X);
        if (l->inner) mmidx_destroy(l->inner);
        l->inner = nullptr;
        l->inner_n = -1;
    }
    if (!on_device || (l->mirror && on_device)) {  // the caller's host array / the mirror's new rows are complete on return
        const hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            if (l->mirror) l->X.resize((size_t)have * l->D);
            HIPCK(e);
        }
    }
    l->n = have + n;
    l->st.uploaded_rows = n;
    return MMIDX_OK;
}

int pow2ceil_host(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

// the exact path for nr queries: rows qidx[r] of dQ (r itself where qidx is null); answers into rows qidx[r] / r of the outputs
int lin_exact(mmidx_linear *l, int k, int64_t nr, const double *dQ, const int32_t *qidx, int32_t *d_iid, double *d_dist, int32_t *d_cnt,
              hipStream_t st) {
    constexpr int QT = 4;
    const int64_t n = l->n;
    const int w = (int)std::min<int64_t>(k, n);
    const int64_t qb = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(nr, 65536), (2ll << 30) / (n * 8)));
    HIPCK(l->ws_dmat.reserve((size_t)qb * n));
    HIPCK(l->ws_cells.reserve((size_t)qb * w));
    for (int64_t r0 = 0; r0 < nr; r0 += qb) {
        const int64_t nb = std::min(qb, nr - r0);
        const double *Qb = qidx ? dQ : dQ + (size_t)r0 * l->D;
        const int32_t *ib = qidx ? qidx + r0 : nullptr;
        hipLaunchKernelGGL(k_lin_exact<QT>, dim3((unsigned)((n + LIN_NT - 1) / LIN_NT), (unsigned)((nb + QT - 1) / QT)), dim3(LIN_NT), 0, st, l->dX, Qb,
                           ib, l->ws_dmat.p, l->D, (long long)n, (int)nb);
        HIPCK(hipGetLastError());
        int rc = mmidx_internal_select_topw(l->ws_dmat.p, (int)n, w, nb, l->ws_cells.p, st);
        if (rc) return rc;
        const size_t o = qidx ? 0 : (size_t)r0;
        hipLaunchKernelGGL(k_lin_place, dim3((unsigned)((nb * w + 255) / 256)), dim3(256), 0, st, l->ws_cells.p, (const double *)nullptr, l->ws_dmat.p, ib,
                           (long long)n, w, k, d_iid + o * k, d_dist + o * k, d_cnt + o, (long long)nb);
        HIPCK(hipGetLastError());
    }
    return MMIDX_OK;
}

// the scan for one round of nq queries (mmidx_linear_scan.h has the stages).  One host synchronisation: the number of queries
// handed back is read after the answer kernel.
int lin_scan_round(mmidx_linear *l, int k, int nq, const double *dQ, int32_t *d_iid, double *d_dist, int32_t *d_cnt, hipStream_t st) {
    const int64_t n = l->n;
    const int D = l->D, Dp = l->Dp, k1 = k + 1;
    const int S = (int)std::min<int64_t>(n, std::max(k1, LIN_SEED_ROWS));
    const int PC = std::min(LIN_POOL_MAX, pow2ceil_host(std::max(4 * k1, 2048)));
    const int64_t cap64 = l->opt_qcap > 0 ? l->opt_qcap : std::min<int64_t>(LIN_REC_MAX, std::max<int64_t>(1 << 16, (int64_t)nq * (8 * k1 + 64)));
    const u32 rec_cap = (u32)cap64;
    HIPCK(l->ws_Qh.reserve((size_t)nq * Dp));
    HIPCK(l->ws_Ql.reserve((size_t)nq * Dp));
    HIPCK(l->ws_qn.reserve((size_t)nq));
    HIPCK(l->ws_a.reserve((size_t)nq));
    HIPCK(l->ws_T.reserve((size_t)nq));
    HIPCK(l->ws_u32.reserve((size_t)nq * 3));
    HIPCK(l->ws_pk.reserve((size_t)nq * PC));
    HIPCK(l->ws_pr.reserve((size_t)nq * PC));
    HIPCK(l->ws_rec.reserve((size_t)rec_cap));
    HIPCK(l->ws_ctr.reserve(4));
    HIPCK(l->ws_redo.reserve((size_t)nq));
    __bf16 *Qh = (__bf16 *)l->ws_Qh.p, *Ql = (__bf16 *)l->ws_Ql.p;
    u32 *pcnt = l->ws_u32.p, *pkept = pcnt + nq, *redo = pkept + nq;
    u64 *surv = l->ws_ctr.p;
    u32 *rec_cnt = (u32 *)(l->ws_ctr.p + 1), *redo_cnt = (u32 *)(l->ws_ctr.p + 2);
    HIPCK(hipMemsetAsync(l->ws_ctr.p, 0, 4 * 8, st));
    hipLaunchKernelGGL(k_lin_split, dim3((unsigned)((nq + LIN_NT / 64 - 1) / (LIN_NT / 64))), dim3(LIN_NT), 0, st, dQ, Qh, Ql, l->ws_qn.p, (u64 *)nullptr, D, Dp,
                       (long long)nq);
    hipLaunchKernelGGL(k_lin_seed, dim3((unsigned)((S + LIN_NT - 1) / LIN_NT), (unsigned)nq), dim3(LIN_NT), 0, st, l->dX, dQ, l->ws_pk.p, l->ws_pr.p, pcnt, pkept,
                       l->ws_T.p, redo, PC, D, S);
    const size_t rlds = (size_t)PC * 12;
    if (rlds > 64 * 1024) HIPCK(hipFuncSetAttribute((const void *)k_lin_reduce, hipFuncAttributeMaxDynamicSharedMemorySize, (int)rlds));
    hipLaunchKernelGGL(k_lin_reduce, dim3((unsigned)nq), dim3(LIN_NT), rlds, st, l->ws_pk.p, l->ws_pr.p, pcnt, pkept, l->ws_T.p, redo, PC, k1);
    HIPCK(hipGetLastError());
    l->st.rows_scanned += S;
    Event ev[3];
    if (l->opt_prof)
        for (int i = 0; i < 3; i++) HIPCK(ev[i].create());
    // Segments grow geometrically: after `done` rows T[q] is the (k + 1)-th of them, so the next g * done rows leave about
    // g (k + 1) survivors per query; g keeps that a quarter of the pool's spare room.  A segment holds fewer than 2^31 / nq
    // rows, so that the record counter cannot wrap even where every pair survives.
    const double g = std::min(3.0, std::max(0.25, (double)(PC - k1) / (4.0 * k1)));
    const unsigned gx = (unsigned)((nq + 127) / 128);
    int rc = MMIDX_OK;
    for (int64_t done = S; done < n && rc == MMIDX_OK;) {
        int64_t len = std::max<int64_t>((int64_t)((double)done * g), 1024);
        len = std::min<int64_t>(len, (1ll << 31) / nq);
        const int64_t r1 = std::min(n, done + len);
        const int64_t ngroups = (r1 - done + 63) / 64;
        const unsigned gy = (unsigned)std::max<int64_t>(1, std::min<int64_t>(ngroups, std::min<int64_t>(65535, 2048 / gx)));
        hipLaunchKernelGGL(k_lin_qprep, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, l->ws_qn.p, l->d_nmax, l->ws_T.p, redo, l->ws_a.p, rec_cnt, Dp, nq);
        if (ev[0]) (void)hipEventRecord(ev[0], st);
        hipLaunchKernelGGL(k_lin_sweep, dim3(gx, gy), dim3(LIN_NT), 0, st, Qh, Ql, l->dXh, l->dXl, l->dxn, l->ws_a.p, l->ws_rec.p, rec_cnt, rec_cap, redo, Dp, nq,
                           (long long)done, (long long)r1);
        if (ev[1]) (void)hipEventRecord(ev[1], st);
        const unsigned vb = (unsigned)std::min<int64_t>(2048, ((int64_t)rec_cap + LIN_NT - 1) / LIN_NT);
        hipLaunchKernelGGL(k_lin_verify, dim3(vb), dim3(LIN_NT), 0, st, l->dX, dQ, l->ws_rec.p, rec_cnt, rec_cap, l->ws_T.p, l->ws_pk.p, l->ws_pr.p, pcnt, surv,
                           PC, D);
        hipLaunchKernelGGL(k_lin_reduce, dim3((unsigned)nq), dim3(LIN_NT), rlds, st, l->ws_pk.p, l->ws_pr.p, pcnt, pkept, l->ws_T.p, redo, PC, k1);
        if (ev[2]) {  // (profiling only: the stage times of this segment are read here)
            (void)hipEventRecord(ev[2], st);
            float a = 0, b = 0;
            if (hipEventSynchronize(ev[2]) == hipSuccess && hipEventElapsedTime(&a, ev[0], ev[1]) == hipSuccess &&
                hipEventElapsedTime(&b, ev[1], ev[2]) == hipSuccess) {
                l->st.scan_ms += a;
                l->st.verify_ms += b;
            }
        }
        if (hipGetLastError() != hipSuccess) rc = mmidx_fail(MMIDX_ERR_HIP, "Linear: a scan kernel could not be launched");
        l->st.segments++;
        l->st.rows_scanned += r1 - done;
        done = r1;
    }
    if (rc) return rc;
    hipLaunchKernelGGL(k_lin_answer, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, l->ws_pk.p, l->ws_pr.p, pcnt, redo, PC, k, d_iid, d_dist, d_cnt,
                       l->ws_redo.p, redo_cnt, nq);
    HIPCK(hipGetLastError());
    u64 ctr[4] = {0, 0, 0, 0};
    HIPCK(hipMemcpyAsync(ctr, l->ws_ctr.p, sizeof(ctr), hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));  // the one read-back of the call: how many queries the exact path has to serve
    const int64_t nredo = (int64_t)(u32)ctr[2];
    l->st.survivors += (int64_t)ctr[0];
    l->st.redo_queries += nredo;
    if (nredo > 0) return lin_exact(l, k, nredo, dQ, l->ws_redo.p, d_iid, d_dist, d_cnt, st);
    return MMIDX_OK;
}

int lin_ensure_inner(mmidx_linear *l) {
    const int64_t n = l->n;
    if (l->inner_n == n) return MMIDX_OK;
    if (l->inner) mmidx_destroy(l->inner);
    l->inner = nullptr;
    l->inner_n = -1;
    int rc = mmidx_create(MMIDX_KIND_IVFPQ, l->D, 1, 2, (int)n, MMIDX_TR_NONE, nullptr, nullptr, l->device, &l->inner);
    if (rc) return rc;
    rc = mmidx_set_coarse(l->inner, l->X.data());
    if (rc) return rc;
    l->inner_n = n;
    return MMIDX_OK;
}

// computeNearestNeighborsInternal for nq queries, everything on the device: [nq][k] ids (-1 beyond the count) and distances
// (+inf beyond it), [nq] counts.  The caller holds l->mu and has reset l->st for the call.
int lin_search_core(mmidx_linear *l, int k, int64_t nq, const double *dQ, int32_t *d_iid, double *d_dist, int32_t *d_cnt, hipStream_t st) {
    const int64_t n = l->n;
    HIPCK(hipSetDevice(l->device));
    lin_wait_other_stream(l, st);
    hipLaunchKernelGGL(k_lin_fill, dim3((unsigned)((nq * std::max(k, 1) + 255) / 256)), dim3(256), 0, st, d_iid, d_dist, d_cnt, (long long)nq, k);
    HIPCK(hipGetLastError());
    if (n == 0) return MMIDX_OK;
    const int w = (int)std::min<int64_t>(k, n);
    if (n <= LIN_SMALL_N && w + 1 <= LIN_SMALL_W1 && l->mirror) {
        l->st.path = 1;
        int rc = lin_ensure_inner(l);
        if (rc) return rc;
        HIPCK(l->ws_cells.reserve((size_t)nq * w));
        HIPCK(l->ws_cd.reserve((size_t)nq * w));
        rc = mmidx_internal_coarse_topw(l->inner, w, nq, dQ, l->ws_cells.p, l->ws_cd.p, st);
        if (rc) return rc;
        hipLaunchKernelGGL(k_lin_place, dim3((unsigned)((nq * w + 255) / 256)), dim3(256), 0, st, l->ws_cells.p, l->ws_cd.p, (const double *)nullptr,
                           (const int32_t *)nullptr, (long long)n, w, k, d_iid, d_dist, d_cnt, (long long)nq);
        HIPCK(hipGetLastError());
        return MMIDX_OK;
    }
    if (l->opt_exact || l->D > LIN_MAX_D || k > LIN_MAX_K) {  // A/B switch, or a shape outside the scan's envelope
        l->st.path = 2;
        return lin_exact(l, k, nq, dQ, nullptr, d_iid, d_dist, d_cnt, st);
    }
    l->st.path = 3;
    const int k1 = k + 1;
    const int PC = std::min(LIN_POOL_MAX, pow2ceil_host(std::max(4 * k1, 2048)));
    // queries per round: the record list (8 (k + 1) + 64 per query) within LIN_REC_MAX, the pools within 512 MiB
    int64_t qb = std::min<int64_t>(MMIDX_COMB_MAX_Q, std::min<int64_t>(LIN_REC_MAX / (8 * k1 + 64), (512ll << 20) / ((int64_t)PC * 12)));
    qb = std::max<int64_t>(qb, 128);
    for (int64_t q0 = 0; q0 < nq; q0 += qb) {
        const int nb = (int)std::min(qb, nq - q0);
        int rc = lin_scan_round(l, k, nb, dQ + (size_t)q0 * l->D, d_iid + (size_t)q0 * k, d_dist + (size_t)q0 * k, d_cnt + q0, st);
        if (rc) return rc;
    }
    return MMIDX_OK;
}

// host-pointer queries through the device core, in rounds of MMIDX_COMB_MAX_Q; results land in [nq][k] host arrays
int lin_search_host(mmidx_linear *l, int k, int64_t nq, const double *Q, const int32_t *ids, int32_t *iid, double *dist, int32_t *cnt) {
    hipStream_t st = l->stream;
    HIPCK(hipSetDevice(l->device));
    const int64_t qb = std::min<int64_t>(nq, MMIDX_COMB_MAX_Q);
    HIPCK(l->ws_Q.reserve((size_t)qb * l->D));
    HIPCK(l->ws_i.reserve((size_t)qb * k));
    HIPCK(l->ws_d.reserve((size_t)qb * k));
    HIPCK(l->ws_c.reserve((size_t)qb));
    if (ids) HIPCK(l->ws_ids.reserve((size_t)qb));
    for (int64_t q0 = 0; q0 < nq; q0 += qb) {
        const int64_t nb = std::min(qb, nq - q0);
        lin_wait_other_stream(l, st);
        if (ids) {  // the stored vectors are the queries (Linear.java:181-184): gathered on the device
            HIPCK(hipMemcpyAsync(l->ws_ids.p, ids + q0, (size_t)nb * 4, hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_lin_gather_rows, dim3((unsigned)((nb * l->D + 255) / 256)), dim3(256), 0, st, l->dX, l->ws_ids.p, l->ws_Q.p, l->D, (long long)nb);
            HIPCK(hipGetLastError());
        } else
            HIPCK(hipMemcpyAsync(l->ws_Q.p, Q + (size_t)q0 * l->D, (size_t)nb * l->D * 8, hipMemcpyHostToDevice, st));
        int rc = lin_search_core(l, k, nb, l->ws_Q.p, l->ws_i.p, l->ws_d.p, l->ws_c.p, st);
        if (rc) return rc;
        HIPCK(hipMemcpyAsync(iid + (size_t)q0 * k, l->ws_i.p, (size_t)nb * k * 4, hipMemcpyDeviceToHost, st));
        HIPCK(hipMemcpyAsync(dist + (size_t)q0 * k, l->ws_d.p, (size_t)nb * k * 8, hipMemcpyDeviceToHost, st));
        HIPCK(hipMemcpyAsync(cnt + q0, l->ws_c.p, (size_t)nb * 4, hipMemcpyDeviceToHost, st));
        HIPCK(hipStreamSynchronize(st));
    }
    return MMIDX_OK;
}

}  // namespace

extern "C" {

int mmidx_linear_create(int D, int64_t capacity, int device, mmidx_linear **out) {
    if (!out) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null out pointer");
    *out = nullptr;
    if (D < 1 || capacity < 0) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "bad vector length / capacity");
    const int ndev = mmidx_device_count();
    if (ndev < 1) return mmidx_fail(MMIDX_ERR_NO_DEVICE, "no HIP device: libmmidx_hip has no CPU fallback");
    if (device < 0 || device >= ndev) return mmidx_fail(MMIDX_ERR_NO_DEVICE, "device %d outside 0..%d", device, ndev - 1);
    HIPCK(hipSetDevice(device));
    std::unique_ptr<mmidx_linear> l(new mmidx_linear());
    l->D = D;
    l->Dp = (D + 31) / 32 * 32;  // the matrix instruction's depth
    l->device = device;
    l->capacity = capacity;
    const hipError_t e = l->stream.create();
    if (e != hipSuccess) return mmidx_fail(MMIDX_ERR_HIP, "Linear: no stream on device %d: %s", device, hipGetErrorString(e));
    *out = l.release();
    return MMIDX_OK;
}

int mmidx_linear_destroy(mmidx_linear *l) {
    if (!l) return MMIDX_OK;
    (void)hipSetDevice(l->device);
    if (l->last_stream_valid && hipStreamSynchronize(l->last_stream) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipDeviceSynchronize();
    }
    if (l->inner) mmidx_destroy(l->inner);
    delete l;
    return MMIDX_OK;
}

int mmidx_linear_add(mmidx_linear *l, int64_t n, const double *X) {  // indexVectorInternal, Linear.java:111-122
    if (!l || n < 0 || (n > 0 && !X)) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null argument");
    std::lock_guard<std::mutex> lk(l->mu);
    return lin_append(l, n, X, false, l->stream);
}

int mmidx_linear_add_device(mmidx_linear *l, int64_t n, const double *dX, void *stream) {
    if (!l || n < 0 || (n > 0 && !dX)) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null argument");
    std::lock_guard<std::mutex> lk(l->mu);
    return lin_append(l, n, dX, true, (hipStream_t)stream);
}

int mmidx_linear_get_dim(const mmidx_linear *l, int *D_out) {
    if (!l || !D_out) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null argument");
    *D_out = l->D;
    return MMIDX_OK;
}

int mmidx_linear_size(const mmidx_linear *l, int64_t *n_out) {
    if (!l || !n_out) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null argument");
    std::lock_guard<std::mutex> lk(l->mu);
    *n_out = l->n;
    return MMIDX_OK;
}

int mmidx_linear_get_vector(const mmidx_linear *cl, int64_t iid, double *out) {  // Linear.getVector, Linear.java:253-263
    if (!cl || !out) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null argument");
    mmidx_linear *l = const_cast<mmidx_linear *>(cl);
    std::lock_guard<std::mutex> lk(l->mu);
    if (iid < 0 || iid >= l->n) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "Internal id %lld is out of range!", (long long)iid);
    if (l->mirror) {
        memcpy(out, l->X.data() + (size_t)iid * l->D, (size_t)l->D * 8);
        return MMIDX_OK;
    }
    HIPCK(hipSetDevice(l->device));
    lin_wait_other_stream(l, l->stream);
    HIPCK(hipMemcpyAsync(out, l->dX + (size_t)iid * l->D, (size_t)l->D * 8, hipMemcpyDeviceToHost, l->stream));
    HIPCK(hipStreamSynchronize(l->stream));
    return MMIDX_OK;
}

int mmidx_linear_copy_rows_device(mmidx_linear *l, int64_t iid0, int64_t n, double *d_out, void *stream) {
    if (!l || n < 0 || (n > 0 && !d_out)) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null argument");
    std::lock_guard<std::mutex> lk(l->mu);
    if (iid0 < 0 || iid0 + n > l->n) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "Internal id %lld is out of range!", (long long)(iid0 < 0 ? iid0 : iid0 + n - 1));
    if (n == 0) return MMIDX_OK;
    HIPCK(hipSetDevice(l->device));
    lin_wait_other_stream(l, (hipStream_t)stream);
    HIPCK(hipMemcpyAsync(d_out, l->dX + (size_t)iid0 * l->D, (size_t)n * l->D * 8, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return MMIDX_OK;
}

int mmidx_linear_set_option(mmidx_linear *l, const char *name, int value) {
    if (!l || !name) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null argument");
    const std::string n(name);
    std::lock_guard<std::mutex> lk(l->mu);
    if (n == "exact") {
        l->opt_exact = value != 0;
        return MMIDX_OK;
    }
    if (n == "mfma_qcap") {
        if (value < 0) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "mfma_qcap = %d must be >= 0", value);
        l->opt_qcap = value;
        return MMIDX_OK;
    }
    if (n == "debug_sync") {
        l->opt_prof = value != 0;
        return MMIDX_OK;
    }
    return mmidx_fail(MMIDX_ERR_INVALID_ARG, "unknown Linear option '%s'", name);
}

int mmidx_linear_get_stats(mmidx_linear *l, mmidx_linear_stats *out) {
    if (!l || !out) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null argument");
    std::lock_guard<std::mutex> lk(l->mu);
    out->path = l->st.path;
    out->segments = l->st.segments;
    out->rows_scanned = l->st.rows_scanned;
    out->survivors = l->st.survivors;
    out->redo_queries = l->st.redo_queries;
    out->uploaded_rows = l->st.uploaded_rows;
    out->scan_ms = l->st.scan_ms;
    out->verify_ms = l->st.verify_ms;
    return MMIDX_OK;
}

// the figures of a search are those of the last call: reset before it is served
static void lin_reset_search_stats(mmidx_linear *l) {
    const int64_t up = l->st.uploaded_rows;
    l->st = LinStatsAcc();
    l->st.uploaded_rows = up;
}

// serves batch[0..nb) (same k) as one search over the concatenated queries; the caller holds l->mu
static int linear_search_batch(mmidx_linear *l, SearchReq *const *batch, size_t nb) {
    const int k = batch[0]->k;
    int64_t nq = 0;
    for (size_t b = 0; b < nb; b++) nq += batch[b]->nq;
    lin_reset_search_stats(l);
    if (nb == 1) return lin_search_host(l, k, nq, batch[0]->Q, nullptr, batch[0]->iid, batch[0]->dist, batch[0]->cnt);
    l->cat_Q.resize((size_t)nq * l->D);
    size_t off = 0;
    for (size_t b = 0; b < nb; b++) {
        memcpy(l->cat_Q.data() + off, batch[b]->Q, (size_t)batch[b]->nq * l->D * 8);
        off += (size_t)batch[b]->nq * l->D;
    }
    std::vector<int32_t> hi((size_t)nq * k), hc((size_t)nq);
    std::vector<double> hd((size_t)nq * k);
    int rc = lin_search_host(l, k, nq, l->cat_Q.data(), nullptr, hi.data(), hd.data(), hc.data());
    if (rc) return rc;
    size_t q = 0;
    for (size_t b = 0; b < nb; b++) {
        SearchReq *r = batch[b];
        memcpy(r->iid, hi.data() + q * k, (size_t)r->nq * k * 4);
        memcpy(r->dist, hd.data() + q * k, (size_t)r->nq * k * 8);
        memcpy(r->cnt, hc.data() + q, (size_t)r->nq * 4);
        q += (size_t)r->nq;
    }
    return MMIDX_OK;
}

int mmidx_linear_search_device(mmidx_linear *l, int k, int64_t nq, const double *dQ, int32_t *d_iid_out, double *d_dist_out, int32_t *d_count_out,
                               void *stream) {
    if (!l) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null handle");
    if (k < 1) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "k must be positive (got %d)", k);
    if (nq < 0 || (nq > 0 && (!dQ || !d_iid_out || !d_dist_out || !d_count_out))) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null argument");
    if (nq == 0) return MMIDX_OK;
    std::lock_guard<std::mutex> lk(l->mu);
    lin_reset_search_stats(l);
    return lin_search_core(l, k, nq, dQ, d_iid_out, d_dist_out, d_count_out, (hipStream_t)stream);
}

int mmidx_linear_search_ids(mmidx_linear *l, int k, int64_t nq, const int32_t *iids, int32_t *iid_out, double *dist_out, int32_t *count_out) {
    if (!l) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null handle");
    if (k < 1) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "k must be positive (got %d)", k);
    if (nq < 0 || (nq > 0 && (!iids || !iid_out || !dist_out || !count_out))) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null argument");
    if (nq == 0) return MMIDX_OK;
    std::lock_guard<std::mutex> lk(l->mu);
    for (int64_t q = 0; q < nq; q++)  // (before any device call)
        if (iids[q] < 0 || iids[q] >= l->n) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "Internal id %lld is out of range!", (long long)iids[q]);
    lin_reset_search_stats(l);
    return lin_search_host(l, k, nq, nullptr, iids, iid_out, dist_out, count_out);
}

int mmidx_linear_search(mmidx_linear *l, int k, int64_t nq, const double *Q, int32_t *iid_out, double *dist_out, int32_t *count_out) {
    if (!l) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null handle");
    if (k < 1) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "k must be positive (got %d)", k);
    if (nq < 0 || (nq > 0 && (!Q || !iid_out || !dist_out || !count_out))) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null argument");
    if (nq == 0) return MMIDX_OK;
    SearchReq me;
    me.k = k;
    me.nq = nq;
    me.Q = Q;
    me.iid = iid_out;
    me.dist = dist_out;
    me.cnt = count_out;
    return combiner_submit(l->comb, me, MMIDX_COMB_MAX_Q, [l](SearchReq *const *batch, size_t nb) {
        std::lock_guard<std::mutex> lk(l->mu);
        return linear_search_batch(l, batch, nb);
    });
}

// ---- the rows, for the exact re-ranking of a PQ / IVFPQ answer (mmidx_search_refine* in mmidx_api.hip; mmidx_host.h has the contract) ----
void mmidx_internal_linear_dims(const mmidx_linear *l, int *D_out, int *device_out) {
    *D_out = l->D;
    *device_out = l->device;
}

// Lock order: the caller already holds its index handle's search_mu; l->mu is taken second, never the other way round.
int mmidx_internal_linear_rows_acquire(mmidx_linear *l, hipStream_t st, MmidxLinearRows *out) {
    l->mu.lock();
    lin_wait_other_stream(l, st);
    out->dX = l->n > 0 ? l->dX : nullptr;
    out->n = l->n;
    out->D = l->D;
    out->device = l->device;
    return MMIDX_OK;
}

void mmidx_internal_linear_rows_release(mmidx_linear *l) { l->mu.unlock(); }

// ---- the walk into other indexes (mmidx_linear_reindex in mmidx_reindex.hip; mmidx_host.h has the lock order) ----
void mmidx_internal_linear_lock(mmidx_linear *l, MmidxLinearInfo *out) {
    l->mu.lock();
    out->dX = l->n > 0 ? l->dX : nullptr;
    out->n = l->n;
    out->capacity = l->capacity;
    out->D = l->D;
    out->device = l->device;
    out->stream = l->stream;
}

void mmidx_internal_linear_unlock(mmidx_linear *l, bool settle) {
    if (settle) l->last_stream_valid = false;
    l->mu.unlock();
}

void mmidx_internal_linear_order(mmidx_linear *l, hipStream_t st) { lin_wait_other_stream(l, st); }

int mmidx_internal_linear_append_locked(mmidx_linear *l, int64_t n, const double *dX, hipStream_t st) { return lin_append(l, n, dX, true, st); }

}  // extern "C"
