// mmidx_linear.hip -- Linear: exhaustive exact search (J/datastructures/Linear.java).  No kernels of its own: the indexed
// vectors are the "centroids" of a hidden index handle and a search is that handle's coarse stage (mmidx_internal_coarse_topw).
#include "mmidx_host.h"

#include <algorithm>
#include <cstring>
#include <limits>
#include <mutex>
#include <vector>

// ---- Linear (exhaustive exact search, J/datastructures/Linear.java) -----------------------------------------------
// computeNearestNeighborsInternal (Linear.java:138-163) offers (i, sum_j (q_j - x_ij)^2) for every vector in index order
// to a bounded queue of size k: exactly what computeNearestCoarseIndices does with the coarse centroids and w, so the
// indexed vectors are handed to the coarse stage as "centroids" (certified bf16 / fp32 matrix-core filter + exact fp64 for
// the few candidates while n <= 16384, the plain exact kernels beyond that); (q - x)^2 and (x - q)^2 are the same bits.

extern "C" {

struct mmidx_linear {
    std::mutex mu;
    int D = 0, device = 0;
    int64_t capacity = 0;
    std::vector<double> X;  // [n][D]; Linear keeps its vectors in memory too (TDoubleArrayList, Linear.java:45)
    mmidx_index *inner = nullptr;
    int64_t inner_n = -1;   // number of vectors the inner handle was built for
    hipStream_t stream = nullptr;
    DevBuf<double> ws_Q, ws_d;
    DevBuf<int32_t> ws_i;
    Combiner comb;              // concurrent one-query callers are served together, as in mmidx_search
    std::vector<double> cat_Q;  // their queries, concatenated
};

int mmidx_linear_create(int D, int64_t capacity, int device, mmidx_linear **out) {
    if (!out) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null out pointer");
    *out = nullptr;
    if (D < 1 || capacity < 0) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "bad vector length / capacity");
    const int ndev = mmidx_device_count();
    if (ndev < 1) return mmidx_fail(MMIDX_ERR_NO_DEVICE, "no HIP device: libmmidx_hip has no CPU fallback");
    if (device < 0 || device >= ndev) return mmidx_fail(MMIDX_ERR_NO_DEVICE, "device %d outside 0..%d", device, ndev - 1);
    HIPCK(hipSetDevice(device));
    mmidx_linear *l = new mmidx_linear();
    l->D = D;
    l->device = device;
    l->capacity = capacity;
    const hipError_t e = hipStreamCreateWithFlags(&l->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete l;
        return mmidx_fail(MMIDX_ERR_HIP, "Linear: no stream on device %d: %s", device, hipGetErrorString(e));
    }
    *out = l;
    return MMIDX_OK;
}

int mmidx_linear_destroy(mmidx_linear *l) {
    if (!l) return MMIDX_OK;
    (void)hipSetDevice(l->device);
    if (l->inner) mmidx_destroy(l->inner);
    l->ws_Q.release();
    l->ws_d.release();
    l->ws_i.release();
    if (l->stream) (void)hipStreamDestroy(l->stream);
    delete l;
    return MMIDX_OK;
}

int mmidx_linear_add(mmidx_linear *l, int64_t n, const double *X) {  // indexVectorInternal, Linear.java:111-122
    if (!l || n < 0 || (n > 0 && !X)) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null argument");
    std::lock_guard<std::mutex> lk(l->mu);
    const int64_t have = (int64_t)(l->X.size() / (size_t)l->D);
    if (l->capacity > 0 && have + n > l->capacity) return mmidx_fail(MMIDX_ERR_CAPACITY, "Maximum index capacity reached, no more vectors can be indexed!");
    l->X.insert(l->X.end(), X, X + (size_t)n * l->D);
    return MMIDX_OK;
}

int mmidx_linear_get_dim(const mmidx_linear *l, int *D_out) {
    if (!l || !D_out) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null argument");
    *D_out = l->D;
    return MMIDX_OK;
}

int mmidx_linear_size(const mmidx_linear *l, int64_t *n_out) {
    if (!l || !n_out) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null argument");
    *n_out = (int64_t)(l->X.size() / (size_t)l->D);
    return MMIDX_OK;
}

int mmidx_linear_get_vector(const mmidx_linear *l, int64_t iid, double *out) {  // Linear.getVector, Linear.java:253-263
    if (!l || !out) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null argument");
    const int64_t have = (int64_t)(l->X.size() / (size_t)l->D);
    if (iid < 0 || iid >= have) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "Internal id %lld is out of range!", (long long)iid);
    memcpy(out, l->X.data() + (size_t)iid * l->D, (size_t)l->D * 8);
    return MMIDX_OK;
}

// serves batch[0..nb) (same k) as one search over the concatenated queries; the caller holds l->mu
static int linear_search_batch(mmidx_linear *l, SearchReq *const *batch, size_t nb) {
    const int k = batch[0]->k;
    const int64_t n = (int64_t)(l->X.size() / (size_t)l->D);
    if (n > 0x7fffffff) return mmidx_fail(MMIDX_ERR_CAPACITY, "internal ids are 32-bit, as in the reference");
    int64_t nq = 0;
    for (size_t b = 0; b < nb; b++) {
        SearchReq *r = batch[b];
        for (int64_t i = 0; i < r->nq * k; i++) {
            r->iid[i] = -1;
            r->dist[i] = std::numeric_limits<double>::infinity();
        }
        for (int64_t q = 0; q < r->nq; q++) r->cnt[q] = 0;
        nq += r->nq;
    }
    if (nq == 0 || n == 0) return MMIDX_OK;
    const double *Q = batch[0]->Q;
    if (nb > 1) {
        l->cat_Q.resize((size_t)nq * l->D);
        size_t off = 0;
        for (size_t b = 0; b < nb; b++) {
            memcpy(l->cat_Q.data() + off, batch[b]->Q, (size_t)batch[b]->nq * l->D * 8);
            off += (size_t)batch[b]->nq * l->D;
        }
        Q = l->cat_Q.data();
    }
    HIPCK(hipSetDevice(l->device));
    if (l->inner_n != n) {
        if (l->inner) mmidx_destroy(l->inner);
        l->inner = nullptr;
        l->inner_n = -1;
        int rc = mmidx_create(MMIDX_KIND_IVFPQ, l->D, 1, 2, (int)n, MMIDX_TR_NONE, nullptr, nullptr, l->device, &l->inner);
        if (rc) return rc;
        rc = mmidx_set_coarse(l->inner, l->X.data());
        if (rc) return rc;
        l->inner_n = n;
    }
    const int w = (int)std::min<int64_t>(k, n);
    hipStream_t st = l->stream;
    const int64_t qb = std::max<int64_t>(1, std::min<int64_t>(nq, (2ll << 30) / ((int64_t)n * 8)));
    HIPCK(l->ws_Q.reserve((size_t)qb * l->D));
    HIPCK(l->ws_i.reserve((size_t)qb * w));
    HIPCK(l->ws_d.reserve((size_t)qb * w));
    std::vector<int32_t> hi((size_t)qb * w);
    std::vector<double> hd((size_t)qb * w);
    size_t cur = 0;        // request that holds query q0 + q, and that query's position in it
    int64_t cur_q = 0;
    for (int64_t q0 = 0; q0 < nq; q0 += qb) {
        const int64_t nbq = std::min(qb, nq - q0);
        HIPCK(hipMemcpyAsync(l->ws_Q.p, Q + (size_t)q0 * l->D, (size_t)nbq * l->D * 8, hipMemcpyHostToDevice, st));
        int rc = mmidx_internal_coarse_topw(l->inner, w, nbq, l->ws_Q.p, l->ws_i.p, l->ws_d.p, st);
        if (rc) return rc;
        HIPCK(hipMemcpyAsync(hi.data(), l->ws_i.p, (size_t)nbq * w * 4, hipMemcpyDeviceToHost, st));
        HIPCK(hipMemcpyAsync(hd.data(), l->ws_d.p, (size_t)nbq * w * 8, hipMemcpyDeviceToHost, st));
        HIPCK(hipStreamSynchronize(st));
        for (int64_t q = 0; q < nbq; q++) {
            while (cur_q >= batch[cur]->nq) {
                cur++;
                cur_q = 0;
            }
            SearchReq *r = batch[cur];
            for (int t = 0; t < w; t++) {
                r->iid[(size_t)cur_q * k + t] = hi[(size_t)q * w + t];
                r->dist[(size_t)cur_q * k + t] = hd[(size_t)q * w + t];
            }
            r->cnt[cur_q] = w;
            cur_q++;
        }
    }
    return MMIDX_OK;
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

}  // extern "C"
