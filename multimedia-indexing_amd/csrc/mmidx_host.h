// mmidx_host.h -- host plumbing shared by every unit of libmmidx_hip.so: the error text, the HIP-check macro, device buffers,
// the caller combiner, the tile constants host code sizes launches with, and the hidden functions one unit calls in another.
//
// Host only: no __global__ is defined here.  A kernel header defines plain external-linkage kernels, so it is included by
// exactly one .hip; what another unit needs of it goes through an mmidx_internal_* function declared at the end of this file.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/mmidx.h"

#define MMIDX_HIDDEN __attribute__((visibility("hidden")))

// records the calling thread's error text (mmidx_last_error) and returns `code`; defined in mmidx_api.hip
MMIDX_HIDDEN int mmidx_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
// empties that text: for a call that recovered from a failure of its own making
MMIDX_HIDDEN void mmidx_clear_error();

#define HIPCK(expr)                                                                                \
    do {                                                                                           \
        hipError_t e__ = (expr);                                                                   \
        if (e__ != hipSuccess)                                                                     \
            return mmidx_fail(MMIDX_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), \
                              __FILE__, __LINE__);                                                 \
    } while (0)

// (the types below stay inside the library: hidden, so that their instantiations add nothing to the exported symbols)
#pragma GCC visibility push(hidden)

// ---- owners: every device block, pinned block, event and stream of the library is a field or a local of one of these types.  Each
// is movable and not copyable, reads as the plain handle it holds, and its destructor frees that handle and nothing else: a handle
// struct needs no release list (members go in reverse order of declaration), and a return between an allocation and its use leaks nothing.
template <typename H, typename A, hipError_t (*Free)(A)>
struct Owned {
    H p{};
    Owned() = default;
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    Owned(Owned &&o) noexcept : p(o.p) { o.p = H{}; }
    Owned &operator=(Owned &&o) noexcept {
        if (this != &o) {
            release();
            p = o.p;
            o.p = H{};
        }
        return *this;
    }
    ~Owned() { release(); }
    void release() {
        if (p) (void)Free(p);
        p = H{};
    }
    operator H() const { return p; }
};

template <typename T>
constexpr size_t elem_bytes = sizeof(T);
template <>
inline constexpr size_t elem_bytes<void> = 1;  // an untyped block is sized in bytes

// a device array of exact size: a handle's persistent table, or the array of one call
template <typename T>
struct DevPtr : Owned<T *, void *, hipFree> {
    hipError_t alloc(size_t n) {  // frees the block held before
        this->release();
        return hipMalloc((void **)&this->p, std::max<size_t>(n, 1) * elem_bytes<T>);
    }
    hipError_t ensure(size_t n) { return this->p ? hipSuccess : alloc(n); }  // allocate if empty
    template <typename U>
    explicit operator U *() const {  // (const unsigned char *)h->d_codes, (__bf16 *)h->d_Ch: the casts a raw pointer allowed
        return (U *)this->p;
    }
};

// a workspace that grows and is released by its owner
template <typename T>
struct DevBuf : Owned<T *, void *, hipFree> {
    size_t cap = 0;  // elements
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : Owned<T *, void *, hipFree>(std::move(o)), cap(o.cap) { o.cap = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        Owned<T *, void *, hipFree>::operator=(std::move(o));
        cap = o.cap;
        o.cap = 0;
        return *this;
    }
    hipError_t reserve(size_t n) {
        if (n <= cap) return hipSuccess;
        release();
        size_t want = n + n / 8 + 64;
        hipError_t e = hipMalloc((void **)&this->p, want * sizeof(T));
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() {
        Owned<T *, void *, hipFree>::release();
        cap = 0;
    }
};
static_assert(!std::is_copy_constructible<DevBuf<int>>::value && !std::is_copy_constructible<DevPtr<int>>::value, "owners are not copied");

// pinned host memory
template <typename T>
struct PinBuf : Owned<T *, void *, hipHostFree> {
    hipError_t alloc(size_t n, unsigned flags = hipHostMallocDefault) {
        this->release();
        return hipHostMalloc((void **)&this->p, std::max<size_t>(n, 1) * elem_bytes<T>, flags);
    }
};

struct Event : Owned<hipEvent_t, hipEvent_t, hipEventDestroy> {
    hipError_t create(unsigned flags = hipEventDefault) {
        release();
        return hipEventCreateWithFlags(&p, flags);
    }
};
static_assert(sizeof(Event) == sizeof(hipEvent_t), "a pool of Event is read as an array of hipEvent_t (take_events)");

struct Stream : Owned<hipStream_t, hipStream_t, hipStreamDestroy> {
    hipError_t create(unsigned flags = hipStreamNonBlocking) {
        release();
        return hipStreamCreateWithFlags(&p, flags);
    }
};

#define MMIDX_COMB_MAX_Q 4096   // queries per combined batch; larger requests run alone with direct copies

// one host-pointer search call waiting to be served (see mmidx_search)
struct SearchReq {
    int k;
    int64_t nq;
    const double *Q;
    int32_t *iid;
    double *dist;
    int32_t *cnt;
    int rc = MMIDX_OK;
    bool done = false;
    std::string err;
    std::condition_variable cv;  // its caller sleeps here: woken when served, or when it is the oldest and nobody leads
};

// Concurrent callers of a host-pointer search are combined into one device batch (the reference's API is one query
// per call, from many reader threads): requests queue here, one caller at a time leads and serves the queue.
struct Combiner {
    std::mutex mu;
    std::deque<SearchReq *> q;
    bool busy = false;
    int enabled = 1;  // 0 = every call runs on its own
};

// Queues `me`, leads batches (serve(requests, count) -> status) until `me` has been served, returns its status.
template <class Serve>
int combiner_submit(Combiner &c, SearchReq &me, int64_t max_q, Serve serve) {
    std::unique_lock<std::mutex> lk(c.mu);
    c.q.push_back(&me);
    while (!me.done) {
        if (c.busy) {
            me.cv.wait(lk);
            continue;
        }
        // lead: the oldest request and everything behind it with the same k, up to the batch limit
        c.busy = true;
        std::vector<SearchReq *> batch;
        {
            SearchReq *first = c.q.front();
            c.q.pop_front();
            batch.push_back(first);
            int64_t tot = first->nq;
            if (c.enabled && tot <= max_q) {
                for (auto it = c.q.begin(); it != c.q.end();) {
                    if ((*it)->k == first->k && tot + (*it)->nq <= max_q) {
                        tot += (*it)->nq;
                        batch.push_back(*it);
                        it = c.q.erase(it);
                    } else {
                        ++it;
                    }
                }
            }
        }
        lk.unlock();
        const int brc = serve(batch.data(), batch.size());
        lk.lock();
        for (SearchReq *r : batch) {
            r->rc = brc;
            if (brc && r != &me) r->err = mmidx_last_error();  // the message lives in the leader's thread
            r->done = true;
            if (r != &me) r->cv.notify_one();
        }
        c.busy = false;
        // hand the lead to the oldest waiting caller (only that thread is woken); if this call is still unserved
        // -- the batch was another k's -- it leads again itself
        if (me.done && !c.q.empty()) c.q.front()->cv.notify_one();
    }
    lk.unlock();
    if (me.rc && !me.err.empty()) return mmidx_fail(me.rc, "%s", me.err.c_str());
    return me.rc;
}

#pragma GCC visibility pop

// tiles of the bf16-split coarse kernels (K1e, the encoder's argmin, K8''): host code of more than one unit sizes launches by them
#define G16_BQ 128     // queries per block (32 per wave)
#define G16_BC 128     // centroids per tile
#define G16_KC 128     // k per LDS tile
#define G16_STRIDE 272 // bytes per LDS row: 256 + 16 (conflict-free 16-byte fragment reads)
// K1e'' (k_coarse_gmin16_grp: two staggered wave groups, Dp == 128)
#define G16G_BLOCK 512       // threads per block: 8 waves, group = wave >> 2
#define G16G_BQ 256          // queries per block (32 per wave)
#define G16G_RING 4          // half-tile buffers of 32 KiB
#define G16G_NORM_TILES 64   // centroid tiles whose norms a block keeps in LDS beside the ring (4 x 32 KiB + 32 KiB = the CU's 160 KiB)

// The auto rule of option "coarse_screen" (the idiom of K3s's pre_skip): the screen runs, unless the pinned word says that the last
// screened call handed on more than a quarter of its queries -- then seven calls go without it and the next one probes again.  A
// stale word costs speed, never results.  (tests/coarse_screen_model.py restates step().)
struct ScreenAuto {
    int skip = 0;        // calls the screen still sits out
    bool fresh = false;  // the pinned word describes a screened call that has not been judged yet ...
    long long nq = 0;    // ... of this many queries
    // handed: the pinned word as it reads now; returns whether this call, of nq_now queries, runs the screen
    bool step(const long long handed, const long long nq_now) {
        if (skip > 0) {
            skip--;
            return false;
        }
        if (fresh) {
            fresh = false;
            if (handed * 4 > nq) {
                skip = 6;  // (this call is the first of the seven)
                return false;
            }
        }
        fresh = true;
        nq = nq_now;
        return true;
    }
};

// ---- calls across units (hidden: none of these is exported) ----------------------------------------------------------------
extern "C" {
// mmidx_api.hip: what K8'' reads of an index handle's coarse quantizer (bf16 head / tail copies padded to Cp x Dp, |c|^2, maxima)
struct MmidxCoarseTables {
    const double *coarseT;
    const unsigned short *Ch, *Cl;
    const double *cn_pad;
    double cnorm_max, cn_max;
    int Cp, Dp;
};
MMIDX_HIDDEN int mmidx_internal_coarse_tables(const mmidx_index *h, MmidxCoarseTables *out);
// mmidx_api.hip: the w nearest centroids of nq queries on device pointers, in rounds of at most 2 GiB of distances: cells
// [nq][w] and, where asked for, their exact distances.  Sets the handle's w.  mmidx_coarse_device and Linear go through it.
MMIDX_HIDDEN int mmidx_internal_coarse_topw(mmidx_index *h, int w, int64_t nq, const double *dQ, int32_t *d_cells, double *d_dist_or_null,
                                            hipStream_t st);
// mmidx_api.hip: K1b alone -- the w nearest columns of every row of a device distance matrix d_dist[nq][C], bounded-queue order
// and ties, cells [nq][w].  Linear's exact path goes through it.
MMIDX_HIDDEN int mmidx_internal_select_topw(const double *d_dist, int C, int w, int64_t nq, int32_t *d_cells, hipStream_t st);
// mmidx_frontend.hip: K7 on plain device pointers, Y[n][nc] = (X[n][ss] - mu[ss]) Vt[nc][ss]^T
MMIDX_HIDDEN int mmidx_internal_gemm_nt(const double *X, const double *mu, const double *Vt, double *Y, long long n, int nc, int ss,
                                        void *stream);
// mmidx_decode.hip: K10 on plain device pointers -- n records (by internal id) back to the vectors the index holds for them, dX[n][D];
// d_found[n] (may be null) = 1 for a stored id, 0 for an unknown one, whose row is zeros
struct MmidxDecodeArgs {
    int64_t n;
    const int32_t *d_iids;
    const int32_t *d_inv;   // iid -> position, -1 = absent
    int64_t inv_size;
    const int64_t *d_off;   // [nlists + 1]
    int nlists;
    int64_t n_csr;
    const void *d_codes;
    int code_bytes;
    const double *d_pq, *d_coarse;
    const int32_t *d_perm;
    const double *d_rotT;   // rotT[j][i] = R[i][j]
    int D, m, ks, dsub, transform, ivf;
    double *dX;
    int32_t *d_found;
};
MMIDX_HIDDEN int mmidx_internal_decode_records(const MmidxDecodeArgs *a, hipStream_t st);
// ... d_found[n] alone; d_dst[j][i] = d_src[i][j] of a D x D matrix; and the rows of an id query whose id is unknown (count -1, ids -1, +inf)
MMIDX_HIDDEN int mmidx_internal_ids_found(const int32_t *d_iids, int64_t n, const int32_t *d_inv, int64_t inv_size, int64_t n_csr, int32_t *d_found,
                                          hipStream_t st);
MMIDX_HIDDEN int mmidx_internal_transpose_square(const double *d_src, double *d_dst, int D, hipStream_t st);
MMIDX_HIDDEN int mmidx_internal_mark_unknown_rows(const int32_t *d_found, int64_t nq, int k, int32_t *d_iid, double *d_dist, int32_t *d_cnt,
                                                  hipStream_t st);
// mmidx_remove.hip: K13 on plain device pointers (mmidx_remove.h) -- the stable compaction of the list-major arrays behind mmidx_remove.
// _ws: the sizes of the three workspaces for n records and a position table of inv_size entries.  _plan: marks the requested ids,
// writes the keep words, the tile prefixes and the nlists + 1 new list offsets (d_off_new[nlists] = the survivors), and d_found where
// asked for; nothing of the index is written.  _compact: the survivors' ids and records into arrays the caller sized from d_off_new.
struct MmidxRemoveArgs {
    const int32_t *d_ids;   // [n] list-major
    const void *d_codes;    // [n][rec_bytes]
    int64_t n;
    int rec_bytes;          // m * code_bytes
    const int64_t *d_off;   // [nlists + 1]
    int nlists;
    const int32_t *d_req;   // [nreq] the ids to take out
    int64_t nreq;
    const int32_t *d_inv;   // iid -> position, -1 = absent
    int64_t inv_size;
    int32_t *d_found;       // [nreq] or null
    unsigned *d_bits;       // [bits_words] one bit per iid
    void *d_keep;           // [keep_words] 64-bit words, bit l of word w = record 64 w + l stays
    unsigned *d_tile_cnt;   // [ntiles]
    int64_t *d_pre;         // [ntiles + 1]
    int64_t *d_off_new;     // [nlists + 1]
};
MMIDX_HIDDEN void mmidx_internal_remove_ws(int64_t n, int64_t inv_size, size_t *bits_words, size_t *keep_words, size_t *ntiles);
MMIDX_HIDDEN int mmidx_internal_remove_plan(const MmidxRemoveArgs *a, hipStream_t st);
MMIDX_HIDDEN int mmidx_internal_remove_compact(const MmidxRemoveArgs *a, int32_t *d_ids_new, void *d_codes_new, hipStream_t st);
// mmidx_linear.hip: what the exact re-ranking (mmidx_search_refine*) reads of a Linear handle -- the fp64 rows in arrival order
// (row iid = the vector of internal id iid, IndexTransformation.java:113-122), their number, the vector length and the device.
// _acquire locks l->mu and, where it returns MMIDX_OK, leaves it locked until _release: an add cannot move the rows under a
// launch that is being enqueued.  It honours lin_wait_other_stream: work another stream still has in flight on the handle (an
// mmidx_linear_add_device, say) is waited for, and `st` becomes the handle's last stream, so a later add on another stream waits
// for the kernels enqueued here.  LOCK ORDER: always the index handle first (DeviceCall, mmidx_index::search_mu), then the Linear
// handle; nothing in the library takes them the other way round.  _dims reads what never changes after mmidx_linear_create.
struct MmidxLinearRows {
    const double *dX;  // [n][D]; null while n == 0
    int64_t n;
    int D, device;
};
MMIDX_HIDDEN void mmidx_internal_linear_dims(const mmidx_linear *l, int *D_out, int *device_out);
MMIDX_HIDDEN int mmidx_internal_linear_rows_acquire(mmidx_linear *l, hipStream_t st, MmidxLinearRows *out);
MMIDX_HIDDEN void mmidx_internal_linear_rows_release(mmidx_linear *l);
// mmidx_refine.hip: K11g -- rows d_iids[q] of dX as queries dQ[nq][D]; d_valid[q] = 0 and a row of zeros for an id outside [0, n)
MMIDX_HIDDEN int mmidx_internal_refine_gather_queries(const double *dX, int64_t n, int D, int64_t nq, const int32_t *d_iids, double *dQ,
                                                      int32_t *d_valid, hipStream_t st);
// mmidx_refine.hip: K11a + K11b for one round of queries on plain device pointers (mmidx_refine.h)
struct MmidxRefineArgs {
    const double *dX;  // the Linear rows [n][D]
    int64_t n;
    int D, k, R;
    int64_t nq;
    const double *dQ;          // [nq][D]
    const int32_t *d_qvalid;   // [nq] or null: 0 = the query does not exist (count 0, padding, nothing counted as missing)
    int32_t *d_cand_iid;       // [nq][R] the compressed answer for k = R; dropped records are overwritten with -1
    double *d_cand_dist;       // [nq][R] its distances on entry, the exact ones of the records kept on return
    const int32_t *d_cand_cnt; // [nq]
    int32_t *d_iid_out;        // [nq][k]
    double *d_dist_out;        // [nq][k]
    int32_t *d_cnt_out;        // [nq]
    int64_t *d_missing;        // one counter the round adds to, or null
};
MMIDX_HIDDEN int mmidx_internal_refine_round(const MmidxRefineArgs *a, hipStream_t st);
// ---- the walk of one Linear index into others (mmidx_linear_reindex, mmidx_reindex.hip) --------------------------------------
// LOCK ORDER of that call, the library's one order: index handles before Linear handles.  First every index target (add_mu, then
// search_mu, as mmidx_add_vectors_device takes them; both recursive, so the appends inside the walk take them again), in ascending
// address order; then the Linear handles -- the source and the Linear targets -- by l->mu, in ascending address order.  The refine rule
// above is the same order (an index handle's search_mu, then the Linear handle), so a refine over a pair that a walk is filling
// waits for the walk or the walk for it; and two walks over the same handles in different argument orders cannot cross.
// mmidx_linear.hip: _lock takes l->mu and reports the handle without any device call; it stays locked until _unlock.  settle = true:
// the caller has waited for everything it enqueued on the handle, so that no later call waits on the caller's stream.
struct MmidxLinearInfo {
    const double *dX;     // [n][D]; null while n == 0
    int64_t n, capacity;  // capacity 0 = unbounded
    int D, device;
    hipStream_t stream;   // the handle's private stream
};
MMIDX_HIDDEN void mmidx_internal_linear_lock(mmidx_linear *l, MmidxLinearInfo *out);
MMIDX_HIDDEN void mmidx_internal_linear_unlock(mmidx_linear *l, bool settle);
// ... orders `st` behind whatever another stream still has in flight on the locked handle (lin_wait_other_stream)
MMIDX_HIDDEN void mmidx_internal_linear_order(mmidx_linear *l, hipStream_t st);
// ... mmidx_linear_add_device on the locked handle
MMIDX_HIDDEN int mmidx_internal_linear_append_locked(mmidx_linear *l, int64_t n, const double *dX, hipStream_t st);
// mmidx_api.hip: the same for an index handle: add_mu and search_mu, and what the walk checks before it launches anything
struct MmidxIndexInfo {
    int64_t n;  // loadCounter
    int D, device, sharded, ready;  // ready: the quantizers the kind needs are loaded
};
MMIDX_HIDDEN void mmidx_internal_index_add_lock(mmidx_index *h, MmidxIndexInfo *out);
MMIDX_HIDDEN void mmidx_internal_index_add_unlock(mmidx_index *h);
// mmidx_frontend.hip: the device of a PCA handle (its sizes: mmidx_pca_get_dims)
MMIDX_HIDDEN int mmidx_internal_pca_device(const mmidx_pca *p);
}  // extern "C"
