// mmidx_reindex.hip -- host side of K12 (mmidx_reindex.h) and the walk built on it: mmidx_truncate_l2_device on plain device
// pointers, and mmidx_linear_reindex, which takes a range of rows of a Linear handle through an optional PCA projection, through K12
// once for all targets, and appends every truncation to its own Linear / PQ / IVFPQ handle (IndexTransformation.java:61-125,
// PCAProjectionExample.java:74-88).  The handles' insides stay in their own units: mmidx_host.h declares what is reached here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <functional>

#include "mmidx_host.h"
#include "mmidx_reindex.h"

namespace {

// the checks of mmidx_truncate_l2_device that need no device; fills the kernel's arguments
int trl_prepare(const char *name, int64_t n, int ncols, int64_t ld, int nt, const int32_t *lens, const int32_t *normalize, double *const *dY, TrlArgs *a) {
    if (nt < 1 || nt > TRL_MAX_T) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "%s: %d targets, 1..%d are possible", name, nt, TRL_MAX_T);
    if (n < 0) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "%s: n = %lld is negative", name, (long long)n);
    if (ncols < 1) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "%s: ncols = %d must be positive", name, ncols);
    if (ld < ncols) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "%s: ld = %lld is below ncols = %d", name, (long long)ld, ncols);
    if (!lens || !normalize || !dY) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "%s: null argument", name);
    *a = TrlArgs{};
    a->nt = nt;
    for (int t = 0; t < nt; t++) {
        if (lens[t] < 1 || lens[t] > ncols) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "%s: target %d has length %d, outside 1..%d", name, t, lens[t], ncols);
        if (normalize[t] < 0 || normalize[t] > 2) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "%s: normalize[%d] = %d, outside 0..2", name, t, normalize[t]);
        if (n > 0 && !dY[t]) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "%s: dY[%d] is null", name, t);
        a->y[t] = dY[t];
        a->len[t] = lens[t];
        a->norm[t] = normalize[t] == 1 || (normalize[t] == 2 && lens[t] < ncols);
        a->maxlen = std::max(a->maxlen, (int)lens[t]);
    }
    return MMIDX_OK;
}

template <bool CACHED, bool VEC>
int trl_launch_as(int64_t n, int64_t ld, const double *dX, const TrlArgs &a, size_t lds, hipStream_t st) {
    // the LDS limit of an instantiation is raised once per device to the most any launch asks for (160 KiB), not per launch
    static std::atomic<bool> raised[TRL_MAX_DEV];
    if (lds > 64 * 1024) {
        int dev = 0;
        HIPCK(hipGetDevice(&dev));
        if (dev < 0 || dev >= TRL_MAX_DEV || !raised[dev].load(std::memory_order_acquire)) {
            HIPCK(hipFuncSetAttribute((const void *)k_truncate_l2<CACHED, VEC>, hipFuncAttributeMaxDynamicSharedMemorySize, TRL_LDS_MAX));
            if (dev >= 0 && dev < TRL_MAX_DEV) raised[dev].store(true, std::memory_order_release);
        }
    }
    hipLaunchKernelGGL((k_truncate_l2<CACHED, VEC>), dim3((unsigned)((n + TRL_ROWS - 1) / TRL_ROWS)), dim3(TRL_NT), lds, st, dX, (long long)n, (long long)ld, a);
    HIPCK(hipGetLastError());
    return MMIDX_OK;
}

// the longest row K12 keeps in LDS.  The environment variable MMIDX_TRL_CACHED_MAX (0 .. 288) moves it for measurements and tests
// (it changes no bit of a result): rows beyond it take the streamed form.
int trl_cached_max() {
    int lim = TRL_CACHED_MAX;
    if (const char *e = getenv("MMIDX_TRL_CACHED_MAX")) {
        const long v = strtol(e, nullptr, 10);
        if (v >= 0 && v <= TRL_CACHED_FIT) lim = (int)v;
    }
    return lim;
}

// The tiling: rows of L = max(lens) columns stay in LDS up to TRL_CACHED_MAX = 128 columns (one read of every element,
// two or more blocks per CU), else two staging tiles and a second read, which the L2 serves; 16-byte loads where every row segment is 16-byte aligned.
int trl_launch(int64_t n, int64_t ld, const double *dX, const TrlArgs &a, hipStream_t st) {
    if (n == 0) return MMIDX_OK;
    if ((n + TRL_ROWS - 1) / TRL_ROWS > 0x7fffffff) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "mmidx_truncate_l2_device: %lld rows in one launch", (long long)n);
    const bool vec = (ld % 2 == 0) && ((uintptr_t)dX % 16 == 0);
    const size_t cached = trl_cached_lds(a.maxlen);
    if (a.maxlen <= trl_cached_max() && cached <= TRL_LDS_MAX)
        return vec ? trl_launch_as<true, true>(n, ld, dX, a, cached, st) : trl_launch_as<true, false>(n, ld, dX, a, cached, st);
    return vec ? trl_launch_as<false, true>(n, ld, dX, a, TRL_STREAM_LDS, st) : trl_launch_as<false, false>(n, ld, dX, a, TRL_STREAM_LDS, st);
}

// The locks of one walk, in the library's one order (mmidx_host.h): index handles, then Linear handles, each class by ascending
// address; released in reverse on every return path.
struct WalkLocks {
    mmidx_index *ix[TRL_MAX_T] = {};
    mmidx_linear *lin[TRL_MAX_T + 1] = {};
    int nix = 0, nlin = 0, ix_held = 0, lin_held = 0;
    mmidx_linear *src = nullptr;
    bool settle = false;  // the walk ran and was waited for: nothing of it is in flight on the Linear targets
    ~WalkLocks() {
        for (int i = lin_held - 1; i >= 0; i--) mmidx_internal_linear_unlock(lin[i], settle && lin[i] != src);
        for (int i = ix_held - 1; i >= 0; i--) mmidx_internal_index_add_unlock(ix[i]);
    }
};

}  // namespace

extern "C" {

int mmidx_truncate_l2_device(int device, int64_t n, int ncols, int64_t ld, const double *dX, int nt, const int32_t *lens, const int32_t *normalize,
                             double *const *dY, void *stream) {
    TrlArgs a;
    int rc = trl_prepare("mmidx_truncate_l2_device", n, ncols, ld, nt, lens, normalize, dY, &a);
    if (rc) return rc;
    if (n > 0 && !dX) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "mmidx_truncate_l2_device: dX is null");
    if (n == 0) return MMIDX_OK;
    const int ndev = mmidx_device_count();
    if (device < 0 || device >= ndev) return mmidx_fail(MMIDX_ERR_NO_DEVICE, "device %d outside 0..%d", device, ndev - 1);
    HIPCK(hipSetDevice(device));
    return trl_launch(n, ld, dX, a, (hipStream_t)stream);
}

int mmidx_linear_reindex(mmidx_linear *src, int64_t iid0, int64_t n, mmidx_pca *pca, int nt, const int32_t *kinds, void *const *targets,
                         const int32_t *normalize, int64_t chunk_rows) {
    const char *name = "mmidx_linear_reindex";
    // ---- what needs no handle contents ----
    if (!src) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "%s: null source handle", name);
    if (nt < 1 || nt > TRL_MAX_T) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "%s: %d targets, 1..%d are possible", name, nt, TRL_MAX_T);
    if (!kinds || !targets || !normalize) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "%s: null argument", name);
    if (n < 0) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "%s: n = %lld is negative", name, (long long)n);
    if (chunk_rows < 0) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "%s: chunk_rows = %lld is negative", name, (long long)chunk_rows);
    if (iid0 < 0) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "%s: iid0 = %lld is negative", name, (long long)iid0);
    for (int t = 0; t < nt; t++) {
        if (!targets[t]) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "%s: targets[%d] is null", name, t);
        if (kinds[t] < 0 || kinds[t] > 1) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "%s: kinds[%d] = %d, outside 0..1", name, t, kinds[t]);
        if (normalize[t] < 0 || normalize[t] > 2) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "%s: normalize[%d] = %d, outside 0..2", name, t, normalize[t]);
    }
    for (int t = 0; t < nt; t++) {  // (before any lock: a handle locked twice would never return)
        if (targets[t] == (void *)src) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "%s: targets[%d] is the source handle", name, t);
        for (int u = 0; u < t; u++)
            if (targets[t] == targets[u]) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "%s: targets[%d] and targets[%d] are the same handle", name, u, t);
    }
    // ---- the handles: every index target (ascending address), then the Linear handles, source included (ascending address) ----
    WalkLocks locks;
    locks.src = src;
    int slot[TRL_MAX_T] = {};  // target t's place among the locks of its class
    locks.lin[locks.nlin++] = src;
    for (int t = 0; t < nt; t++) {
        if (kinds[t] == 0) locks.lin[locks.nlin++] = (mmidx_linear *)targets[t];
        else locks.ix[locks.nix++] = (mmidx_index *)targets[t];
    }
    std::sort(locks.ix, locks.ix + locks.nix, std::less<mmidx_index *>());
    std::sort(locks.lin, locks.lin + locks.nlin, std::less<mmidx_linear *>());
    for (int t = 0; t < nt; t++)
        slot[t] = kinds[t] == 0 ? (int)(std::find(locks.lin, locks.lin + locks.nlin, (mmidx_linear *)targets[t]) - locks.lin)
                                : (int)(std::find(locks.ix, locks.ix + locks.nix, (mmidx_index *)targets[t]) - locks.ix);
    MmidxIndexInfo xi[TRL_MAX_T] = {};
    MmidxLinearInfo li[TRL_MAX_T + 1] = {};
    for (int i = 0; i < locks.nix; i++) {
        mmidx_internal_index_add_lock(locks.ix[i], &xi[i]);
        locks.ix_held = i + 1;
    }
    for (int i = 0; i < locks.nlin; i++) {
        mmidx_internal_linear_lock(locks.lin[i], &li[i]);
        locks.lin_held = i + 1;
    }
    const MmidxLinearInfo si = li[std::find(locks.lin, locks.lin + locks.nlin, src) - locks.lin];
    int32_t lens[TRL_MAX_T] = {};
    int64_t sizes[TRL_MAX_T] = {};
    int devs[TRL_MAX_T] = {};
    bool sharded[TRL_MAX_T] = {}, ready[TRL_MAX_T] = {};
    int64_t caps[TRL_MAX_T] = {};
    for (int t = 0; t < nt; t++) {
        ready[t] = true;
        caps[t] = 0x7fffffff;
        if (kinds[t] == 0) {
            const MmidxLinearInfo &ti = li[slot[t]];
            lens[t] = ti.D;
            sizes[t] = ti.n;
            devs[t] = ti.device;
            if (ti.capacity > 0) caps[t] = std::min<int64_t>(ti.capacity, 0x7fffffff);
        } else {
            const MmidxIndexInfo &ti = xi[slot[t]];
            lens[t] = ti.D;
            sizes[t] = ti.n;
            devs[t] = ti.device;
            sharded[t] = ti.sharded != 0;
            ready[t] = ti.ready != 0;
        }
    }
    for (int t = 0; t < nt; t++)
        if (sharded[t])
            return mmidx_fail(MMIDX_ERR_UNSUPPORTED, "%s: targets[%d] is a sharded handle: the walk fills plain handles on the source's device", name, t);
    if (n > si.n - iid0)  // (not iid0 + n: two huge values would overflow before the refusal)
        return mmidx_fail(MMIDX_ERR_INVALID_ARG, "%s: %lld rows from row %lld are asked for, the source holds %lld", name, (long long)n, (long long)iid0, (long long)si.n);
    int ncols = si.D;
    if (pca) {
        int nc = 0, ss = 0;
        mmidx_pca_get_dims(pca, &nc, &ss);
        if (ss != si.D) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "%s: the PCA takes samples of length %d, the source holds vectors of length %d", name, ss, si.D);
        const int pdev = mmidx_internal_pca_device(pca);
        if (pdev != si.device) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "%s: the PCA is on device %d, the source on device %d", name, pdev, si.device);
        ncols = nc;
    }
    for (int t = 0; t < nt; t++) {
        if (devs[t] != si.device) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "%s: targets[%d] is on device %d, the source on device %d", name, t, devs[t], si.device);
        if (lens[t] > ncols) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "%s: targets[%d] holds vectors of length %d, the walk delivers %d columns", name, t, lens[t], ncols);
        if (sizes[t] != iid0)
            return mmidx_fail(MMIDX_ERR_INVALID_ARG, "%s: targets[%d] holds %lld records, iid0 = %lld: record i of a target must be row i of the source", name, t,
                              (long long)sizes[t], (long long)iid0);
        if (n > caps[t] - iid0)
            return mmidx_fail(MMIDX_ERR_INVALID_ARG, "%s: targets[%d] has room for %lld more vectors, n = %lld", name, t, (long long)(caps[t] - iid0), (long long)n);
    }
    for (int t = 0; t < nt; t++)
        if (!ready[t]) return mmidx_fail(MMIDX_ERR_NOT_READY, "%s: targets[%d] has no codebooks yet (loadCoarseQuantizer / loadProductQuantizer)", name, t);
    if (n == 0) return MMIDX_OK;

    // ---- the walk ----
    HIPCK(hipSetDevice(si.device));
    hipStream_t st = si.stream;
    mmidx_internal_linear_order(src, st);  // (an mmidx_linear_add_device on another stream may still be writing the rows)
    // the default chunk: 2^25 doubles (256 MiB) of the widest row the walk buffers -- the projected row with a PCA, else the longest
    // target (the stored rows are read in place) -- within 4096 .. 2^20 rows, whole blocks of K12.  Every chunk ends in a host wait
    // (the appends are synchronous), so few large chunks beat many small ones.
    const int wide = pca ? ncols : *std::max_element(lens, lens + nt);
    int64_t chunk = chunk_rows > 0 ? chunk_rows : std::min<int64_t>(1 << 20, std::max<int64_t>(4096, ((int64_t)1 << 25) / wide)) / TRL_ROWS * TRL_ROWS;
    chunk = std::min(chunk, n);
    DevPtr<double> proj, out[TRL_MAX_T];
    double *dY[TRL_MAX_T] = {};
    if (pca) HIPCK(proj.alloc((size_t)chunk * ncols));
    for (int t = 0; t < nt; t++) {
        HIPCK(out[t].alloc((size_t)chunk * lens[t]));
        dY[t] = out[t].p;
    }
    TrlArgs a;
    int rc = trl_prepare(name, chunk, ncols, ncols, nt, lens, normalize, dY, &a);
    if (rc) return rc;
    for (int64_t r0 = 0; r0 < n && rc == MMIDX_OK; r0 += chunk) {
        const int64_t nb = std::min(chunk, n - r0);
        const double *rows = si.dX + (size_t)(iid0 + r0) * si.D;
        int64_t ld = si.D;
        if (pca) {
            rc = mmidx_pca_project_device(pca, nb, rows, proj.p, st);
            if (rc) break;
            rows = proj.p;
            ld = ncols;
        }
        rc = trl_launch(nb, ld, rows, a, st);
        for (int t = 0; t < nt && rc == MMIDX_OK; t++) {
            if (kinds[t] == 0) rc = mmidx_internal_linear_append_locked((mmidx_linear *)targets[t], nb, dY[t], st);
            else rc = mmidx_add_vectors_device((mmidx_index *)targets[t], nb, dY[t], nullptr, (int32_t)(iid0 + r0), st);
        }
    }
    const hipError_t e = hipStreamSynchronize(st);  // synchronous: every target is complete on return (and the buffers can go)
    if (rc) return rc;
    HIPCK(e);
    locks.settle = true;
    return MMIDX_OK;
}

}  // extern "C"
