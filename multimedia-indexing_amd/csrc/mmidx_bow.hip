// mmidx_bow.hip -- bag-of-words aggregation on the GPU: BowAggregator.aggregateInternal (J/aggregation/BowAggregator.java:39-74).
//
// The reference, for one image's descriptors and bow = new double[numCentroids]:
//   k == 1   bow[computeNearestCentroid(d)]++ per descriptor (AbstractFeatureAggregator.java:136-155, strict `<`: the first of
//            several equally near centroids wins);
//   k  > 1   nn = computeKNearestCentroids(d, k) (AFA:193-220: the bounded queue of IVFPQ.computeNearestCoarseIndices, line for
//            line), and for each of the k indices bow[nn[j]]++ runs descriptorLength times (the inner loop :47-51, sic): every
//            (descriptor, neighbour) hit adds dl.  Only the SET of the k indices matters; ties at the k-th position follow the
//            bounded queue (assumption A1).
// Here:
//   assignment  a hidden index handle whose coarse quantizer is the vocabulary, as mmidx_vlad_create builds: hard through
//               mmidx_assign_device (certified bf16-split MFMA argmin, flagged rows redone in fp64), soft through mmidx_set_w(k) +
//               mmidx_coarse_device (cells [n][k]; the distances are not needed).  Descriptors are taken in chunks of at most
//               BOW_CELL_BUDGET cell entries.  nc == 1 (the handle needs two centroids) is served directly: bow[0] = n.
//   histogram   K9a k_bow_hist_lds: a block per image counts HITS in 32-bit LDS counters (ds_add_u32) and writes the image's row
//               once, zeros included, as hits * (k == 1 ? 1 : dl) -- no memset of the output.  Vocabularies of up to 40960 words
//               (160 KiB of counters), calls whose descriptors fit one assignment chunk.
//               K9b k_bow_hist_global + k_bow_convert: the output itself, zeroed, holds the counters (the low 32 bits of every
//               8-byte slot); a thread per hit finds its image by bisection of desc_off and adds 1 with a plain atomicAdd -- a long
//               image is spread over as many blocks as it has hits / 256 --, then every slot is converted in place to
//               (double)(hits * weight).  Larger vocabularies, calls of several chunks, option "hist_global".
// The weight is never accumulated: counters hold hits, so they overflow only at 2^32 hits of one word in one image.  All values are
// integers far below 2^53: the result is bit-exact whatever the order of the atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "mmidx_host.h"

namespace {

constexpr long long BOW_CELL_BUDGET = 1ll << 25;   // int32 cell entries per assignment chunk (128 MiB)
constexpr long long BOW_OUT_BUDGET = 1ll << 27;    // doubles of the host form's dense [chunk][nc] workspace (1 GiB)
constexpr long long BOW_DESC_BUDGET = 1ll << 28;   // doubles of descriptors staged per host-form chunk (2 GiB; one image may exceed it)
constexpr int BOW_LDS_MAX_NC = 160 * 1024 / 4;     // K9a: the counters alone fill the LDS
constexpr int BOW_K_MAX = (64 * 1024 - 16) / 12 - 1;  // 5459: the coarse stage's exact selection keeps k + 1 entries of 12 bytes in a 64 KiB block
constexpr int BOW_LDS_SMALL = 32 * 1024;           // counters up to here: 256-thread blocks, five or more per CU; above: 1024 threads

// ------------------------------------------------------------------------------------------------
// K9a: a block per image.  cells[(d - d0) * k + j] = the j-th nearest word of descriptor d (absolute index d, as desc_off counts).
// Counting: ds_add_u32 without return; lanes that hit one word serialise on its bank, which a 1000-descriptor image never notices
// next to the assignment in front of it.  The row is written with consecutive lanes on consecutive doubles.
// ------------------------------------------------------------------------------------------------
__global__ void k_bow_hist_lds(const int32_t *__restrict__ cells, const long long *__restrict__ desc_off, long long d0, long long nhits, int nc,
                               int k, unsigned weight, double *__restrict__ out) {
    extern __shared__ unsigned bow_cnt[];
    const int tid = threadIdx.x, nt = blockDim.x;
    const long long img = blockIdx.x;
    for (int c = tid; c < nc; c += nt) bow_cnt[c] = 0u;
    __syncthreads();
    // (clamped to the cells the assignment wrote: offsets that leave the call's descriptor range count nothing out of bounds)
    const long long lo = std::max<long long>((desc_off[img] - d0) * k, 0), hi = std::min<long long>((desc_off[img + 1] - d0) * k, nhits);
    for (long long t = lo + tid; t < hi; t += nt) {
        const int c = cells[t];
        if ((unsigned)c < (unsigned)nc) atomicAdd(&bow_cnt[c], 1u);
    }
    __syncthreads();
    double *row = out + (size_t)img * nc;
    for (int c = tid; c < nc; c += nt) row[c] = (double)((unsigned long long)bow_cnt[c] * weight);
}

// ------------------------------------------------------------------------------------------------
// K9b: a thread per hit of the chunk [d0, d0 + n).  The image of descriptor d is the last i < nimg with desc_off[i] <= d (empty
// images repeat an offset: they own no descriptor); the offsets are a few KiB that every block reads, so the bisection runs out
// of L1 / L2.  Counter = the low 32 bits of the image's 8-byte output slot (little-endian; the slot was zeroed by the caller).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bow_hist_global(const int32_t *__restrict__ cells, const long long *__restrict__ desc_off,
                                                         long long nimg, long long d0, long long nhits, int nc, int k,
                                                         double *__restrict__ out) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= nhits) return;
    const long long d = d0 + t / k;
    long long a = 0, b = nimg;  // invariant: desc_off[a] <= d, (b == nimg or desc_off[b] > d)
    while (b - a > 1) {
        const long long m = (a + b) >> 1;
        if (desc_off[m] <= d) a = m;
        else b = m;
    }
    const int c = cells[t];
    if (d < desc_off[a] || d >= desc_off[a + 1] || (unsigned)c >= (unsigned)nc) return;  // (offsets that do not cover d: nothing to count)
    atomicAdd(reinterpret_cast<unsigned *>(out + (size_t)a * nc + c), 1u);
}

// every slot in place: 8 bytes read, 8 bytes written by the same thread
__global__ __launch_bounds__(256) void k_bow_convert(double *__restrict__ out, long long n, unsigned weight) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long u = reinterpret_cast<const unsigned long long *>(out)[i];
    out[i] = (double)((u & 0xFFFFFFFFull) * weight);
}

// nc == 1: the one word takes every descriptor (k == 1, weight 1)
__global__ __launch_bounds__(256) void k_bow_single(const long long *__restrict__ desc_off, long long nimg, double *__restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < nimg) out[i] = (double)(desc_off[i + 1] - desc_off[i]);
}

}  // namespace

struct MMIDX_HIDDEN mmidx_bow {
    Stream stream;  // (before what is used on it: members are destroyed in reverse order)
    std::mutex mu;  // one call at a time per handle enqueues: the workspaces, the options and last_stream are shared
    hipStream_t last_stream = nullptr;  // the stream the workspaces were last used on: another stream waits for it first
    bool last_stream_valid = false;
    PinBuf<long long> pin_ends;  // 16 pinned bytes for the read-back of the call's descriptor range
    int nc = 0, dl = 0, k = 1, device = 0;
    mmidx_index *asg = nullptr;  // the vocabulary as the coarse quantizer of a hidden index (nc >= 2)
    DevBuf<int32_t> ws_cells;
    DevBuf<double> ws_desc, ws_out;
    DevBuf<long long> ws_off;
    int hist_global = 0;   // option "hist_global": K9b also where K9a applies
    int chunk_images = 0;  // option "chunk_images": images per round of the host form (0 = sized from the budgets)
};

namespace {

// images [0, nimg) whose descriptors are [dlo, dhi) of d_descs (both known on the host); everything is enqueued on st
int bow_run(mmidx_bow *b, int64_t nimg, const long long *d_off, const double *d_descs, long long dlo, long long dhi, double *d_out,
            hipStream_t st) {
    const long long ndesc = dhi - dlo;
    if (ndesc < 0) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "descriptor offsets decrease (%lld .. %lld)", dlo, dhi);
    if (ndesc > 0 && !d_descs) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null descriptors");
    const int nc = b->nc, k = b->k;
    if (b->last_stream_valid && b->last_stream != st) {
        // the cell buffer may still be read by the histogram of the call before, on another stream (which the caller may have
        // destroyed since: HIP then rejects the handle and the device is waited for instead)
        if (hipStreamSynchronize(b->last_stream) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipDeviceSynchronize();
        }
    }
    b->last_stream = st;
    b->last_stream_valid = true;
    const unsigned weight = k == 1 ? 1u : (unsigned)b->dl;  // BowAggregator.java:47-51: bow[nn[j]]++ descriptorLength times
    if (nc == 1) {
        hipLaunchKernelGGL(k_bow_single, dim3((unsigned)((nimg + 255) / 256)), dim3(256), 0, st, d_off, (long long)nimg, d_out);
        HIPCK(hipGetLastError());
        return MMIDX_OK;
    }
    const long long chunk = std::max<long long>(1, BOW_CELL_BUDGET / k);
    const bool lds_form = !b->hist_global && nc <= BOW_LDS_MAX_NC && ndesc <= chunk;
    const long long slots = (long long)nimg * nc;
    if (!lds_form) HIPCK(hipMemsetAsync(d_out, 0, (size_t)slots * 8, st));
    HIPCK(b->ws_cells.reserve((size_t)std::max<long long>(1, std::min(ndesc, chunk) * k)));
    for (long long c0 = dlo; c0 < dhi; c0 += chunk) {
        const long long n = std::min(chunk, dhi - c0);
        const double *x = d_descs + (size_t)c0 * b->dl;
        int rc = k == 1 ? mmidx_assign_device(b->asg, n, x, b->ws_cells.p, st) : mmidx_coarse_device(b->asg, n, x, b->ws_cells.p, nullptr, st);
        if (rc) return rc;
        HIPCK(hipSetDevice(b->device));
        if (!lds_form) {
            const long long nhits = n * k;
            hipLaunchKernelGGL(k_bow_hist_global, dim3((unsigned)((nhits + 255) / 256)), dim3(256), 0, st, b->ws_cells.p, d_off, (long long)nimg, c0,
                               nhits, nc, k, d_out);
            HIPCK(hipGetLastError());
        }
    }
    if (lds_form) {
        const size_t lds = (size_t)nc * 4;
        const int nt = lds <= (size_t)BOW_LDS_SMALL ? 256 : 1024;
        if (lds > 64 * 1024)  // (beyond the default limit of dynamic LDS only)
            HIPCK(hipFuncSetAttribute((const void *)k_bow_hist_lds, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        hipLaunchKernelGGL(k_bow_hist_lds, dim3((unsigned)nimg), dim3(nt), lds, st, b->ws_cells.p, d_off, dlo, ndesc * k, nc, k, weight, d_out);
    } else {
        hipLaunchKernelGGL(k_bow_convert, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, st, d_out, slots, weight);
    }
    HIPCK(hipGetLastError());
    return MMIDX_OK;
}

}  // namespace

extern "C" {

int mmidx_bow_create(int nc, int dl, int k, const double *codebook, int device, mmidx_bow **out) {
    if (!out) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null out pointer");
    *out = nullptr;
    if (!codebook) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null codebook");
    if (nc < 1) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "numCentroids = %d: the codebook is empty", nc);
    if (dl < 1) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "descriptorLength = %d must be >= 1", dl);
    if (k < 1) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "k = %d must be >= 1 (BoundedPriorityQueue constructor)", k);
    if (k > nc) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "k = %d exceeds the %d centroids of the codebook (AFA:214-217 polls an empty queue)", k, nc);
    if (k > BOW_K_MAX)
        return mmidx_fail(MMIDX_ERR_UNSUPPORTED, "k = %d beyond the %d neighbours the coarse stage's selection holds in LDS", k, BOW_K_MAX);
    const int ndev = mmidx_device_count();
    if (ndev < 1) return mmidx_fail(MMIDX_ERR_NO_DEVICE, "no HIP device: libmmidx_hip has no CPU fallback");
    if (device < 0 || device >= ndev) return mmidx_fail(MMIDX_ERR_NO_DEVICE, "device %d outside 0..%d", device, ndev - 1);
    HIPCK(hipSetDevice(device));
    std::unique_ptr<mmidx_bow, int (*)(mmidx_bow *)> b(new mmidx_bow(), mmidx_bow_destroy);  // (destroy: the hidden index goes with it)
    if (b->pin_ends.alloc(2) != hipSuccess) {  // (the read-back then lands in pageable memory)
        b->pin_ends.p = nullptr;
        (void)hipGetLastError();
    }
    b->nc = nc;
    b->dl = dl;
    b->k = k;
    b->device = device;
    hipError_t e = b->stream.create();
    if (e != hipSuccess) return mmidx_fail(MMIDX_ERR_HIP, "hipStreamCreate failed: %s", hipGetErrorString(e));
    if (nc >= 2) {
        // m = 1, ks = 2 with an all-zero product quantizer: never used, but mmidx_coarse_device wants a complete index
        int rc = mmidx_create(MMIDX_KIND_IVFPQ, dl, 1, 2, nc, MMIDX_TR_NONE, nullptr, nullptr, device, &b->asg);
        if (rc == MMIDX_OK) rc = mmidx_set_coarse(b->asg, codebook);
        if (rc == MMIDX_OK && k > 1) {
            std::vector<double> zero((size_t)2 * dl, 0.0);
            rc = mmidx_set_pq(b->asg, zero.data());
            if (rc == MMIDX_OK) rc = mmidx_set_w(b->asg, k);
        }
        if (rc != MMIDX_OK) return rc;  // (the message of the failing call stands)
    }
    *out = b.release();
    return MMIDX_OK;
}

int mmidx_bow_destroy(mmidx_bow *b) {
    if (!b) return MMIDX_OK;
    (void)hipSetDevice(b->device);
    if (b->asg) mmidx_destroy(b->asg);
    delete b;
    return MMIDX_OK;
}

int mmidx_bow_get_dims(const mmidx_bow *b, int *nc, int *dl, int *k) {
    if (!b) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null handle");
    if (nc) *nc = b->nc;
    if (dl) *dl = b->dl;
    if (k) *k = b->k;
    return MMIDX_OK;
}

int mmidx_bow_set_option(mmidx_bow *b, const char *name, int value) {
    if (!b || !name) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null argument");
    const std::string n(name);
    std::lock_guard<std::mutex> lk(b->mu);
    if (n == "exact") return b->asg ? mmidx_set_option(b->asg, "exact_coarse", value != 0) : MMIDX_OK;
    if (n == "hist_global") {
        b->hist_global = value != 0;
        return MMIDX_OK;
    }
    if (n == "chunk_images") {
        if (value < 0) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "chunk_images = %d must be >= 0", value);
        b->chunk_images = value;
        return MMIDX_OK;
    }
    return mmidx_fail(MMIDX_ERR_INVALID_ARG, "unknown option '%s'", name);
}

int mmidx_bow_aggregate_device(mmidx_bow *b, int64_t nimg, const int64_t *d_desc_off, const double *d_descs, int max_desc, double *d_out,
                               void *stream) {
    if (!b) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null handle");
    if (nimg < 0 || max_desc < 0 || (nimg > 0 && (!d_desc_off || !d_out))) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null argument");
    if (nimg == 0) return MMIDX_OK;
    std::lock_guard<std::mutex> lk(b->mu);  // (held while the call is ENQUEUED; bow_run orders the workspaces between streams)
    HIPCK(hipSetDevice(b->device));
    hipStream_t st = (hipStream_t)stream;
    long long stack_ends[2] = {0, 0};
    long long *ends = b->pin_ends ? b->pin_ends.p : stack_ends;  // the descriptor range of the call: the assignment is sized by it
    ends[0] = ends[1] = 0;
    if (b->nc > 1) {
        if (nimg == 1) {
            HIPCK(hipMemcpyAsync(ends, d_desc_off, 16, hipMemcpyDeviceToHost, st));
        } else {
            HIPCK(hipMemcpyAsync(&ends[0], d_desc_off, 8, hipMemcpyDeviceToHost, st));
            HIPCK(hipMemcpyAsync(&ends[1], d_desc_off + nimg, 8, hipMemcpyDeviceToHost, st));
        }
        HIPCK(hipStreamSynchronize(st));
    }
    const long long dlo = ends[0], dhi = ends[1];
    return bow_run(b, nimg, (const long long *)d_desc_off, d_descs, dlo, dhi, d_out, st);
}

int mmidx_bow_aggregate(mmidx_bow *b, int64_t nimg, const int64_t *desc_off, const double *descs, double *out) {
    if (!b) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null handle");
    if (nimg < 0 || (nimg > 0 && (!desc_off || !out))) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null argument");
    if (nimg == 0) return MMIDX_OK;
    for (int64_t i = 0; i < nimg; i++)
        if (desc_off[i + 1] < desc_off[i]) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "desc_off decreases at image %lld", (long long)i);
    if (desc_off[nimg] > desc_off[0] && !descs) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null descriptors");
    std::lock_guard<std::mutex> lk(b->mu);
    HIPCK(hipSetDevice(b->device));
    const int64_t by_out = std::max<int64_t>(1, BOW_OUT_BUDGET / b->nc);
    std::vector<long long> off;
    for (int64_t i0 = 0; i0 < nimg;) {
        // a round: as many images as the dense output workspace takes, cut where the staged descriptors pass their budget
        int64_t nb = std::min<int64_t>(nimg - i0, b->chunk_images > 0 ? b->chunk_images : by_out);
        if (b->chunk_images == 0) {
            int64_t j = 1;
            while (j < nb && (desc_off[i0 + j + 1] - desc_off[i0]) * (int64_t)b->dl <= BOW_DESC_BUDGET) j++;
            nb = j;
        }
        const int64_t total = desc_off[i0 + nb] - desc_off[i0];
        off.resize((size_t)nb + 1);
        for (int64_t i = 0; i <= nb; i++) off[(size_t)i] = desc_off[i0 + i] - desc_off[i0];
        HIPCK(b->ws_off.reserve((size_t)nb + 1));
        HIPCK(b->ws_desc.reserve((size_t)std::max<int64_t>(total, 1) * b->dl));
        HIPCK(b->ws_out.reserve((size_t)nb * b->nc));
        HIPCK(hipMemcpyAsync(b->ws_off.p, off.data(), ((size_t)nb + 1) * 8, hipMemcpyHostToDevice, b->stream));
        if (total > 0)
            HIPCK(hipMemcpyAsync(b->ws_desc.p, descs + (size_t)desc_off[i0] * b->dl, (size_t)total * b->dl * 8, hipMemcpyHostToDevice, b->stream));
        int rc = bow_run(b, nb, b->ws_off.p, b->ws_desc.p, 0, total, b->ws_out.p, b->stream);
        if (rc) return rc;
        HIPCK(hipMemcpyAsync(out + (size_t)i0 * b->nc, b->ws_out.p, (size_t)nb * b->nc * 8, hipMemcpyDeviceToHost, b->stream));
        HIPCK(hipStreamSynchronize(b->stream));  // (off is reused by the next round)
        i0 += nb;
    }
    return MMIDX_OK;
}

}  // extern "C"
