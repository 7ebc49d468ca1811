// mmidx_remove.hip -- host side of K13 (mmidx_remove.h): launches on plain device pointers.  The entry points that own a handle
// (mmidx_remove, mmidx_remove_device) live in mmidx_api.hip and reach these through mmidx_host.h.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mmidx_host.h"
#include "mmidx_remove.h"

namespace {

template <typename V>
int launch_compact(const MmidxRemoveArgs *a, int rec_bytes, int32_t *d_ids_new, void *d_codes_new, hipStream_t st) {
    const long long ntiles = (a->n + RM_TILE - 1) / RM_TILE;
    hipLaunchKernelGGL(k_rm_compact<V>, dim3((unsigned)ntiles), dim3(RM_NT), 0, st, a->d_ids, (const V *)a->d_codes, (long long)a->n,
                       rec_bytes / (int)sizeof(V), (const rm_u64 *)a->d_keep, (const long long *)a->d_pre, d_ids_new, (V *)d_codes_new);
    HIPCK(hipGetLastError());
    return MMIDX_OK;
}

}  // namespace

extern "C" {

void mmidx_internal_remove_ws(int64_t n, int64_t inv_size, size_t *bits_words, size_t *keep_words, size_t *ntiles) {
    *bits_words = (size_t)((inv_size + 31) / 32);
    *keep_words = (size_t)((n + 63) / 64);
    *ntiles = (size_t)((n + RM_TILE - 1) / RM_TILE);
}

int mmidx_internal_remove_plan(const MmidxRemoveArgs *a, hipStream_t st) {
    if (a->n <= 0) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "remove: no records");
    // (2^31 - 1 records at most: mmidx_add_* refuses more, so a tile count fits a grid)
    size_t bw, kw, nt;
    mmidx_internal_remove_ws(a->n, a->inv_size, &bw, &kw, &nt);
    HIPCK(hipMemsetAsync(a->d_bits, 0, (bw ? bw : 1) * sizeof(unsigned), st));
    if (a->nreq > 0)
        hipLaunchKernelGGL(k_rm_mark, dim3((unsigned)((a->nreq + 255) / 256)), dim3(256), 0, st, a->d_req, (long long)a->nreq, a->d_inv,
                           (long long)a->inv_size, (long long)a->n, a->d_bits, a->d_found);
    hipLaunchKernelGGL(k_rm_flags, dim3((unsigned)nt), dim3(RM_NT), 0, st, a->d_ids, (long long)a->n, (const unsigned *)a->d_bits, (long long)a->inv_size,
                       (rm_u64 *)a->d_keep, a->d_tile_cnt);
    hipLaunchKernelGGL(k_rm_scan, dim3(1), dim3(RM_SCAN_NT), 0, st, (const unsigned *)a->d_tile_cnt, (long long)nt, (long long *)a->d_pre);
    hipLaunchKernelGGL(k_rm_offsets, dim3((unsigned)((a->nlists + 1 + 255) / 256)), dim3(256), 0, st, (const long long *)a->d_off, a->nlists, (long long)a->n,
                       (const rm_u64 *)a->d_keep, (const long long *)a->d_pre, (long long)nt, (long long *)a->d_off_new);
    HIPCK(hipGetLastError());
    return MMIDX_OK;
}

int mmidx_internal_remove_compact(const MmidxRemoveArgs *a, int32_t *d_ids_new, void *d_codes_new, hipStream_t st) {
    const int rb = a->rec_bytes;
    if (rb <= 0) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "remove: a record of %d bytes", rb);
    if (rb % 16 == 0) return launch_compact<uint4>(a, rb, d_ids_new, d_codes_new, st);
    if (rb % 8 == 0) return launch_compact<uint2>(a, rb, d_ids_new, d_codes_new, st);
    if (rb % 4 == 0) return launch_compact<unsigned>(a, rb, d_ids_new, d_codes_new, st);
    if (rb % 2 == 0) return launch_compact<unsigned short>(a, rb, d_ids_new, d_codes_new, st);
    return launch_compact<unsigned char>(a, rb, d_ids_new, d_codes_new, st);
}

}  // extern "C"
