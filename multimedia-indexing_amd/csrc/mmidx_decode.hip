// mmidx_decode.hip -- host side of K10 (mmidx_decode.h): launches on plain device pointers.  The entry points that own a handle
// (mmidx_reconstruct, mmidx_search_ids and their _device forms) live in mmidx_api.hip and reach these through mmidx_host.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "mmidx_decode.h"
#include "mmidx_host.h"

namespace {

template <typename CodeT, int R>
int launch_decode(const DecodeParams &P, hipStream_t st) {
    const size_t lds = (size_t)R * P.D * sizeof(double) + 2 * (size_t)R * sizeof(int32_t);
    // (the block is never wider than the vector is long: at D = 128 two waves walk the row, at D >= 256 four)
    const int nt = std::min(256, std::max(64, (P.D + 63) / 64 * 64));
    HIPCK(hipFuncSetAttribute((const void *)k_decode_records<CodeT, R>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const long long blocks = (P.n + R - 1) / R;
    hipLaunchKernelGGL((k_decode_records<CodeT, R>), dim3((unsigned)blocks), dim3(nt), lds, st, P);
    HIPCK(hipGetLastError());
    return MMIDX_OK;
}

}  // namespace

extern "C" {

int mmidx_internal_decode_records(const MmidxDecodeArgs *a, hipStream_t st) {
    if (a->n <= 0) return MMIDX_OK;
    if (a->transform == MMIDX_TR_ROTATION && !a->d_rotT) return mmidx_fail(MMIDX_ERR_NOT_READY, "decode: the transposed rotation is missing");
    if (a->transform == MMIDX_TR_PERMUTATION && !a->d_perm) return mmidx_fail(MMIDX_ERR_NOT_READY, "decode: the permutation is missing");
    DecodeParams P{};
    P.iids = a->d_iids;
    P.inv = a->d_inv;
    P.off = (const long long *)a->d_off;
    P.codes = a->d_codes;
    P.pq = a->d_pq;
    P.coarse = a->d_coarse;
    P.perm = a->d_perm;
    P.rotT = a->d_rotT;
    P.X = a->dX;
    P.found = a->d_found;
    P.n = a->n;
    P.inv_size = a->inv_size;
    P.n_csr = a->n_csr;
    P.nlists = a->nlists;
    P.D = a->D;
    P.m = a->m;
    P.ks = a->ks;
    P.dsub = a->dsub;
    P.transform = a->transform;
    P.ivf = a->ivf;
    // records per block: eight while their z rows stay within 64 KiB of LDS (D <= 1024), then four (D <= 2048), two, one
    const size_t row = (size_t)a->D * sizeof(double);
    const bool b1 = a->code_bytes == 1;
    if (8 * row <= (64u << 10)) return b1 ? launch_decode<unsigned char, 8>(P, st) : launch_decode<unsigned short, 8>(P, st);
    if (4 * row <= (64u << 10)) return b1 ? launch_decode<unsigned char, 4>(P, st) : launch_decode<unsigned short, 4>(P, st);
    if (2 * row <= (128u << 10)) return b1 ? launch_decode<unsigned char, 2>(P, st) : launch_decode<unsigned short, 2>(P, st);
    if (row <= (128u << 10)) return b1 ? launch_decode<unsigned char, 1>(P, st) : launch_decode<unsigned short, 1>(P, st);
    return mmidx_fail(MMIDX_ERR_UNSUPPORTED, "decode: a vector of %d doubles does not fit the LDS", a->D);
}

int mmidx_internal_ids_found(const int32_t *d_iids, int64_t n, const int32_t *d_inv, int64_t inv_size, int64_t n_csr, int32_t *d_found, hipStream_t st) {
    if (n <= 0) return MMIDX_OK;
    hipLaunchKernelGGL(k_ids_found, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_iids, (long long)n, d_inv, (long long)inv_size, (long long)n_csr,
                       d_found);
    HIPCK(hipGetLastError());
    return MMIDX_OK;
}

int mmidx_internal_transpose_square(const double *d_src, double *d_dst, int D, hipStream_t st) {
    const unsigned g = (unsigned)((D + 31) / 32);
    hipLaunchKernelGGL(k_transpose_square, dim3(g, g), dim3(32, 8), 0, st, d_src, d_dst, D);
    HIPCK(hipGetLastError());
    return MMIDX_OK;
}

int mmidx_internal_mark_unknown_rows(const int32_t *d_found, int64_t nq, int k, int32_t *d_iid, double *d_dist, int32_t *d_cnt, hipStream_t st) {
    const long long tot = (long long)nq * k;
    if (tot <= 0) return MMIDX_OK;
    hipLaunchKernelGGL(k_mark_unknown_rows, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, d_found, (long long)nq, k, d_iid, d_dist, d_cnt);
    HIPCK(hipGetLastError());
    return MMIDX_OK;
}

}  // extern "C"
