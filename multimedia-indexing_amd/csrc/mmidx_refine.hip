// mmidx_refine.hip -- host side of K11 (mmidx_refine.h): launches on plain device pointers.  The entry points that own the handles
// (mmidx_search_refine, _device, _ids) live in mmidx_api.hip beside the id queries and reach these through mmidx_host.h.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mmidx_host.h"
#include "mmidx_refine.h"

namespace {

// K11b: one block per query, LDS sized for the round's R
template <int CAP>
int launch_select(const MmidxRefineArgs *a, hipStream_t st) {
    hipLaunchKernelGGL(k_refine_select<CAP>, dim3((unsigned)a->nq), dim3(RF_NT), 0, st, a->k, a->R, a->d_qvalid, a->d_cand_iid, a->d_cand_dist, a->d_cand_cnt,
                       a->d_iid_out, a->d_dist_out, a->d_cnt_out);
    HIPCK(hipGetLastError());
    return MMIDX_OK;
}

}  // namespace

extern "C" {

int mmidx_internal_refine_gather_queries(const double *dX, int64_t n, int D, int64_t nq, const int32_t *d_iids, double *dQ, int32_t *d_valid,
                                         hipStream_t st) {
    if (nq <= 0) return MMIDX_OK;
    hipLaunchKernelGGL(k_refine_gather_queries, dim3((unsigned)((nq * D + 255) / 256)), dim3(256), 0, st, dX, (long long)n, D, d_iids, dQ, d_valid,
                       (long long)nq);
    HIPCK(hipGetLastError());
    return MMIDX_OK;
}

int mmidx_internal_refine_round(const MmidxRefineArgs *a, hipStream_t st) {
    if (a->nq <= 0) return MMIDX_OK;
    if (a->k < 1 || a->R < a->k || a->R >= RF_CAP) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "refine: k = %d, R = %d outside 1 <= k <= R <= %d", a->k, a->R, RF_CAP - 1);
    if (a->nq > 0x7fffffff) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "refine: %lld queries in one round", (long long)a->nq);
    // K11a: (query, tile of 256 candidates); tiles beyond a query's count return at once
    hipLaunchKernelGGL(k_refine_dist, dim3((unsigned)a->nq, (unsigned)((a->R + RF_NT - 1) / RF_NT)), dim3(RF_NT), 0, st, a->dX, (long long)a->n, a->D, a->dQ,
                       a->d_qvalid, a->R, a->d_cand_iid, a->d_cand_dist, a->d_cand_cnt, (unsigned long long *)a->d_missing);
    HIPCK(hipGetLastError());
    return a->R <= 512 ? launch_select<512>(a, st) : a->R <= 1024 ? launch_select<1024>(a, st) : launch_select<RF_CAP>(a, st);
}

}  // extern "C"
