// mmidx_frontend.hip -- front end of BASELINE config 5: PCA projection (K7) and VLAD aggregation (K8, K8', K8''), and
// mmidx_vectorize, which chains them.  The one unit that includes mmidx_frontend.h.
#include "mmidx_frontend.h"
#include "mmidx_host.h"

#include <algorithm>
#include <cmath>
#include <mutex>
#include <string>
#include <vector>

struct MMIDX_HIDDEN mmidx_pca {
    std::mutex mu;  // host-pointer calls share the workspaces
    int nc = 0, ss = 0, whitening = 0, device = 0;
    Stream stream;  // (before what is used on it: members are destroyed in reverse order)
    DevPtr<double> d_mu, d_Vt;
    DevBuf<double> ws_X, ws_Y;
};
struct MMIDX_HIDDEN mmidx_vlad {
    std::mutex mu;  // host-pointer calls share the workspaces
    int nvocab = 0, dl = 0, norms = 0, device = 0, veclen = 0;
    std::vector<int> nc;
    std::vector<size_t> cb_off;  // element offset of each codebook
    Stream stream;  // (before what is used on it: members are destroyed in reverse order)
    DevPtr<double> d_cb;
    DevBuf<double> ws_desc, ws_out;
    DevBuf<long long> ws_off;
    // K8': the assignment of every descriptor of a launch through the encoder's certified MFMA argmin -- one hidden index handle
    // per vocabulary whose "coarse quantizer" is the vocabulary
    std::vector<mmidx_index *> asg;
    DevBuf<int32_t> ws_nn;
    int exact = 0;  // option "exact": the one-kernel form (k_vlad: fp64 brute-force assignment inside the block)
    int two_pass = 0;  // option "two_pass": K8' also where K8'' (k_vlad_fused) applies
};

extern "C" {

int mmidx_pca_create(int nc, int ss, int whitening, const double *means, const double *eig, const double *Vt, int device,
                     mmidx_pca **out) {
    if (!out) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null out pointer");
    *out = nullptr;
    if (nc < 1 || ss < 1 || !means || !Vt) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "bad PCA shape or null matrix");
    if (whitening && !eig) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "whitening needs the eigenvalues line of the PCA file");
    const int ndev = mmidx_device_count();
    if (ndev < 1) return mmidx_fail(MMIDX_ERR_NO_DEVICE, "no HIP device: libmmidx_hip has no CPU fallback");
    if (device < 0 || device >= ndev) return mmidx_fail(MMIDX_ERR_NO_DEVICE, "device %d outside 0..%d", device, ndev - 1);
    HIPCK(hipSetDevice(device));
    std::unique_ptr<mmidx_pca> p(new mmidx_pca());
    p->nc = nc;
    p->ss = ss;
    p->whitening = whitening ? 1 : 0;
    p->device = device;
    std::vector<double> V((size_t)nc * ss);
    for (int i = 0; i < nc; i++) {
        // W(i,i) = pow(eig_i, -0.5); V_t <- W * V_t  (PCA.java:283-285, :311): row i scaled by w_ii
        const double wv = whitening ? std::pow(eig[i], -0.5) : 1.0;
        for (int j = 0; j < ss; j++) V[(size_t)i * ss + j] = whitening ? wv * Vt[(size_t)i * ss + j] : Vt[(size_t)i * ss + j];
    }
    HIPCK(p->stream.create());
    HIPCK(p->d_mu.alloc((size_t)ss));
    HIPCK(p->d_Vt.alloc((size_t)nc * ss));
    HIPCK(hipMemcpy(p->d_mu, means, (size_t)ss * 8, hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(p->d_Vt, V.data(), (size_t)nc * ss * 8, hipMemcpyHostToDevice));
    *out = p.release();
    return MMIDX_OK;
}

int mmidx_pca_get_dims(const mmidx_pca *p, int *nc_out, int *ss_out) {
    if (!p) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null handle");
    if (nc_out) *nc_out = p->nc;
    if (ss_out) *ss_out = p->ss;
    return MMIDX_OK;
}

int mmidx_internal_pca_device(const mmidx_pca *p) { return p->device; }  // (mmidx_linear_reindex checks it against its handles')

int mmidx_pca_destroy(mmidx_pca *p) {
    if (!p) return MMIDX_OK;
    (void)hipSetDevice(p->device);
    delete p;
    return MMIDX_OK;
}

int mmidx_pca_project_device(mmidx_pca *p, int64_t n, const double *dX, double *dY, void *stream) {
    if (!p) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null handle");
    if (n < 0 || (n > 0 && (!dX || !dY))) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null argument");
    if (n == 0) return MMIDX_OK;
    HIPCK(hipSetDevice(p->device));
    hipStream_t st = (hipStream_t)stream;
    dim3 grid((unsigned)((n + PCA_BM - 1) / PCA_BM), (unsigned)((p->nc + PCA_BN - 1) / PCA_BN));
    HIPCK(hipFuncSetAttribute((const void *)k_pca_project, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PCA_LDS_BYTES));
    hipLaunchKernelGGL(k_pca_project, grid, dim3(PCA_NT), PCA_LDS_BYTES, st, dX, p->d_mu, p->d_Vt, dY, (long long)n, p->nc, p->ss);
    if (p->whitening)
        hipLaunchKernelGGL(k_rows_normalize_l2, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dY, (long long)n, p->nc);
    HIPCK(hipGetLastError());
    return MMIDX_OK;
}

// for mmidx_pca_learn.hip (declared in mmidx_host.h): K7 on plain device pointers, the tall products of the PCA learner's
// subspace iteration
int mmidx_internal_gemm_nt(const double *X, const double *mu, const double *Vt, double *Y, long long n, int nc, int ss, void *stream) {
    dim3 grid((unsigned)((n + PCA_BM - 1) / PCA_BM), (unsigned)((nc + PCA_BN - 1) / PCA_BN));
    static_assert(PCA_LDS_BYTES <= 64 * 1024, "K7's tiles fit the default dynamic LDS limit: no attribute to raise per launch");
    hipLaunchKernelGGL(k_pca_project, grid, dim3(PCA_NT), PCA_LDS_BYTES, (hipStream_t)stream, X, mu, Vt, Y, n, nc, ss);
    HIPCK(hipGetLastError());
    return MMIDX_OK;
}

int mmidx_pca_project(mmidx_pca *p, int64_t n, const double *X, double *Y) {
    if (!p) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null handle");
    if (n < 0 || (n > 0 && (!X || !Y))) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null argument");
    std::lock_guard<std::mutex> lk(p->mu);
    HIPCK(hipSetDevice(p->device));
    const int64_t B = std::max<int64_t>(1, (int64_t)(1ll << 28) / p->ss);  // <= 2 GiB of samples per round
    for (int64_t i0 = 0; i0 < n; i0 += B) {
        const int64_t nb = std::min(B, n - i0);
        HIPCK(p->ws_X.reserve((size_t)nb * p->ss));
        HIPCK(p->ws_Y.reserve((size_t)nb * p->nc));
        HIPCK(hipMemcpyAsync(p->ws_X.p, X + (size_t)i0 * p->ss, (size_t)nb * p->ss * 8, hipMemcpyHostToDevice, p->stream));
        int rc = mmidx_pca_project_device(p, nb, p->ws_X.p, p->ws_Y.p, p->stream);
        if (rc) return rc;
        HIPCK(hipMemcpyAsync(Y + (size_t)i0 * p->nc, p->ws_Y.p, (size_t)nb * p->nc * 8, hipMemcpyDeviceToHost, p->stream));
        HIPCK(hipStreamSynchronize(p->stream));
    }
    return MMIDX_OK;
}

int mmidx_vlad_create(int nvocab, const int32_t *ncent, int dl, const double *codebooks, int normalizations_on, int device,
                      mmidx_vlad **out) {
    if (!out) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null out pointer");
    *out = nullptr;
    if (nvocab < 1 || !ncent || dl < 1 || !codebooks) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "bad codebook description");
    const int ndev = mmidx_device_count();
    if (ndev < 1) return mmidx_fail(MMIDX_ERR_NO_DEVICE, "no HIP device: libmmidx_hip has no CPU fallback");
    if (device < 0 || device >= ndev) return mmidx_fail(MMIDX_ERR_NO_DEVICE, "device %d outside 0..%d", device, ndev - 1);
    HIPCK(hipSetDevice(device));
    std::unique_ptr<mmidx_vlad> v(new mmidx_vlad());
    v->nvocab = nvocab;
    v->dl = dl;
    v->norms = normalizations_on ? 1 : 0;
    v->device = device;
    size_t tot = 0;
    for (int i = 0; i < nvocab; i++) {
        if (ncent[i] < 1) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "empty codebook");
        v->nc.push_back(ncent[i]);
        v->cb_off.push_back(tot);
        tot += (size_t)ncent[i] * dl;
    }
    v->veclen = (int)tot;
    HIPCK(v->stream.create());
    HIPCK(v->d_cb.alloc(tot));
    HIPCK(hipMemcpy(v->d_cb, codebooks, tot * 8, hipMemcpyHostToDevice));
    for (int i = 0; i < nvocab; i++) {  // (a vocabulary the assignment kernels cannot take leaves its slot empty: k_vlad serves it)
        mmidx_index *a = nullptr;
        if (ncent[i] >= 2) {
            int rca = mmidx_create(MMIDX_KIND_IVFPQ, dl, 1, 2, ncent[i], MMIDX_TR_NONE, nullptr, nullptr, device, &a);
            if (rca == MMIDX_OK) rca = mmidx_set_coarse(a, codebooks + v->cb_off[(size_t)i]);
            if (rca != MMIDX_OK) {  // the slot falls back to k_vlad: not an error of this call, so no stale message either
                if (a) mmidx_destroy(a);
                a = nullptr;
                mmidx_clear_error();
            }
        }
        v->asg.push_back(a);
    }
    *out = v.release();
    return MMIDX_OK;
}

int mmidx_vlad_set_option(mmidx_vlad *v, const char *name, int value) {
    if (!v || !name) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null argument");
    if (std::string(name) == "exact") {
        v->exact = value != 0;
        return MMIDX_OK;
    }
    if (std::string(name) == "two_pass") {  // K8' (assignment kernel + accumulation kernel) also where the one-kernel form K8'' applies (A/B switch)
        v->two_pass = value != 0;
        return MMIDX_OK;
    }
    return mmidx_fail(MMIDX_ERR_INVALID_ARG, "unknown option '%s'", name);
}

int mmidx_vlad_destroy(mmidx_vlad *v) {
    if (!v) return MMIDX_OK;
    (void)hipSetDevice(v->device);
    for (mmidx_index *a : v->asg)
        if (a) mmidx_destroy(a);
    delete v;
    return MMIDX_OK;
}

int mmidx_vlad_descriptor_length(const mmidx_vlad *v, int *dl_out) {
    if (!v || !dl_out) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null argument");
    *dl_out = v->dl;
    return MMIDX_OK;
}

int mmidx_vlad_vector_length(const mmidx_vlad *v, int *len_out) {
    if (!v || !len_out) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null argument");
    *len_out = v->veclen;
    return MMIDX_OK;
}

// max_desc: largest descriptor count of any image in the batch (sizes the LDS work lists)
int mmidx_vlad_aggregate_device(mmidx_vlad *v, int64_t nimg, const int64_t *d_desc_off, const double *d_descs, int max_desc,
                                double *d_out, void *stream) {
    if (!v) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null handle");
    if (nimg < 0 || (nimg > 0 && (!d_desc_off || !d_out))) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null argument");
    if (nimg == 0) return MMIDX_OK;
    HIPCK(hipSetDevice(v->device));
    hipStream_t st = (hipStream_t)stream;
    const int maxnd = (std::max(max_desc, 2) + 1) & ~1;
    long long ndesc = -1;  // descriptors of the launch (read back once when the assignment runs as its own stage)
    for (int i = 0; i < v->nvocab; i++) {
        const int nc = v->nc[(size_t)i];
        if (!v->exact && !v->two_pass && v->asg[(size_t)i] && d_descs && v->dl == 64 && nc <= 128 && ((uintptr_t)d_descs & 15) == 0) {
            // K8'': one kernel, one pass over the descriptors in HBM, no host synchronisation (the flagged descriptors are redone by the
            // image's own block): 64-dimensional descriptors, vocabularies of at most 128 centroids.  It reads rows as double2, so a
            // base that is only 8-byte aligned goes to K8', whose kernels read single doubles (as assign_device gates its FROMX form)
            MmidxCoarseTables a;
            int rct = mmidx_internal_coarse_tables(v->asg[(size_t)i], &a);
            if (rct) return rct;
            if (a.Ch && a.Cp == G16_BC && a.Dp >= 64 && a.Dp <= G16_KC) {
                const size_t lf = 2 * (size_t)G16_BC * (64 * 2 + 16) + 2 * (size_t)maxnd * 4 + (size_t)((nc + 2) & ~1) * 4 + (size_t)(VF_FLAG_CAP + 2) * 4 + 32;
                if (lf <= 160 * 1024 && a.coarseT) {
                    HIPCK(hipFuncSetAttribute((const void *)k_vlad_fused, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lf));
                    hipLaunchKernelGGL(k_vlad_fused, dim3((unsigned)nimg), dim3(256), lf, st, v->d_cb + v->cb_off[(size_t)i], a.coarseT, nc, maxnd, (const __bf16 *)a.Ch,
                                       (const __bf16 *)a.Cl, a.cn_pad, a.cnorm_max, a.cn_max, a.Dp, (const long long *)d_desc_off, d_descs, d_out, v->veclen,
                                       (int)v->cb_off[(size_t)i], v->norms);
                    HIPCK(hipGetLastError());
                    continue;
                }
            }
        }
        if (!v->exact && v->asg[(size_t)i] && d_descs) {
            // K8': nearest centroid of EVERY descriptor on the matrix cores (certified, exact redo of the flagged few), then one
            // block per image for the ordered accumulation
            if (ndesc < 0) {
                HIPCK(hipMemcpyAsync(&ndesc, d_desc_off + nimg, sizeof(long long), hipMemcpyDeviceToHost, st));
                HIPCK(hipStreamSynchronize(st));
                HIPCK(v->ws_nn.reserve((size_t)std::max<long long>(ndesc, 1)));
            }
            if (ndesc > 0) {
                int rca = mmidx_assign_device(v->asg[(size_t)i], ndesc, d_descs, v->ws_nn.p, st);
                if (rca) return rca;
                HIPCK(hipSetDevice(v->device));
            }
            const size_t lds2 = 2 * (size_t)maxnd * 4 + (size_t)((nc + 2) & ~1) * 4 + 32;
            if (lds2 > 64 * 1024) return mmidx_fail(MMIDX_ERR_UNSUPPORTED, "%d descriptors per image exceed the accumulation kernel's LDS", max_desc);
            if (v->dl == 64)
                hipLaunchKernelGGL(k_vlad_accum<64>, dim3((unsigned)nimg), dim3(256), lds2, st, v->d_cb + v->cb_off[(size_t)i], nc, v->dl, maxnd, v->ws_nn.p,
                                   (const long long *)d_desc_off, d_descs, d_out, v->veclen, (int)v->cb_off[(size_t)i], v->norms);
            else
                hipLaunchKernelGGL(k_vlad_accum<0>, dim3((unsigned)nimg), dim3(256), lds2, st, v->d_cb + v->cb_off[(size_t)i], nc, v->dl, maxnd, v->ws_nn.p,
                                   (const long long *)d_desc_off, d_descs, d_out, v->veclen, (int)v->cb_off[(size_t)i], v->norms);
            HIPCK(hipGetLastError());
            continue;
        }
        const size_t lds = (size_t)nc * v->dl * 8 + 2 * (size_t)maxnd * 4 + (size_t)((nc + 2) & ~1) * 4 + 32;
        if (lds > 160 * 1024)
            return mmidx_fail(MMIDX_ERR_UNSUPPORTED, "codebook %d x %d plus %d descriptors per image exceed the 160 KiB LDS", nc, v->dl, max_desc);
        const int norms = v->norms;
        if (v->dl == 64) {
            HIPCK(hipFuncSetAttribute((const void *)k_vlad<64>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(k_vlad<64>, dim3((unsigned)nimg), dim3(256), lds, st, v->d_cb + v->cb_off[(size_t)i], nc, v->dl, maxnd,
                               (const long long *)d_desc_off, d_descs, d_out, v->veclen, (int)v->cb_off[(size_t)i], norms);
        } else {
            HIPCK(hipFuncSetAttribute((const void *)k_vlad<0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(k_vlad<0>, dim3((unsigned)nimg), dim3(256), lds, st, v->d_cb + v->cb_off[(size_t)i], nc, v->dl, maxnd,
                               (const long long *)d_desc_off, d_descs, d_out, v->veclen, (int)v->cb_off[(size_t)i], norms);
        }
    }
    if (v->nvocab > 1 && v->norms)
        hipLaunchKernelGGL(k_rows_normalize_l2_block, dim3((unsigned)nimg), dim3(256), 0, st, d_out, v->veclen);
    HIPCK(hipGetLastError());
    return MMIDX_OK;
}

int mmidx_vlad_aggregate(mmidx_vlad *v, int64_t nimg, const int64_t *desc_off, const double *descs, double *out) {
    if (!v) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null handle");
    if (nimg < 0 || (nimg > 0 && (!desc_off || !out))) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null argument");
    if (nimg == 0) return MMIDX_OK;
    std::lock_guard<std::mutex> lk(v->mu);
    HIPCK(hipSetDevice(v->device));
    const int64_t total = desc_off[nimg] - desc_off[0];
    if (total > 0 && !descs) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null descriptors");
    int max_desc = 0;
    std::vector<long long> off((size_t)nimg + 1);
    for (int64_t i = 0; i <= nimg; i++) off[(size_t)i] = desc_off[i] - desc_off[0];
    for (int64_t i = 0; i < nimg; i++) max_desc = std::max<int>(max_desc, (int)(off[(size_t)i + 1] - off[(size_t)i]));
    HIPCK(v->ws_off.reserve((size_t)nimg + 1));
    HIPCK(v->ws_desc.reserve((size_t)std::max<int64_t>(total, 1) * v->dl));
    HIPCK(v->ws_out.reserve((size_t)nimg * v->veclen));
    HIPCK(hipMemcpyAsync(v->ws_off.p, off.data(), ((size_t)nimg + 1) * 8, hipMemcpyHostToDevice, v->stream));
    if (total > 0)
        HIPCK(hipMemcpyAsync(v->ws_desc.p, descs + (size_t)desc_off[0] * v->dl, (size_t)total * v->dl * 8, hipMemcpyHostToDevice, v->stream));
    int rc = mmidx_vlad_aggregate_device(v, nimg, (const int64_t *)v->ws_off.p, v->ws_desc.p, max_desc, v->ws_out.p, v->stream);
    if (rc) return rc;
    HIPCK(hipMemcpyAsync(out, v->ws_out.p, (size_t)nimg * v->veclen * 8, hipMemcpyDeviceToHost, v->stream));
    HIPCK(hipStreamSynchronize(v->stream));
    return MMIDX_OK;
}

// ImageVectorization.transformToVector (J/vectorization/ImageVectorization.java:169-208) for a batch: aggregate, then
// PCA.sampleToEigenSpace -- descriptors in, projected vectors out, the VLAD vectors never leave the device
int mmidx_vectorize_device(mmidx_vlad *v, mmidx_pca *p, int64_t nimg, const int64_t *d_desc_off, const double *d_descs, int max_desc,
                           double *d_out, void *stream) {
    if (!v || !p) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null handle");
    if (v->veclen != p->ss)
        return mmidx_fail(MMIDX_ERR_WRONG_DIM, "VLAD vector length %d does not match the PCA sample size %d", v->veclen, p->ss);
    if (v->device != p->device) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "aggregator and PCA live on different devices");
    if (nimg < 0 || (nimg > 0 && (!d_desc_off || !d_out))) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null argument");
    if (nimg == 0) return MMIDX_OK;
    HIPCK(hipSetDevice(v->device));
    const int64_t B = std::max<int64_t>(1, (int64_t)(1ll << 28) / v->veclen);  // <= 2 GiB of VLAD vectors per round
    for (int64_t i0 = 0; i0 < nimg; i0 += B) {
        const int64_t nb = std::min(B, nimg - i0);
        HIPCK(v->ws_out.reserve((size_t)nb * v->veclen));
        // (the offsets are absolute into d_descs: a sub-range of images needs no rebasing)
        int rc = mmidx_vlad_aggregate_device(v, nb, d_desc_off + i0, d_descs, max_desc, v->ws_out.p, stream);
        if (rc) return rc;
        rc = mmidx_pca_project_device(p, nb, v->ws_out.p, d_out + (size_t)i0 * p->nc, stream);
        if (rc) return rc;
    }
    return MMIDX_OK;
}

int mmidx_vectorize(mmidx_vlad *v, mmidx_pca *p, int64_t nimg, const int64_t *desc_off, const double *descs, double *out) {
    if (!v || !p) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null handle");
    if (nimg < 0 || (nimg > 0 && (!desc_off || !out))) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null argument");
    if (nimg == 0) return MMIDX_OK;
    std::lock_guard<std::mutex> lk(v->mu);
    std::lock_guard<std::mutex> lk2(p->mu);
    HIPCK(hipSetDevice(v->device));
    const int64_t total = desc_off[nimg] - desc_off[0];
    if (total > 0 && !descs) return mmidx_fail(MMIDX_ERR_INVALID_ARG, "null descriptors");
    int max_desc = 0;
    std::vector<long long> off((size_t)nimg + 1);
    for (int64_t i = 0; i <= nimg; i++) off[(size_t)i] = desc_off[i] - desc_off[0];
    for (int64_t i = 0; i < nimg; i++) max_desc = std::max<int>(max_desc, (int)(off[(size_t)i + 1] - off[(size_t)i]));
    HIPCK(v->ws_off.reserve((size_t)nimg + 1));
    HIPCK(v->ws_desc.reserve((size_t)std::max<int64_t>(total, 1) * v->dl));
    HIPCK(p->ws_Y.reserve((size_t)nimg * p->nc));
    HIPCK(hipMemcpyAsync(v->ws_off.p, off.data(), ((size_t)nimg + 1) * 8, hipMemcpyHostToDevice, v->stream));
    if (total > 0)
        HIPCK(hipMemcpyAsync(v->ws_desc.p, descs + (size_t)desc_off[0] * v->dl, (size_t)total * v->dl * 8, hipMemcpyHostToDevice, v->stream));
    int rc = mmidx_vectorize_device(v, p, nimg, (const int64_t *)v->ws_off.p, v->ws_desc.p, max_desc, p->ws_Y.p, v->stream);
    if (rc) return rc;
    HIPCK(hipMemcpyAsync(out, p->ws_Y.p, (size_t)nimg * p->nc * 8, hipMemcpyDeviceToHost, v->stream));
    HIPCK(hipStreamSynchronize(v->stream));
    return MMIDX_OK;
}

}  // extern "C"
