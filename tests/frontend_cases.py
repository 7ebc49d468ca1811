"""Inputs and the derived PCA bound shared by tests/test_gpu_frontend_shapes.py and tests/test_frontend_bound_cpu.py.

PCA projection y_c = sum_k (x_k - mu_k) V_ck over ss terms.  Every fp64 evaluation -- any summation order, blocked or not, with or
without fused multiply-add -- rounds the difference once (1 + d), each product at most once and passes every term through at most
ss - 1 additions: at most ss + 1 roundings per term, so with u = 2^-53

    |y_c - yhat_c| <= ((1 + u)^(ss + 1) - 1) S_c <= (ss + 2) u S_c,     S_c = sum_k |x_k - mu_k| |V_ck|

(the last step holds while (ss + 1) u < 1e-3; ss <= 16384 here).  yhat and S are evaluated in np.longdouble (64-bit significand: their
own error is 2^-11 of the bound).  The bound follows from the length of the sum and the format alone; no measured figure enters it."""
import functools

import numpy as np

import near_ties

# (numComponents, sampleSize, rows, whitening).  129 / 200 / 256 / 300 components: more than one 128-column block of K7, the last one
# ragged; 16384 = a 128 x 128 SIFT VLAD vector; 33: an odd sample length shorter than the component count (the last k tile is one wide)
PCA_SHAPES = [(129, 260, 70, False), (200, 1000, 65, True), (256, 4096, 130, True), (128, 16384, 64, True), (300, 33, 5, False)]


@functools.lru_cache(maxsize=None)
def pca_case(nc, ss, n, whiten):
    """(Vt, mu, eig, X), read-only; the callers fold the whitening into Vt with oracle.pca_whiten"""
    rng = np.random.default_rng(1000 * nc + ss)
    if nc <= ss:
        Vt = np.linalg.qr(rng.standard_normal((ss, nc)))[0].T.copy()  # orthonormal rows
    else:
        Vt = rng.standard_normal((nc, ss)) / np.sqrt(ss)  # (more rows than columns: no orthonormal set exists)
    mu = 0.01 * rng.standard_normal(ss)
    eig = np.sort(rng.uniform(0.5, 4.0, nc))[::-1].copy()
    X = rng.standard_normal((n, ss)) / np.sqrt(ss)
    X[1] = mu  # projects to the zero vector: whitening then yields all ones (Normalization.java:29-30)
    for a in (Vt, mu, eig, X):
        a.setflags(write=False)
    return Vt, mu, eig, X


def pca_exact_and_bound(Vw, mu, X):
    """(yhat [n][nc], bound [n][nc]) as np.longdouble: the projection without normalisation and (ss + 2) 2^-53 S"""
    ss = Vw.shape[1]
    ld = np.longdouble
    Vl = np.asarray(Vw, ld)
    d = np.asarray(X, ld) - np.asarray(mu, ld)
    yhat = np.einsum("ik,ck->ic", d, Vl)  # (rows of both operands contiguous: the fast order for a type without BLAS)
    S = np.einsum("ik,ck->ic", np.abs(d), np.abs(Vl))
    return yhat, ld(ss + 2) * ld(2.0) ** -53 * S


def image_sets(rng, cb, sizes):
    """images of near-tie midpoints of codebook rows, every third row an ordinary one"""
    sets = []
    for n in sizes:
        s = near_ties.midpoints(rng, cb, n) if n else np.zeros((0, cb.shape[1]))
        s[2::3] = rng.standard_normal(s[2::3].shape)
        sets.append(s)
    return sets


def exact_lds_bytes(nc, dl, max_desc):
    """LDS of the `exact` option's block (include/mmidx.h): the codebook, two integer lists of max_desc (rounded up to even, at least
    2), the centroid starts and the reduction words; the call is refused above 160 KiB"""
    maxnd = (max(max_desc, 2) + 1) & ~1
    return nc * dl * 8 + 2 * maxnd * 4 + ((nc + 2) & ~1) * 4 + 32
