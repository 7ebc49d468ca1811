// mmidx_small_solve.h -- the two dense b x b solves of the PCA learner's subspace iteration, plain C++ on the host
// (b = numComponents + 32 <= 1056; DESIGN.md section 5.6 gives their measured times):
//   chol_inverse   S = L L^T, returns L^-1 (CholeskyQR: Q = Z L^-T); a pivot at rounding level marks the column as deficient
//   sym_eig        all eigenpairs of a symmetric matrix: Householder tridiagonalisation + implicit QL (the EISPACK tred2 / tql2
//                  pair in the public-domain JAMA formulation), eigenvalues descending, eigenvectors as ROWS
// No dependency beyond the C++ library (libmmidx_hip.so links -ldl only).
#pragma once
#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

namespace mmidx_small {

// every entry finite?  Both solves below check it first: a NaN never passes the deflation test of the QL sweep.
inline bool all_finite(const double *A, size_t count) {
    for (size_t i = 0; i < count; i++)
        if (!std::isfinite(A[i])) return false;
    return true;
}

// S[b][b] (row-major, lower triangle read) -> Linv[b][b] (lower triangular, zeros above).  Column j whose pivot is <= thr_rel * max diag
// is listed in `deficient` (false, nothing written, when S holds a non-finite entry): its L column becomes e_j, so that Q_j = Z_j minus its projections (the caller replaces it).
inline bool chol_inverse(const double *S, int b, double thr_rel, std::vector<double> &Linv, std::vector<int> &deficient) {
    deficient.clear();
    if (!all_finite(S, (size_t)b * b)) return false;
    std::vector<double> L((size_t)b * b, 0.0);
    double dmax = 0.0;
    for (int j = 0; j < b; j++) dmax = std::max(dmax, S[(size_t)j * b + j]);
    const double thr = thr_rel * dmax;
    std::vector<char> bad((size_t)b, 0);
    for (int j = 0; j < b; j++) {
        double *Lj = L.data() + (size_t)j * b;
        double d = S[(size_t)j * b + j];
        for (int k = 0; k < j; k++) d -= Lj[k] * Lj[k];
        if (!(d > thr)) {
            bad[(size_t)j] = 1;
            deficient.push_back(j);
            Lj[j] = 1.0;
            continue;  // rows below keep L[i][j] = 0
        }
        const double ljj = std::sqrt(d);
        Lj[j] = ljj;
        for (int i = j + 1; i < b; i++) {
            double *Li = L.data() + (size_t)i * b;
            double s = S[(size_t)i * b + j];
            for (int k = 0; k < j; k++) s -= Li[k] * Lj[k];
            Li[j] = s / ljj;
        }
    }
    // X = L^-1, built by rows: X[i][j] = -(sum_{k=j}^{i-1} L[i][k] X[k][j]) / L[i][i]; Xt holds X transposed so the sum runs over
    // contiguous memory
    std::vector<double> Xt((size_t)b * b, 0.0);  // Xt[j][i] = X[i][j]
    for (int j = 0; j < b; j++) {
        double *xj = Xt.data() + (size_t)j * b;
        xj[j] = 1.0 / L[(size_t)j * b + j];
        for (int i = j + 1; i < b; i++) {
            const double *Li = L.data() + (size_t)i * b;
            double s = 0.0;
            for (int k = j; k < i; k++) s += Li[k] * xj[k];
            xj[i] = -s / Li[i];
        }
    }
    Linv.assign((size_t)b * b, 0.0);
    for (int j = 0; j < b; j++)
        for (int i = j; i < b; i++) Linv[(size_t)i * b + j] = Xt[(size_t)j * b + i];
    return true;
}

// A[n][n] symmetric (row-major), finite -> lam[n] descending, Wt[n][n] with row i = unit eigenvector of lam[i].
// false (nothing written) when A holds a non-finite entry.
inline bool sym_eig(const double *A, int n, std::vector<double> &lam, std::vector<double> &Wt) {
    if (!all_finite(A, (size_t)n * n)) return false;
    std::vector<double> V(A, A + (size_t)n * n), d((size_t)n, 0.0), e((size_t)n, 0.0);
    auto v = [&](int i, int j) -> double & { return V[(size_t)i * n + j]; };
    // ---- tred2 ----
    for (int j = 0; j < n; j++) d[j] = v(n - 1, j);
    for (int i = n - 1; i > 0; i--) {
        double scale = 0.0, h = 0.0;
        for (int k = 0; k < i; k++) scale += std::fabs(d[k]);
        if (scale == 0.0) {
            e[i] = d[i - 1];
            for (int j = 0; j < i; j++) {
                d[j] = v(i - 1, j);
                v(i, j) = 0.0;
                v(j, i) = 0.0;
            }
        } else {
            for (int k = 0; k < i; k++) {
                d[k] /= scale;
                h += d[k] * d[k];
            }
            double f = d[i - 1];
            double g = std::sqrt(h);
            if (f > 0) g = -g;
            e[i] = scale * g;
            h = h - f * g;
            d[i - 1] = f - g;
            for (int j = 0; j < i; j++) e[j] = 0.0;
            for (int j = 0; j < i; j++) {
                f = d[j];
                v(j, i) = f;
                g = e[j] + v(j, j) * f;
                for (int k = j + 1; k <= i - 1; k++) {
                    g += v(k, j) * d[k];
                    e[k] += v(k, j) * f;
                }
                e[j] = g;
            }
            f = 0.0;
            for (int j = 0; j < i; j++) {
                e[j] /= h;
                f += e[j] * d[j];
            }
            const double hh = f / (h + h);
            for (int j = 0; j < i; j++) e[j] -= hh * d[j];
            for (int j = 0; j < i; j++) {
                f = d[j];
                g = e[j];
                for (int k = j; k <= i - 1; k++) v(k, j) -= (f * e[k] + g * d[k]);
                d[j] = v(i - 1, j);
                v(i, j) = 0.0;
            }
        }
        d[i] = h;
    }
    for (int i = 0; i < n - 1; i++) {
        v(n - 1, i) = v(i, i);
        v(i, i) = 1.0;
        const double h = d[i + 1];
        if (h != 0.0) {
            for (int k = 0; k <= i; k++) d[k] = v(k, i + 1) / h;
            for (int j = 0; j <= i; j++) {
                double g = 0.0;
                for (int k = 0; k <= i; k++) g += v(k, i + 1) * v(k, j);
                for (int k = 0; k <= i; k++) v(k, j) -= g * d[k];
            }
        }
        for (int k = 0; k <= i; k++) v(k, i + 1) = 0.0;
    }
    for (int j = 0; j < n; j++) {
        d[j] = v(n - 1, j);
        v(n - 1, j) = 0.0;
    }
    v(n - 1, n - 1) = 1.0;
    e[0] = 0.0;
    // ---- tql2 on the transposed accumulator (a rotation then mixes two contiguous rows) ----
    std::vector<double> U((size_t)n * n);  // U[i][k] = V[k][i]
    for (int i = 0; i < n; i++)
        for (int k = 0; k < n; k++) U[(size_t)i * n + k] = V[(size_t)k * n + i];
    for (int i = 1; i < n; i++) e[i - 1] = e[i];
    e[n - 1] = 0.0;
    double f = 0.0, tst1 = 0.0;
    const double eps = 0x1p-52;
    for (int l = 0; l < n; l++) {
        tst1 = std::max(tst1, std::fabs(d[l]) + std::fabs(e[l]));
        int m = l;
        while (m < n - 1) {  // (e[n - 1] = 0 ends the search on finite input; the bound holds whatever the input)
            if (std::fabs(e[m]) <= eps * tst1) break;
            m++;
        }
        if (m > l) {
            int iter = 0;
            do {
                iter++;
                double g = d[l];
                double p = (d[l + 1] - g) / (2.0 * e[l]);
                double r = std::hypot(p, 1.0);
                if (p < 0) r = -r;
                d[l] = e[l] / (p + r);
                d[l + 1] = e[l] * (p + r);
                const double dl1 = d[l + 1];
                double h = g - d[l];
                for (int i = l + 2; i < n; i++) d[i] -= h;
                f += h;
                p = d[m];
                double c = 1.0, c2 = c, c3 = c;
                const double el1 = e[l + 1];
                double s = 0.0, s2 = 0.0;
                for (int i = m - 1; i >= l; i--) {
                    c3 = c2;
                    c2 = c;
                    s2 = s;
                    g = c * e[i];
                    h = c * p;
                    r = std::hypot(p, e[i]);
                    e[i + 1] = s * r;
                    s = e[i] / r;
                    c = p / r;
                    p = c * d[i] - s * g;
                    d[i + 1] = h + s * (c * g + s * d[i]);
                    double *u0 = U.data() + (size_t)i * n, *u1 = u0 + n;
                    for (int k = 0; k < n; k++) {
                        const double hk = u1[k];
                        u1[k] = s * u0[k] + c * hk;
                        u0[k] = c * u0[k] - s * hk;
                    }
                }
                p = -s * s2 * c3 * el1 * e[l] / dl1;
                e[l] = s * p;
                d[l] = c * p;
            } while (std::fabs(e[l]) > eps * tst1 && iter < 300);
        }
        d[l] = d[l] + f;
        e[l] = 0.0;
    }
    // descending order (stable: equal eigenvalues keep their position)
    std::vector<int> ord((size_t)n);
    std::iota(ord.begin(), ord.end(), 0);
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return d[a] > d[b]; });
    lam.resize((size_t)n);
    Wt.resize((size_t)n * n);
    for (int i = 0; i < n; i++) {
        lam[i] = d[ord[i]];
        std::copy(U.begin() + (size_t)ord[i] * n, U.begin() + (size_t)(ord[i] + 1) * n, Wt.begin() + (size_t)i * n);
    }
    return true;
}

}  // namespace mmidx_small
