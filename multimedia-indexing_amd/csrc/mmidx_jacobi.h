// mmidx_jacobi.h -- the two pieces of the cyclic Jacobi eigen-solver that carry its arithmetic and its order, as plain functions
// that compile for the host (g++, no HIP header) and for the device: the pair schedule and the rotation.  mmidx_dense_solve.h runs
// them inside its kernels; a CPU program can run the same functions in a host loop (tests/test_pca_stream_cpu.py does).
//
// Schedule: round-robin ("circle method", the Brent-Luk parallel ordering).  n = b rounded up to even; a sweep has n - 1 steps of
// n / 2 disjoint pairs; over a sweep every pair {i, j}, i < j < n, appears exactly once.  For odd b the index n - 1 is idle: a pair
// that holds it rotates nothing.
// Rotation: the classical symmetric 2 x 2 one (Rutishauser): t = tan(theta) of the smaller angle that annihilates a_pq.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MMIDX_HD __host__ __device__
#else
#define MMIDX_HD
#endif

namespace mmidx_jacobi {

// b rounded up to an even count of schedule slots
MMIDX_HD inline int slots(int b) { return (b + 1) & ~1; }

// pair k (0 <= k < n / 2) of step s (0 <= s < n - 1), n even and >= 2: *p < *q
MMIDX_HD inline void pair_of(int n, int s, int k, int *p, int *q) {
    int a, c;
    if (k == 0) {
        a = n - 1;
        c = s;
    } else {
        a = (s + k) % (n - 1);
        c = (s - k + (n - 1)) % (n - 1);
    }
    *p = a < c ? a : c;
    *q = a < c ? c : a;
}

struct Rot {
    double c, s, t;  // J = [[c, s], [-s, c]] on (p, q); t = s / c
};

// the rotation that makes (J^T A J)_pq = 0 for the block [[app, apq], [apq, aqq]]; identity where there is nothing to annihilate
MMIDX_HD inline Rot rotation(double app, double aqq, double apq) {
    Rot r;
    r.c = 1.0;
    r.s = 0.0;
    r.t = 0.0;
    if (apq == 0.0) return r;
    const double tau = (aqq - app) / (2.0 * apq);
    const double at = fabs(tau);
    const double t = 1.0 / (at + sqrt(1.0 + at * at));  // (an overflowing tau gives t = 0: the identity)
    r.t = tau < 0.0 ? -t : t;
    r.c = 1.0 / sqrt(1.0 + r.t * r.t);
    r.s = r.t * r.c;
    return r;
}

// rows (or columns) x_p, x_q of one pair under J^T from the left (J from the right): x_p' = c x_p - s x_q, x_q' = s x_p + c x_q
MMIDX_HD inline void rotate(const Rot &r, double *xp, double *xq) {
    const double a = *xp, b = *xq;
    *xp = r.c * a - r.s * b;
    *xq = r.s * a + r.c * b;
}

}  // namespace mmidx_jacobi
