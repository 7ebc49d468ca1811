"""Near-tie inputs for the certified coarse / assignment filters, and the magnitude sweep they are run at.

A filter row is decided by `second - best > 2 eps`.  A query in the middle of two neighbouring centroids, a relative 1e-3 off the
exact middle, has its two nearest centroids a few 1e-3 apart in distance: far from an fp64 tie (the reference's argmin is unique and
no tie rule is involved), and close enough that a bound which is too small anywhere certifies the wrong one of the two.
Everything is generated at unit scale from a seed; the callers multiply rows and centroids by the scale under test."""
import numpy as np

# 1e-17 .. 1e-25 in half decades: between "every fp32 square is normal" and "every fp32 square is zero"
BAND = [10.0 ** (-e / 2.0) for e in range(34, 51)]
ORDINARY = [1e-9, 1.0, 1e9]
SWEEP = BAND + ORDINARY


def sqdist(X, C):
    """[n][C] squared distances in fp64 (matrix form: good to 1e-15 of the norms, used for ranking only)"""
    return (X * X).sum(1)[:, None] + (C * C).sum(1)[None, :] - 2.0 * (X @ C.T)


def midpoints(rng, C, n, spread=1e-3):
    """n rows t c_a + (1 - t) c_b, c_b the nearest other centroid of a random c_a, t = 0.5 + spread N(0, 1)"""
    a = rng.integers(0, C.shape[0], n)
    d = sqdist(C[a], C)
    d[np.arange(n), a] = np.inf
    b = d.argmin(1)
    t = 0.5 + spread * rng.standard_normal(n)
    return t[:, None] * C[a] + (1.0 - t)[:, None] * C[b]


def problem(D, C, n, seed):
    """(centroids [C][D], rows [n][D]) at unit scale: Gaussian centroids and near-tie rows between neighbouring ones"""
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((C, D))
    return cent, midpoints(rng, cent, n)


def tie_at_rank(rng, cent, Q, k, count, spread=1e-3):
    """A copy of the centroids in which, for rows of Q, the k-th and
    (k+1)-th nearest centroids (1-based) are replaced by q + r u1 and q + r (1 + delta) u2: r the k-th nearest distance, u1 / u2
    random unit vectors, delta = spread N(0, 1).  The ranks k and k + 1 of the row then differ by a relative 2 delta in squared
    distance and everything else keeps its rank.  The first `count` rows of Q whose two centroids no earlier row has taken are used
    (no centroid is replaced twice); returns the new centroids and those rows."""
    cent = cent.copy()
    order = np.argsort(sqdist(Q, cent), axis=1)
    used = set()
    keep = []
    for i in range(len(Q)):
        a, b = int(order[i, k - 1]), int(order[i, k])
        if a in used or b in used or len(keep) == count:
            continue
        used.update((a, b))
        r = float(np.sqrt(((Q[i] - cent[a]) ** 2).sum()))
        u = rng.standard_normal((2, cent.shape[1]))
        u /= np.linalg.norm(u, axis=1)[:, None]
        cent[a] = Q[i] + r * u[0]
        cent[b] = Q[i] + r * (1.0 + spread * rng.standard_normal()) * u[1]
        keep.append(i)
    return cent, Q[keep]
