"""Numpy twin of mmidx_truncate_l2_device (include/mmidx.h), row by row on np_twin.normalize_l2, and the
rows the tests plant: the ones at which a truncation and its longer sibling part ways, or at which fp64 leaves its normal range."""
import numpy as np

import np_twin as tw


def normalises(T, ncols, mode):
    """0 never, 1 always (PCAProjectionExample.java:83-85), 2 if and only if truncated (IndexTransformation.java:118-120)"""
    return mode == 1 or (mode == 2 and T < ncols)


def truncate_l2(X, lens, normalize):
    """one array [n][T] per target: X[:, :T], every row through Normalization.normalizeL2 where the mode says so"""
    X = np.asarray(X, np.float64)
    outs = []
    for T, mode in zip(lens, normalize):
        Y = np.array(X[:, :T], np.float64, order="C")
        if normalises(T, X.shape[1], mode):
            with np.errstate(all="ignore"):  # (the planted rows overflow and underflow on purpose)
                for r in range(Y.shape[0]):
                    Y[r] = tw.normalize_l2(Y[r])
        outs.append(Y)
    return outs


EDGE_ROWS = 5


def plant_edge_rows(X, r0=1):
    """writes the five edge rows into X[r0 .. r0 + 5) in place (X has at least two columns and r0 + 5 rows) and returns r0:
      r0      the first min(12, ncols - 1) entries zero, the tail not: a short target is all ones, a longer one is not
      r0 + 1  all zero
      r0 + 2  scaled by 1e-170: every square underflows to zero, so every target is all ones
      r0 + 3  scaled by 1e160: the sum overflows, the norm is +inf, every entry a signed zero
      r0 + 4  the first min(33, ncols) entries scaled by 1e-160: subnormal squares that must not be flushed"""
    ncols = X.shape[1]
    assert ncols >= 2 and X.shape[0] >= r0 + EDGE_ROWS
    X[r0, :min(12, ncols - 1)] = 0.0
    assert (X[r0, min(12, ncols - 1):] != 0).all()
    X[r0 + 1] = 0.0
    X[r0 + 2] *= 1e-170
    X[r0 + 3] *= 1e160
    X[r0 + 4, :min(33, ncols)] *= 1e-160
    return r0


def same_bits(a, b):
    a = np.ascontiguousarray(a, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
