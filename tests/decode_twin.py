"""numpy twin of the record decoder (csrc/mmidx_decode.h): the vector an index holds for a stored record.

For a record with list `cell`, sub-quantizer indices idx[s] and the index's transformation:
  1. z[s * dsub + t] = pq[s][idx[s]][t]
  2. none: y = z;  RandomPermutation (permuted[i] = v[perm[i]]): y[perm[i]] = z[i];
     RandomRotation (rotated[j] = sum_i v[i] R[i][j], R orthogonal): y[i] = sum_j z[j] R[i][j], fp64 from 0.0, j ascending, every
     product rounded before its add (numpy's elementwise * and + never fuse)
  3. IVFPQ: x[d] = coarse[cell][d] - y[d] (the residual is centroid - vector, IVFPQ.java:645);  PQ: x = y
The rotation loops over j, so every output is one sequential sum, whatever the batch."""
import numpy as np

TR_NONE, TR_ROTATION, TR_PERMUTATION = 0, 1, 2


def stored_to_index(codes_stored):
    """stored byte + 128 (PQ.java:555); a short code is the index itself"""
    c = np.asarray(codes_stored)
    return c.astype(np.int64) + 128 if c.dtype == np.int8 else c.astype(np.int64)


def decode(pq, idx, cells=None, coarse=None, transform=TR_NONE, perm=None, rot=None):
    """pq [m][ks][dsub]; idx [n][m] sub-quantizer indices (not the stored bytes); cells [n] and coarse [C][D] for IVFPQ, None for
    PQ.  Returns [n][D] float64."""
    pq = np.asarray(pq, np.float64)
    m, ks, dsub = pq.shape
    D = m * dsub
    idx = np.asarray(idx, np.int64).reshape(-1, m)
    n = idx.shape[0]
    z = pq[np.arange(m)[None, :], idx].reshape(n, D)  # [n][m][dsub] -> [n][D]
    if transform == TR_NONE:
        y = z
    elif transform == TR_PERMUTATION:
        perm = np.asarray(perm, np.int64)
        y = np.empty_like(z)
        y[:, perm] = z
    elif transform == TR_ROTATION:
        R = np.asarray(rot, np.float64).reshape(D, D)
        y = np.zeros((n, D), np.float64)
        for j in range(D):
            y = y + z[:, j:j + 1] * R[None, :, j]
    else:
        raise ValueError(transform)
    if coarse is None:
        return np.ascontiguousarray(y)
    coarse = np.asarray(coarse, np.float64)
    return np.ascontiguousarray(coarse[np.asarray(cells, np.int64)] - y)


def decode_exported(pq, off, iids, codes_stored, want_iids, coarse=None, transform=TR_NONE, perm=None, rot=None):
    """decode the records of `want_iids` from a list-major export (list_off [nlists + 1], iids [n], stored codes [n][m]): the
    list of a record is the last one whose start is <= its position"""
    off = np.asarray(off, np.int64)
    iids = np.asarray(iids, np.int64)
    pos_of = np.full(int(iids.max()) + 1, -1, np.int64)
    pos_of[iids] = np.arange(len(iids))
    pos = pos_of[np.asarray(want_iids, np.int64)]
    assert (pos >= 0).all()
    cells = np.searchsorted(off, pos, side="right") - 1
    idx = stored_to_index(np.asarray(codes_stored)[pos])
    return decode(pq, idx, cells if coarse is not None else None, coarse, transform, perm, rot)
