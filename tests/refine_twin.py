"""Twin of the exact re-ranking (mmidx_search_refine*) for the tests: test infrastructure, never the code
under test.  The candidates are an oracle answer for k = R over the same records; their rows come from the test's own base array,
their distances from np_twin.sq_dists_rows (j ascending, one rounding per operation) and the queue from np_twin.bpq_result."""
import numpy as np

import np_twin as tw


def refine_one(cand, base, q, k, n_lin=None):
    """cand: the internal ids of one compressed answer in its order (count entries, no padding); base[iid] the vector of iid;
    n_lin: rows the Linear index holds (default: all of base).  -> (ids, distances, missing), nearest first."""
    n_lin = len(base) if n_lin is None else n_lin
    cand = np.asarray(cand, np.int64)
    have = (cand >= 0) & (cand < n_lin)
    ids = cand[have]
    if len(ids) == 0:
        return np.zeros(0, np.int32), np.zeros(0), int((~have).sum())
    d = tw.sq_dists_rows(np.asarray(base)[ids], np.asarray(q, np.float64))
    pos = tw.bpq_result(d, k)
    return ids[pos].astype(np.int32), d[pos], int((~have).sum())


def refine_batch(cands, base, Q, k, n_lin=None, known=None):
    """cands = (iids [nq][R], dists, counts) as the oracle's search_batch(Q, R) returns them.  -> (iids [nq][k] padded with -1,
    distances [nq][k] padded with +inf, counts [nq], missing summed).  known[q] False: the query does not exist (count 0, padding,
    nothing missing)."""
    ci, _, cc = cands
    nq = len(cc)
    oi = np.full((nq, k), -1, np.int32)
    od = np.full((nq, k), np.inf)
    oc = np.zeros(nq, np.int32)
    missing = 0
    for q in range(nq):
        if known is not None and not known[q]:
            continue
        i, d, ms = refine_one(ci[q, :cc[q]], base, Q[q], k, n_lin)
        oi[q, :len(i)], od[q, :len(i)], oc[q] = i, d, len(i)
        missing += ms
    return oi, od, oc, missing


def boundary_ties(cands, base, Q, k, n_lin=None):
    """queries whose k-th and (k + 1)-th exact distances among their candidates are equal"""
    ci, _, cc = cands
    out = []
    for q in range(len(cc)):
        _, d, _ = refine_one(ci[q, :cc[q]], base, Q[q], k + 1, n_lin)
        if len(d) == k + 1 and d[k - 1] == d[k]:
            out.append(q)
    return out
