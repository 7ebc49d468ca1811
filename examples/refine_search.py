"""Exact re-ranking of IVFPQ answers against a Linear index over the same vectors (mmidx_search_refine).

The reference's deployment keeps both structures (IndexTransformation.java:61-125 builds the compressed index from the Linear one,
Example.java:155-182 compares their answers).  Here the comparison becomes a search: the R best records by code distance meet
their full vectors on the GPU and the k best by exact distance come back -- one call, nothing crosses the bus in between.

    python examples/refine_search.py [--n 30000] [--dim 64] [--k 10] [--R 50 200]"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=30000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--R", type=int, nargs="+", default=[50, 200])
    ap.add_argument("--nq", type=int, default=500)
    a = ap.parse_args()
    mi = importlib.import_module("multimedia-indexing_amd")
    rng = np.random.default_rng(0)
    n, D, k = a.n, a.dim, a.k
    centers = rng.standard_normal((64, D)) * 2.0
    X = centers[rng.integers(0, 64, n)] + rng.standard_normal((n, D))
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    ids = [f"img{i}" for i in range(n)]

    # codebooks from a sample, as examples/index_transformation.py draws them
    m, ks, C_ = 8, 256, 64
    coarse = X[rng.choice(n, C_, replace=False)]
    resid = coarse[((X[:4096, None, :] - coarse[None]) ** 2).sum(-1).argmin(1)] - X[:4096]  # centroid - vector, IVFPQ.java:645
    pq = np.stack([resid[rng.choice(4096, ks, replace=False), j * (D // m):(j + 1) * (D // m)] for j in range(m)])
    ivf = mi.IVFPQ(D, n, False, "", m, ks, mi.TransformationType.None_, C_, 512)
    ivf.loadCoarseQuantizer(coarse)
    ivf.loadProductQuantizer(pq)
    ivf.setW(16)
    exact = mi.Linear(D, n)
    # the same vectors in the same order: record iid of the IVFPQ index is row iid of the Linear one (IndexTransformation.java:113-122)
    exact.indexVectors(ids, X)
    ivf.indexVectors(ids, X)

    Q = X[rng.choice(n, a.nq, replace=False)] + 0.05 * rng.standard_normal((a.nq, D))
    ei, _, ec = exact.search_batch(k, Q)

    def recall(got, cnt):
        return float(np.mean([len(set(ei[q, :ec[q]]) & set(got[q, :cnt[q]])) / k for q in range(len(Q))]))

    pi, _, pc = ivf.search_batch(k, Q)
    print(f"{n} vectors of length {D}, {a.nq} queries, w = 16")
    print(f"recall@{k} of the plain IVFPQ answer against Linear.search_batch: {recall(pi, pc):.3f}")
    for R in a.R:
        ri, rd, rc, missing = ivf.search_refine_batch(k, R, Q, exact)
        print(f"recall@{k} after exact re-ranking of the best R = {R:4d}:          {recall(ri, rc):.3f}   (missing rows: {missing})")
    ans = ivf.computeNearestNeighborsRefined(k, max(a.R), "img7", exact)
    print("neighbours of img7, exact distances:", list(zip(ans.getIds()[:3], np.round(ans.getDistances()[:3], 6))))
    for ix in (ivf, exact):
        ix.close()


if __name__ == "__main__":
    main()
