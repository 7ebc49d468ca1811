"""PCAProjectionExample.java:74-88 as one native walk: every vector of a full-length Linear index is projected once to the largest
length, and each shorter length is a truncation of that projection (:79-82), L2-normalised on request (:83-85) and indexed in a
Linear index of its own under the same id (:86).  PCAProjection.project (mmidx_linear_reindex) does the projection on the f64 matrix
cores and all truncations in one pass over the projected rows; nothing leaves HBM.

    python examples/pca_projection.py [--n 20000] [--dim 256] [--lengths 16,32,64] [--whitening] [--no-l2]"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--lengths", default="16,32,64", help="projection lengths, increasing (at most eight)")
    ap.add_argument("--whitening", action="store_true")
    ap.add_argument("--no-l2", action="store_true", help="skip the L2 normalisation after the projection")
    a = ap.parse_args()

    mi = importlib.import_module("multimedia-indexing_amd")
    rng = np.random.default_rng(0)
    n, D = a.n, a.dim
    lengths = [int(s) for s in a.lengths.split(",")]
    X = rng.standard_normal((n, 24)) @ rng.standard_normal((24, D)) + 0.1 * rng.standard_normal((n, D))  # 24 strong directions

    full = mi.Linear(D, n)  # (:56-59)
    full.indexVectors([f"img{i}" for i in range(n)], X)

    nc = lengths[-1]  # the largest projection length (:62-64)
    # the basis comes from a file in the reference (:64); here numpy makes one of a sample (examples/learn_pca.py learns it on the GPU)
    sample = X[:min(n, 8192)]
    means = sample.mean(0)
    _, sv, Vt = np.linalg.svd(sample - means, full_matrices=False)
    pca = mi.PCA(nc, 1, D, a.whitening)
    pca.load(means, sv[:nc], Vt[:nc])

    projected = [mi.Linear(T, n) for T in lengths]  # (:67-77)
    moved = mi.PCAProjection.project(full, pca, projected, L2Normalization=not a.no_l2)
    print(f"projected {moved} vectors {D} -> {lengths} (whitening {a.whitening}, L2 {not a.no_l2})")

    P = pca.project(X[:64])
    for t, T in zip(projected, lengths):
        assert t.size() == n and t.getId(n - 1) == f"img{n - 1}"
        y = P[:, :T] if a.no_l2 else P[:, :T] / np.linalg.norm(P[:, :T], axis=1, keepdims=True)
        got = np.stack([t.getVector(i) for i in range(64)])
        print(f"  length {T}: first 64 rows within {np.abs(got - y).max():.1e} of numpy's")
        assert np.allclose(got, y, rtol=0, atol=1e-12)
    # neighbours of one image at every length (the shorter projections are what a compressed index is then built on)
    for t, T in zip(projected, lengths):
        ans = t.computeNearestNeighbors(5, "img7")
        print(f"  length {T}: neighbours of img7 {ans.getIds()}")
    for h in [full, pca] + projected:
        h.close()


if __name__ == "__main__":
    main()
