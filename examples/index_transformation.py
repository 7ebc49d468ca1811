"""IndexTransformation.java:61-125 for the `ivfpq` target, with nothing leaving HBM between the two indexes.

A full-dimensional Linear index is walked in chunks (mmidx_linear_copy_rows_device: the getVector loop of :113-122), every
vector is truncated to the target length and L2-normalised (:117-120; torch is the plumbing here), and fed to an IVFPQ handle
with mmidx_add_vectors_device.  Then, as Example.java:155-182 sketches, a handful of exact neighbours from a Linear index over
the transformed vectors are compared with the IVFPQ answers.

    python examples/index_transformation.py [--n 30000] [--dim 128] [--target 64]"""
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
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--target", type=int, default=64)
    ap.add_argument("--chunk", type=int, default=8192)
    a = ap.parse_args()
    import torch

    mi = importlib.import_module("multimedia-indexing_amd")
    N = importlib.import_module("multimedia-indexing_amd._native")
    L = mi.lib()
    rng = np.random.default_rng(0)
    n, D, T = a.n, a.dim, a.target
    centers = rng.standard_normal((64, D)) * 2.0
    X = centers[rng.integers(0, 64, n)] + rng.standard_normal((n, D))

    src = mi.Linear(D, n)  # the index to transform (IndexTransformation.java:71-76)
    src.indexVectors([f"img{i}" for i in range(n)], X)

    # the target's codebooks, learned on a sample of transformed vectors (the reference loads them from files, :84-100)
    Y = X[:, :T] / np.linalg.norm(X[:, :T], axis=1, keepdims=True)
    m, ks, C_ = 8, 256, 64
    coarse = Y[rng.choice(n, C_, replace=False)]
    resid = Y[:4096] - coarse[((Y[:4096, None, :] - coarse[None]) ** 2).sum(-1).argmin(1)]
    pq = np.stack([resid[rng.choice(4096, ks, replace=False), j * (T // m):(j + 1) * (T // m)] for j in range(m)])
    ivf = mi.IVFPQ(T, n, False, "", m, ks, mi.TransformationType.None_, C_, 512)
    ivf.loadCoarseQuantizer(coarse)
    ivf.loadProductQuantizer(pq)
    ivf.setW(16)
    exact = mi.Linear(T, n)  # the exact yardstick over the transformed vectors (Example.java:155-182)

    buf = torch.empty((a.chunk, D), dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    for i0 in range(0, n, a.chunk):  # the walk of :113-122
        nb = min(a.chunk, n - i0)
        src.copy_rows_device(i0, buf[:nb])
        y = buf[:nb, :T].contiguous()
        y = (y / torch.linalg.vector_norm(y, dim=1, keepdim=True)).contiguous()  # :117-120
        N.check(L.mmidx_add_vectors_device(ivf._h, nb, y.data_ptr(), None, i0, st))
        exact.add_device(y)
    torch.cuda.synchronize()
    N.check(L.mmidx_sync_index(ivf._h))
    print(f"transformed {n} vectors {D} -> {T}; target holds {ivf.size()}, exact yardstick {exact.size()}")

    k = 10
    qids = rng.choice(n, 8, replace=False)
    ei, ed, ec = exact.search_ids_batch(k, qids)  # stored vectors as queries
    Qt = np.stack([exact.getVector(int(i)) for i in qids])
    ai, ad, ac = ivf.search_batch(k, Qt)
    recall = np.mean([len(set(ei[q, :ec[q]]) & set(ai[q, :ac[q]])) / k for q in range(len(qids))])
    print("exact path stats:", exact.get_stats())
    print(f"recall@{k} of IVFPQ (w = 16) against exact search: {recall:.2f}")
    assert all(ei[q, 0] == qids[q] and ed[q, 0] == 0.0 for q in range(len(qids)))
    for ix in (src, ivf, exact):
        ix.close()


if __name__ == "__main__":
    main()
