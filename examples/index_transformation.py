"""IndexTransformation.java:61-125 for its three targets (`small`, `pq`, `ivfpq`), as one native walk with nothing leaving HBM.

A full-dimensional Linear index is re-indexed by Linear.reindex (mmidx_linear_reindex): every vector is truncated to the target
length, L2-normalised because that was a truncation (:117-120), and appended under its id (:121) -- to a shorter Linear index, and
for `pq` / `ivfpq` to the compressed index as well, both filled from the same pass over the rows.  That pair is what the exact
re-ranking needs (record i of one is row i of the other), so the example ends, as Example.java:155-182 sketches, by comparing the
compressed answers with and without re-ranking against exact search.

    python examples/index_transformation.py [--kind small|pq|ivfpq] [--n 30000] [--dim 128] [--target 64]"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", choices=["small", "pq", "ivfpq"], default="ivfpq")
    ap.add_argument("--n", type=int, default=30000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--target", type=int, default=64)
    ap.add_argument("--chunk", type=int, default=8192)
    a = ap.parse_args()

    mi = importlib.import_module("multimedia-indexing_amd")
    rng = np.random.default_rng(0)
    n, D, T = a.n, a.dim, a.target
    centers = rng.standard_normal((64, D)) * 2.0
    X = centers[rng.integers(0, 64, n)] + rng.standard_normal((n, D))

    src = mi.Linear(D, n)  # the index to transform (IndexTransformation.java:71-76)
    src.indexVectors([f"img{i}" for i in range(n)], X)

    small = mi.Linear(T, n)  # `small`, and the exact side of the pair for the two compressed kinds
    targets = [small]
    if a.kind != "small":
        # the target's codebooks, learned on a sample of transformed vectors (the reference loads them from files, :84-100)
        Y = X[:, :T] / np.linalg.norm(X[:, :T], axis=1, keepdims=True)
        m, ks, C_ = 8, 256, 64
        if a.kind == "ivfpq":
            coarse = Y[rng.choice(n, C_, replace=False)]
            train = Y[:4096] - coarse[((Y[:4096, None, :] - coarse[None]) ** 2).sum(-1).argmin(1)]
            ix = mi.IVFPQ(T, n, False, "", m, ks, mi.TransformationType.None_, C_, 512)
            ix.loadCoarseQuantizer(coarse)
            ix.setW(16)
        else:
            train = Y[:4096]
            ix = mi.PQ(T, n, False, "", m, ks, mi.TransformationType.None_, 512)
        ix.loadProductQuantizer(np.stack([train[rng.choice(len(train), ks, replace=False), j * (T // m):(j + 1) * (T // m)] for j in range(m)]))
        targets.append(ix)

    moved = src.reindex(targets, chunk_rows=a.chunk)  # the walk of :111-123: truncate, renormalise, index under the same id
    print(f"re-indexed {moved} vectors {D} -> {T} ({a.kind}); targets hold {[t.size() for t in targets]}")
    assert all(t.size() == n and t.getId(n - 1) == f"img{n - 1}" for t in targets)

    k, R = 10, 100
    qids = rng.choice(n, 8, replace=False)
    ei, ed, ec = small.search_ids_batch(k, qids)  # stored vectors as queries
    assert all(ei[q, 0] == qids[q] and ed[q, 0] == 0.0 for q in range(len(qids)))
    print("exact path stats:", small.get_stats())
    if a.kind != "small":
        ix = targets[1]
        Q = np.stack([small.getVector(int(i)) for i in qids])
        ai, ad, ac = ix.search_batch(k, Q)
        ri, rd, rc, missing = ix.search_refine_batch(k, R, Q, small)  # re-ranked over the pair this walk has just built
        plain = np.mean([len(set(ei[q, :ec[q]]) & set(ai[q, :ac[q]])) / k for q in range(len(qids))])
        refined = np.mean([len(set(ei[q, :ec[q]]) & set(ri[q, :rc[q]])) / k for q in range(len(qids))])
        print(f"recall@{k} against exact search: {plain:.2f} plain, {refined:.2f} re-ranked from R = {R} (missing rows: {int(missing)})")
        assert int(missing) == 0  # every record of the compressed index has its row in the exact one
    for t in [src] + targets:
        t.close()


if __name__ == "__main__":
    main()
