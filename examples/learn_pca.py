#!/usr/bin/env python3
"""From descriptors to a searchable index without leaving the project (the reference's PCALearningExample.java:36-55 followed
by its indexing examples), on one MI355X:

  synthetic SURF-64 descriptors -> batched VLAD (power + L2)
     -> PCA basis LEARNED on the GPU (addSamples / computeBasis) -> savePCAToFile
     -> a fresh PCA loads the file with whitening -> projection -> IVFPQ index / search

  python examples/learn_pca.py --images 4000 --centroids 32 --components 64
  python examples/learn_pca.py --streaming     # PCA.streaming: the VLAD batches are folded in as they come and are not kept
"""
import argparse
import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def run(n_images=4000, ncent=32, nc_out=64, n_queries=64, k=10, seed=0, cells=64, w=8, pca_file=None, verbose=True, streaming=False):
    mi = importlib.import_module("multimedia-indexing_amd")
    rng = np.random.default_rng(seed)
    dl = 64
    codebook = rng.standard_normal((ncent, dl)) / 8.0
    topics = rng.standard_normal((64, 24, dl))

    def make_image(t, noise):
        nd = int(rng.integers(200, 801))
        d = topics[t][rng.integers(0, 24, size=nd)] + noise * rng.standard_normal((nd, dl))
        return d / np.linalg.norm(d, axis=1, keepdims=True)

    images = [make_image(t, 0.35) for t in rng.integers(0, 64, size=n_images)]
    vlad = mi.VladAggregatorMultipleVocabularies([codebook], normalizationsOn=True)
    V = np.concatenate([vlad.aggregate_batch(images[i:i + 4096]) for i in range(0, n_images, 4096)])
    ss = V.shape[1]
    # ---- learn the basis: PCA(numComponents, numSamples, sampleSize), addSample x n, computeBasis, savePCAToFile ----
    t0 = time.time()
    if streaming:  # no sample count up front; any split over the calls gives the same bytes
        learner = mi.PCA.streaming(nc_out, ss, False)
        for i in range(0, n_images, 1000):
            learner.addSamples(V[i:i + 1000])
    else:
        learner = mi.PCA(nc_out, n_images, ss, False)
        learner.addSamples(V)
    learner.computeBasis(tol=1e-10, max_iter=500)
    t_learn = time.time() - t0
    path = pca_file or os.path.join(tempfile.mkdtemp(), "pca.txt")
    learner.savePCAToFile(path)
    # ---- apply: a fresh object loads the file, whitening on (PCA.java:257-318) ----
    pca = mi.PCA(nc_out, 1, ss, True)
    pca.loadPCAFromFile(path)
    X = pca.project(V)
    D, m, ks = nc_out, 16, 256
    coarse = mi.quantization.CoarseQuantizerLearning.learn(X, cells, maxIterations=10, seed=1, kMeansPlusPlus=True)
    if coarse.shape[0] < cells:
        coarse = np.concatenate([coarse, np.full((cells - coarse.shape[0], D), 1000.0)])
    pq = mi.quantization.ProductQuantizationLearning.learn(X, m, ks, maxIterations=8, numKmeansRepeats=1, coarseQuantizer=coarse)
    ix = mi.IVFPQ(D, n_images, False, "", m, ks, mi.TransformationType.None_, cells, 512)
    ix.loadCoarseQuantizer(coarse)
    ix.loadProductQuantizer(pq)
    ix.setW(w)
    ix.indexVectors([f"img{i}" for i in range(n_images)], X)
    qi = rng.choice(n_images, n_queries, replace=False)
    qimgs = [images[i] + 0.02 * rng.standard_normal(images[i].shape) for i in qi]
    Q = mi.frontend.ImageVectorizer(vlad, pca).transform_batch(qimgs)
    iids, _, _ = ix.search_batch(k, Q)
    out = {"images": n_images, "vlad_length": ss, "components": nc_out, "streaming": bool(streaming), "pca_learn_seconds": round(t_learn, 3),
           "pca_iterations": learner.iterations, "pca_residual": learner.residual,
           "singular_values_first_last": [float(learner.singularValues[0]), float(learner.singularValues[-1])],
           "self_hit_rate": float(np.mean(iids[:, 0] == qi)), "pca_file": path}
    for o in (vlad, learner, pca, ix):
        o.close()
    if verbose:
        print(json.dumps(out))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=4000)
    ap.add_argument("--centroids", type=int, default=32)
    ap.add_argument("--components", type=int, default=64)
    ap.add_argument("--pca-file", default=None)
    ap.add_argument("--streaming", action="store_true", help="learn with PCA.streaming (mmidx_pca_stream_*)")
    a = ap.parse_args()
    run(a.images, a.centroids, a.components, pca_file=a.pca_file, streaming=a.streaming)
