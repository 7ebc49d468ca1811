#!/usr/bin/env python3
"""Learn a product quantizer in one device-resident call, then load it, index and query.

ProductQuantizationLearning.learn_batched does what ProductQuantizationLearning.java:225-305 does -- residuals w.r.t. the coarse
quantizer, the index's transformation, k-means++ per sub-space with several seeds, the repeat of lowest squared error kept -- with
all sub-spaces and repeats sharing every kernel launch:

  python examples/learn_pq.py             # 20000 vectors: learn, write the file, load it into an IVFPQ index, query
  python examples/learn_pq.py --measure   # the figures of DESIGN.md section 5.10: one batched call against a loop of
                                          # mmidx_kmeans_device calls, one per sub-space, at the bench's and the yfcc shape
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def small(mi):
    q = mi.quantization
    D, Cc, m, ks, n, k = 64, 32, 8, 256, 20000, 5
    rng = np.random.default_rng(7)
    mu = 2.0 * rng.standard_normal((Cc, D))
    X = mu[rng.integers(0, Cc, n)] + 0.5 * rng.standard_normal((n, D))
    coarse = q.CoarseQuantizerLearning.learn(X, Cc, maxIterations=10, kMeansPlusPlus=True)
    perm = q.RandomPermutation(1, D).randomlyPermutatedIndices  # the permutation the index derives from the same seed
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, f"pq_{D}_{m}x8_{n}_rp_ivf_c{Cc}.csv")
        t0 = time.time()
        pq = q.ProductQuantizationLearning.learn_batched(X, m, ks, maxIterations=20, numKmeansRepeats=2, coarseQuantizer=coarse,
                                                         transformation=mi.TransformationType.RandomPermutation, perm=perm, outFilePath=path)
        st = q.ProductQuantizationLearning.last_stats
        print(f"learned {m} x {ks} x {D // m} in {time.time() - t0:.2f} s; kept seeds {st['seed'].tolist()}, iterations {st['iterations'].tolist()}")
        ix = mi.IVFPQ(D, n, False, "", m, ks, mi.TransformationType.RandomPermutation, Cc, 512)
        ix.loadCoarseQuantizer(coarse)
        ix.loadProductQuantizer(path)
    ix.setW(8)
    assert ix.indexVectors([f"img{i}" for i in range(n)], X) == n
    hits = 0
    for i in (17, 4242, 9999, 12345, 19999):
        a = ix.computeNearestNeighbors(k, X[i])
        print(f"img{i}", [(j, float(f"{d:.4g}")) for j, d in zip(a.getIds(), a.getDistances())])
        hits += f"img{i}" in a.getIds()
    print(f"{hits} of 5 vectors found among their own {k} nearest codes")
    err = np.mean([np.sum((ix.reconstructVector(f"img{i}") - X[i]) ** 2) for i in range(0, n, 97)])
    print("mean squared quantisation error", float(f"{err:.4g}"), "of", float(f"{np.mean(np.sum((X - X.mean(0)) ** 2, 1)):.4g}"))
    assert pq.shape == (m, ks, D // m) and hits >= 4
    ix.close()


def measure(mi, out_path, shapes):
    """wall time of one mmidx_pq_learn_device call against the loop it replaces (one mmidx_kmeans_device call per sub-space, as
    bench.py builds its codebooks): residual-ready vectors on the device, ks = 256, one repeat, not normalised, the iterations of the
    two benchmarks' own builds.  The loop's time includes the contiguous copy of each sub-space's slice and the wait before each
    call, as in bench.py; the batched call reads the [n][D] array as it is.  Two warm-up runs, then the two forms alternating, five
    times each; median, minimum and maximum."""
    import torch

    torch.cuda.init()
    L, chk = mi.lib(), mi._native.check
    dev = torch.device("cuda", 0)
    out = {}
    for name, n, D, m, iters in shapes:
        ks, dsub = 256, D // m
        g = torch.Generator(device=dev)
        g.manual_seed(1234)
        X = 0.15 * torch.randn(n, D, generator=g, device=dev, dtype=torch.float64)
        torch.cuda.synchronize()
        pq_b = np.zeros((m, ks, dsub))
        pq_l = np.full((m, ks, dsub), 1000.0)
        sse = np.zeros(m)

        def batched():
            chk(L.mmidx_pq_learn_device(0, n, D, m, ks, iters, 1, 0, X.data_ptr(), 0, None, 0, None, None, pq_b.ctypes.data, sse.ctypes.data, None,
                                        None, None, None))

        def loop():
            kout, it = C.c_int32(0), C.c_int32(0)
            for s in range(m):
                sub = X[:, s * dsub:(s + 1) * dsub].contiguous()
                torch.cuda.synchronize()
                chk(L.mmidx_kmeans_device(0, n, dsub, ks, iters, 1, 1, sub.data_ptr(), None, pq_l[s].ctypes.data, None, None, C.addressof(it),
                                          C.addressof(kout), None))

        def wall(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        for _ in range(2):
            wall(batched)
        wall(loop)
        tb, tl = [], []
        for _ in range(5):
            tb.append(wall(batched))
            tl.append(wall(loop))
        tb.sort()
        tl.sort()
        res = {"n": n, "D": D, "m": m, "iterations": iters, "batched_ms": {"median": round(tb[2], 2), "min": round(tb[0], 2), "max": round(tb[-1], 2)},
               "loop_ms": {"median": round(tl[2], 2), "min": round(tl[0], 2), "max": round(tl[-1], 2)},
               "speedup_of_medians": round(tl[2] / tb[2], 2), "same_codebooks": bool(np.array_equal(pq_b, pq_l))}
        out[name] = res
        print(name, json.dumps(res), flush=True)
        del X
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", action="store_true", help="time the batched call against the per-sub-space loop instead of the small run")
    ap.add_argument("--shapes", default="bench,yfcc", help="with --measure: bench (2^18 x 128, m = 16, 8 iterations) and / or yfcc (2^17 x 1024, m = 64, 6 iterations)")
    ap.add_argument("--out", default=None, help="with --measure: write the figures as JSON to this file")
    a = ap.parse_args()
    mi = importlib.import_module("multimedia-indexing_amd")
    if mi.lib().mmidx_device_count() < 1:
        raise SystemExit("learn_pq.py needs an MI355X: libmmidx_hip has no CPU fallback")
    if a.measure:
        table = {"bench": ("bench", 1 << 18, 128, 16, 8), "yfcc": ("yfcc", 1 << 17, 1024, 64, 6)}
        measure(mi, a.out, [table[s] for s in a.shapes.split(",")])
    else:
        small(mi)


if __name__ == "__main__":
    main()
