#!/usr/bin/env python3
""""More like this indexed image" on an IVFPQ index that keeps no vectors.

The reference's computeNearestNeighbors(k, String id) fails on IVFPQ (computeKnnIVFSDC is a stub, IVFPQ.java:509-511); its example
keeps a second, full-precision Linear index only to fetch the query vector from (Example.java:101-110).  Here the stored record of
the id is decoded on the GPU and searched as any vector:

  python examples/query_by_id.py             # a small index: a handful of ids, next to the vector query with the original vector
  python examples/query_by_id.py --measure   # the figures of DESIGN.md section 5.9: cfg3's shape, 16384 ids per call, HIP events
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def small(mi):
    import synth

    D, C_, m, ks, n, k, w = 64, 32, 8, 256, 20000, 5, 8
    p = synth.make_ivfpq_problem(n=n, D=D, C=C_, m=m, ks=ks, nq=1, seed=3)
    ix = mi.IVFPQ(D, n, False, "", m, ks, mi.TransformationType.None_, C_, 512)
    ix.loadCoarseQuantizer(p["coarse"])
    ix.loadProductQuantizer(p["pq"])
    ix.setW(w)
    names = [f"img{i}" for i in range(n)]
    assert ix.indexVectors(names, p["base"]) == n
    for id_ in ("img17", "img4242", "img9999", "img12345", "img19999"):
        by_id = ix.computeNearestNeighbors(k, id_)                                # the index alone answers
        by_vec = ix.computeNearestNeighbors(k, p["base"][int(id_[3:])])           # what needed the original vector before
        print(id_)
        print("  by id     ", [(i, float(f"{d:.4g}")) for i, d in zip(by_id.getIds(), by_id.getDistances())])
        print("  by vector ", [(i, float(f"{d:.4g}")) for i, d in zip(by_vec.getIds(), by_vec.getDistances())])
        assert by_id.getIds()[0] == id_, "an id's own record comes first"
        x = ix.reconstructVector(id_)
        print("  |original - reconstructed| =", float(f"{np.linalg.norm(p['base'][int(id_[3:])] - x):.4g}"))
    ix.close()


def measure(mi, out_path):
    """mmidx_search_ids_device against mmidx_search_device on the same decoded vectors plus mmidx_reconstruct_device alone, with no
    transformation and behind a rotation: 5 warm-up calls, median of 20, twice over (the spread between the rounds is the run-to-run
    spread)."""
    import synth
    import torch

    torch.cuda.init()
    L = mi.lib()
    N, D, C_, w, m, ks, k, B = 1_000_000, 128, 1024, 8, 16, 256, 100, 16384
    base, mu = synth.mixture(N, D, C_, sigma=0.15, seed=1234)
    cell = ((base[:40000] * base[:40000]).sum(1)[:, None] - 2 * base[:40000] @ mu.T + (mu * mu).sum(1)[None]).argmin(1)
    resid = mu[cell] - base[:40000]
    pq = np.stack([synth.kmeans(resid[:, s * 8:(s + 1) * 8], ks, iters=5, seed=s) for s in range(m)])
    rng = np.random.default_rng(0)
    rot = np.linalg.qr(rng.standard_normal((D, D)))[0]
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)

    def timed(fn, warm=5, reps=20):
        with torch.cuda.stream(st):
            for _ in range(warm):
                fn()
            st.synchronize()
            ts = []
            for _ in range(reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(st)
                fn()
                b.record(st)
                b.synchronize()
                ts.append(a.elapsed_time(b))
        ts.sort()
        return {"median_ms": round(ts[len(ts) // 2], 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4)}

    out = {}
    for name, tr, r in (("none", 0, None), ("rotation", 1, rot)):
        ix = mi.IVFPQ(D, N, False, "", m, ks, tr, C_, 512, rot=r)
        ix.loadCoarseQuantizer(mu)
        ix.loadProductQuantizer(pq)
        ix.setW(w)
        ix.indexVectors(list(range(N)), base)
        ids = torch.from_numpy(rng.choice(N, B, replace=False).astype(np.int32)).to(dev)
        X = torch.empty((B, D), dtype=torch.float64, device=dev)
        found = torch.empty(B, dtype=torch.int32, device=dev)
        oi, od, oc = (torch.empty((B, k), dtype=torch.int32, device=dev), torch.empty((B, k), dtype=torch.float64, device=dev),
                      torch.empty(B, dtype=torch.int32, device=dev))
        oi2, od2, oc2 = torch.empty_like(oi), torch.empty_like(od), torch.empty_like(oc)
        chk = mi._native.check
        calls = {
            "reconstruct": lambda: chk(L.mmidx_reconstruct_device(ix._h, B, ids.data_ptr(), X.data_ptr(), found.data_ptr(), st.cuda_stream)),
            "search_vectors": lambda: chk(L.mmidx_search_device(ix._h, k, B, X.data_ptr(), oi2.data_ptr(), od2.data_ptr(), oc2.data_ptr(), st.cuda_stream)),
            "search_ids": lambda: chk(L.mmidx_search_ids_device(ix._h, k, B, ids.data_ptr(), oi.data_ptr(), od.data_ptr(), oc.data_ptr(), st.cuda_stream)),
        }
        res = {f"{what}_{rnd}": timed(fn) for rnd in range(2) for what, fn in calls.items()}
        st.synchronize()
        assert torch.equal(oi, oi2) and torch.equal(od, od2) and torch.equal(oc, oc2), "id search and vector search differ"
        res["own_record_first"] = float((oi[:, 0] == ids).float().mean())
        t = res["reconstruct_1"]["median_ms"] * 1e-3
        moved = B * D * 8 * 2 + B * m + B * 8  # rows written, centroid rows read, codes, ids and found
        res["decode_bytes"] = moved
        res["decode_fraction_of_copy_ceiling"] = round(moved / t / 6.29e12, 4)
        if tr == 1:
            res["decode_fp64_GFLOPs"] = round(2.0 * B * D * D / t / 1e9, 1)
        out[name] = res
        print(name, json.dumps(res), flush=True)
        ix.close()
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", action="store_true", help="time the device forms at cfg3's shape instead of the small run")
    ap.add_argument("--out", default=None, help="with --measure: write the figures as JSON to this file")
    a = ap.parse_args()
    mi = importlib.import_module("multimedia-indexing_amd")
    if mi.lib().mmidx_device_count() < 1:
        raise SystemExit("query_by_id.py needs an MI355X: libmmidx_hip has no CPU fallback")
    if a.measure:
        measure(mi, a.out)
    else:
        small(mi)


if __name__ == "__main__":
    main()
