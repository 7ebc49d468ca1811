"""The exact re-ranking at scale (mmidx_search_refine_device): what it costs on top of the search it starts from.

    python tools/refine_scale.py [--n 1000000] [--dim 128] [--nq 16384] [--R 100 400 1000] [--k 100] [--reps 7]

The shape of BASELINE config 3 (IVFPQ, C = 1024, w = 8, m = 16 x 256) with a Linear index over the same vectors.  Per R:
  search_ms   mmidx_search_device with k = R alone (the path the refine call starts with: the floor)
  refine_ms   mmidx_search_refine_device(k, R)
  their difference as bytes gathered per second (the kept candidates' fp64 rows), beside the 6.29 TB/s measured copy ceiling
  recall@k of the plain answer (k = `--k`) and of the refined one against Linear
  a 64-query parity sample against the CPU oracle + the numpy twin (tests/refine_twin.py), in the same run
Timing: device-resident queries and outputs, HIP events around each call on one stream, one warm-up of both, then `reps` rounds in
which the two calls alternate; median and spread (min, max).  One JSON object on stdout."""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

COPY_CEILING_TBS = 6.29


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--nq", type=int, default=16384)
    ap.add_argument("--R", type=int, nargs="+", default=[100, 400, 1000])
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    import torch

    import refine_twin as rt
    import synth
    from oracle import oracle as o

    o.build()
    mi = importlib.import_module("multimedia-indexing_amd")
    N = importlib.import_module("multimedia-indexing_amd._native")
    L = mi.lib()
    n, D, nq, k = a.n, a.dim, a.nq, a.k
    C_, w, m, ks = 1024, 8, 16, 256
    rng = np.random.default_rng(99)
    base, coarse = synth.mixture(n, D, C_, sigma=0.15, seed=1234)
    ns = min(n, 40000)
    cell = ((base[:ns] * base[:ns]).sum(1)[:, None] - 2 * base[:ns] @ coarse.T + (coarse * coarse).sum(1)[None]).argmin(1)
    resid = coarse[cell] - base[:ns]
    ds = D // m
    pq = np.stack([synth.kmeans(resid[:, s * ds:(s + 1) * ds], ks, iters=5, seed=s) for s in range(m)])
    ix = mi.IVFPQ(D, n, False, "", m, ks, 0, C_, 512)
    ix.loadCoarseQuantizer(coarse)
    ix.loadProductQuantizer(pq)
    ix.setW(w)
    lin = mi.Linear(D, n)
    for r0 in range(0, n, 100_000):
        ix._add_vectors(base[r0:r0 + 100_000], np.arange(r0, min(n, r0 + 100_000), dtype=np.int32))
        lin._add_vectors(base[r0:r0 + 100_000], None)
    N.check(L.mmidx_sync_index(ix._h))
    Q = np.ascontiguousarray(base[rng.choice(n, nq, replace=False)] + 0.05 * rng.standard_normal((nq, D)))
    dQ = torch.from_numpy(Q).cuda()
    ref = o.OracleIndex(o.KIND_IVFPQ, D, m, ks, C_)
    ref.set_coarse(coarse)
    ref.set_pq(pq)
    ref.set_w(w)
    ref.load_lists(*ix.export())
    xi, _, xc = lin.search_batch(k, Q)  # the exact yardstick
    s = torch.cuda.Stream()

    def timed_pair(fa, fb):
        """the two calls alternate inside one timed window, so that whatever else the machine does meets both alike"""
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(a.reps)]
        with torch.cuda.stream(s):
            fa()
            fb()
            s.synchronize()
            for e in ev:
                e[0].record(s)
                fa()
                e[1].record(s)
                fb()
                e[2].record(s)
            s.synchronize()
        out = []
        for i in (0, 1):
            ts = [e[i].elapsed_time(e[i + 1]) for e in ev]
            out.append({"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "reps": a.reps})
        return out

    def recall(ids, cnt):
        return float(np.mean([len(set(xi[q, :xc[q]].tolist()) & set(ids[q, :cnt[q]].tolist())) / k for q in range(0, nq, 8)]))

    pi, _, pc = ix.search_batch(k, Q)
    out = {"n": n, "dim": D, "nq": nq, "k": k, "C": C_, "w": w, "m": m, "copy_ceiling_TBs": COPY_CEILING_TBS, "recall_plain": recall(pi, pc), "R": {}}
    for R in a.R:
        if R < k:
            continue
        oi = torch.empty((nq, R), dtype=torch.int32, device="cuda")
        od = torch.empty((nq, R), dtype=torch.float64, device="cuda")
        oc = torch.empty(nq, dtype=torch.int32, device="cuda")
        ri = torch.empty((nq, k), dtype=torch.int32, device="cuda")
        rd = torch.empty((nq, k), dtype=torch.float64, device="cuda")
        rc = torch.empty(nq, dtype=torch.int32, device="cuda")
        rm = torch.zeros(1, dtype=torch.int64, device="cuda")
        st = s.cuda_stream
        t_s, t_r = timed_pair(
            lambda: N.check(L.mmidx_search_device(ix._h, R, nq, dQ.data_ptr(), oi.data_ptr(), od.data_ptr(), oc.data_ptr(), st)),
            lambda: N.check(L.mmidx_search_refine_device(ix._h, lin._h, k, R, nq, dQ.data_ptr(), ri.data_ptr(), rd.data_ptr(), rc.data_ptr(),
                                                         rm.data_ptr(), st)))
        gi, gd, gc = ri.cpu().numpy(), rd.cpu().numpy(), rc.cpu().numpy()
        rows = int(oc.sum().item())
        extra_ms = t_r["median_ms"] - t_s["median_ms"]
        want = rt.refine_batch(ref.search_batch(Q[:64], R, nthreads=16), base, Q[:64], k)
        parity = bool(np.array_equal(gi[:64], want[0]) and np.array_equal(gd[:64].view(np.uint64), want[1].view(np.uint64)) and
                      np.array_equal(gc[:64], want[2]))
        out["R"][str(R)] = {"search": t_s, "refine": t_r, "extra_ms": extra_ms, "rows_gathered": rows, "bytes_gathered": rows * D * 8,
                            "gather_TBs": (rows * D * 8 / (extra_ms * 1e-3) / 1e12) if extra_ms > 0 else None, "missing": int(rm.item()),
                            "recall_refined": recall(gi, gc), "parity_64": parity}
        if not parity:
            print(json.dumps(out))
            raise SystemExit("parity gate failed")
    ix.close()
    lin.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
