"""Linear at scale: queries per second of exact search over a large HBM-resident index, and the cost of interleaved appends.

    python tools/linear_scale.py [--n 1000000] [--dim 128] [--k 10 100] [--nq 4096] [--reps 5] [--lib PATH] [--exact]

Runs on any build of libmmidx_hip.so: with --lib pointing at an older library that lacks the device entry points and the
option switch, only mmidx_linear_add / mmidx_linear_search are used, so the same script measures the commit before the scan
on the same box in the same session (the reference point).  --exact sets the option "exact" (a second column, never the
reference point).  Every run carries a parity gate: 64 queries against the CPU oracle, ids and distance bits.  Timing: one
warm-up call, `reps` timed calls, the median and the spread (min, max) are reported.  One JSON object on stdout."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(fn, reps):
    fn()  # warm-up: workspaces, first launches
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--k", type=int, nargs="+", default=[10, 100])
    ap.add_argument("--nq", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lib", default=os.path.join(ROOT, "multimedia-indexing_amd", "csrc", "libmmidx_hip.so"))
    ap.add_argument("--exact", action="store_true")
    ap.add_argument("--steps", type=int, default=50, help="interleaved pattern: add 100 rows, one query, this many times")
    a = ap.parse_args()

    torch = None
    try:
        import torch  # binds the HIP runtime torch ships before the library loads, as the package does

        torch.cuda.init()
    except Exception:
        torch = None
    from oracle import oracle as o

    o.build()
    L = C.CDLL(a.lib)
    L.mmidx_last_error.restype = C.c_char_p
    has_new = hasattr(L, "mmidx_linear_search_device")
    vp = C.c_void_p
    L.mmidx_linear_create.argtypes = [C.c_int, C.c_int64, C.c_int, C.POINTER(vp)]
    L.mmidx_linear_add.argtypes = [vp, C.c_int64, vp]
    L.mmidx_linear_search.argtypes = [vp, C.c_int, C.c_int64, vp, vp, vp, vp]
    L.mmidx_linear_destroy.argtypes = [vp]

    def ck(rc):
        if rc:
            raise RuntimeError(L.mmidx_last_error().decode())

    rng = np.random.default_rng(1)
    n, D, extra = a.n, a.dim, 100 * a.steps
    X = rng.standard_normal((n + extra, D))
    Q = np.ascontiguousarray(X[rng.choice(n, a.nq, replace=False)] + 0.05 * rng.standard_normal((a.nq, D)))
    h = vp()
    ck(L.mmidx_linear_create(D, n + extra, 0, C.byref(h)))
    t0 = time.perf_counter()
    for r0 in range(0, n, 100_000):
        blk = np.ascontiguousarray(X[r0:min(n, r0 + 100_000)])
        ck(L.mmidx_linear_add(h, blk.shape[0], blk.ctypes.data))
    out = {"lib": os.path.relpath(a.lib, ROOT), "has_scan": has_new, "exact_option": bool(a.exact), "n": n, "dim": D, "nq": a.nq,
           "fill_s": round(time.perf_counter() - t0, 3), "k": {}}
    if a.exact:
        if not has_new:
            raise SystemExit("--exact needs a library with mmidx_linear_set_option")
        L.mmidx_linear_set_option.argtypes = [vp, C.c_char_p, C.c_int]
        ck(L.mmidx_linear_set_option(h, b"exact", 1))

    def host_search(k, Qm):
        ii = np.empty((Qm.shape[0], k), np.int32)
        dd = np.empty((Qm.shape[0], k), np.float64)
        cc = np.empty(Qm.shape[0], np.int32)
        ck(L.mmidx_linear_search(h, k, Qm.shape[0], Qm.ctypes.data, ii.ctypes.data, dd.ctypes.data, cc.ctypes.data))
        return ii, dd, cc

    for k in a.k:
        res = {}
        gi, gd, gc = host_search(k, Q[:64])
        wi, wd, wc = o.linear_search_batch(X[:n], Q[:64], k, nthreads=16)
        res["parity_64"] = bool(np.array_equal(gi, wi) and np.array_equal(gd, wd) and np.array_equal(gc, wc))
        if not res["parity_64"]:
            out["k"][str(k)] = res
            print(json.dumps(out))
            raise SystemExit("parity gate failed")
        t = _timed(lambda: host_search(k, Q), a.reps)
        res["host_call"] = dict(t, qps=round(a.nq / t["median_s"], 1))
        if has_new and torch is not None:
            L.mmidx_linear_search_device.argtypes = [vp, C.c_int, C.c_int64, vp, vp, vp, vp, vp]
            dQ = torch.from_numpy(Q).cuda()
            di = torch.empty((a.nq, k), dtype=torch.int32, device="cuda")
            dd = torch.empty((a.nq, k), dtype=torch.float64, device="cuda")
            dc = torch.empty(a.nq, dtype=torch.int32, device="cuda")

            def dev():
                ck(L.mmidx_linear_search_device(h, k, a.nq, dQ.data_ptr(), di.data_ptr(), dd.data_ptr(), dc.data_ptr(), None))
                torch.cuda.synchronize()

            t = _timed(dev, a.reps)
            res["device_call"] = dict(t, qps=round(a.nq / t["median_s"], 1))
        if has_new:
            from importlib import import_module

            St = import_module("multimedia-indexing_amd._native").LinearStats
            L.mmidx_linear_set_option.argtypes = [vp, C.c_char_p, C.c_int]
            L.mmidx_linear_get_stats.argtypes = [vp, C.POINTER(St)]
            ck(L.mmidx_linear_set_option(h, b"debug_sync", 1))
            host_search(k, Q)
            s = St()
            ck(L.mmidx_linear_get_stats(h, C.byref(s)))
            res["stats"] = {f: getattr(s, f) for f, _ in s._fields_}
            ck(L.mmidx_linear_set_option(h, b"debug_sync", 0))
        out["k"][str(k)] = res
    # interleaved: add 100 rows, one query (k = 10), `steps` times
    ts = []
    for s_ in range(a.steps):
        blk = np.ascontiguousarray(X[n + 100 * s_:n + 100 * (s_ + 1)])
        t0 = time.perf_counter()
        ck(L.mmidx_linear_add(h, 100, blk.ctypes.data))
        host_search(10, Q[s_:s_ + 1])
        ts.append(time.perf_counter() - t0)
    gi, gd, gc = host_search(10, Q[:8])
    wi, wd, wc = o.linear_search_batch(X, Q[:8], 10, nthreads=16)
    out["interleaved"] = {"steps": a.steps, "median_step_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts),
                          "parity_after": bool(np.array_equal(gi, wi) and np.array_equal(gd, wd))}
    L.mmidx_linear_destroy(h)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
