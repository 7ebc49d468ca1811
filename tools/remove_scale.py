"""Removal at scale (mmidx_remove_device) against the round trip it replaces, in one process.

    python tools/remove_scale.py [--shape cfg3 cfg4] [--reps 5] [--out FILE]

Shapes: cfg3  1 M records, C = 1024, m = 16 byte codes (BASELINE config 3)
        cfg4  100 M records, C = 8192, m = 16 byte codes (the headline index)
The records are random (list, code) pairs under the internal ids 0 .. n - 1 in random arrival order: a removal never looks into a
code, so no quantizer is trained.  Per shape and per request set -- 1 id, 1 % and 50 % of the ids, drawn uniformly --:
  (a) remove     mmidx_remove_device on a freshly restored index whose iid -> position table is built (one mmidx_get_codes first),
                 host clock around the synchronous call; `remove_cold` is the same call where the table has to be built first
  (b) roundtrip  the only way on a library without the call: mmidx_export -> numpy filter -> fresh handle -> mmidx_add_codes ->
                 mmidx_sync_index, host clock around all of it
  (c) bytes      what the call must move: every id read once, the survivors' ids and codes read and written; divided by (a), beside
                 a plain device-to-device copy of as many bytes timed in the same run (HIP events) and the 6.29 TB/s the guide quotes
  gate           the export after (a) equals the export after (b), array for array
  deferred       what (a) leaves to the next calls: with random quantizers loaded and the search path warm, the first 64-query search
                 after a removal of 1 % (it rebuilds the per-code norms of pass B over all codes) beside the second, and the first
                 mmidx_get_codes (it rebuilds the iid -> position table) beside the second
Medians and spreads (min, max) of `reps` runs, each on an index of its own.  One JSON object on stdout."""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

COPY_CEILING_TBS = 6.29
SHAPES = {"cfg3": (1_000_000, 1024, 16), "cfg4": (100_000_000, 8192, 16)}  # n, C, m
D_, KS = 128, 256


def spread(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "reps": len(ts)}


def run_shape(mi, N, torch, name, reps):
    L = mi.lib()
    n, C_, m = SHAPES[name]
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(99)
    d_iids = torch.randperm(n, device=dev, generator=g).to(torch.int32)
    d_cells = torch.randint(0, C_, (n,), device=dev, generator=g, dtype=torch.int32)
    d_codes = torch.randint(-128, 128, (n, m), device=dev, generator=g, dtype=torch.int8)
    st = torch.cuda.current_stream(dev).cuda_stream
    one = np.array([0], np.int32)

    def restore(prep=None):
        ix = mi.IVFPQ(D_, n, False, "", m, KS, 0, C_, 512)
        if prep:
            prep(ix)  # (quantizers, for the runs that search)
        N.check(L.mmidx_add_codes_device(ix._h, n, d_iids.data_ptr(), d_cells.data_ptr(), d_codes.data_ptr(), st))
        N.check(L.mmidx_sync_index(ix._h))
        return ix

    def remove(ix, d_req, warm):
        if warm:  # builds the iid -> position table, as any per-id call before would have
            N.check(L.mmidx_get_codes(ix._h, 1, one.ctypes.data, None, None))
        removed = C.c_int64(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        N.check(L.mmidx_remove_device(ix._h, d_req.shape[0], d_req.data_ptr(), None, C.byref(removed), st))
        return (time.perf_counter() - t0) * 1e3, removed.value

    def roundtrip(ix, req):
        t0 = time.perf_counter()
        off, iids, codes = ix.export()
        keep = ~np.isin(iids, req)
        cells = np.repeat(np.arange(C_, dtype=np.int32), np.diff(off))
        fresh = mi.IVFPQ(D_, n, False, "", m, KS, 0, C_, 512)
        ki, kc, kk = np.ascontiguousarray(iids[keep]), np.ascontiguousarray(cells[keep]), np.ascontiguousarray(codes[keep])
        N.check(L.mmidx_add_codes(fresh._h, len(ki), ki.ctypes.data, kc.ctypes.data, kk.ctypes.data))
        N.check(L.mmidx_sync_index(fresh._h))
        return (time.perf_counter() - t0) * 1e3, fresh

    def copy_ms(nbytes):
        """a plain device copy that reads and writes nbytes in all"""
        a = torch.empty(max(nbytes // 2, 1), dtype=torch.uint8, device=dev)
        b = torch.empty_like(a)
        b.copy_(a)
        ts = []
        for _ in range(7):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            b.copy_(a)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return statistics.median(ts)

    rng = np.random.default_rng(7)
    out = {"n": n, "C": C_, "m": m, "record_bytes": m}
    for label, count in (("one", 1), ("1pct", n // 100), ("50pct", n // 2)):
        req = rng.choice(n, count, replace=False).astype(np.int32)
        d_req = torch.from_numpy(req).to(dev)
        warm, cold, rt_ms = [], [], []
        last = None
        for r in range(reps + 1):  # round 0 warms up
            for is_warm, ts in ((True, warm), (False, cold)):
                ix = restore()
                ms, removed = remove(ix, d_req, is_warm)
                assert removed == count
                if r > 0:
                    ts.append(ms)
                if is_warm and r == reps:
                    last = ix
                else:
                    ix.close()
        for r in range(max(1, min(reps, 3))):
            ix = restore()
            ms, fresh = roundtrip(ix, req)
            ix.close()
            rt_ms.append(ms)
            if r == 0:
                a, b = last.export(), fresh.export()
                gate = all(np.array_equal(x, y) for x, y in zip(a, b))
                last.close()
            fresh.close()
        kept = n - count
        nbytes = n * 4 + 2 * kept * (4 + m)
        row = {"ids": count, "remove": spread(warm), "remove_cold": spread(cold), "roundtrip": spread(rt_ms), "export_equal": bool(gate), "bytes": nbytes}
        row["TBs"] = nbytes / (row["remove"]["median_ms"] * 1e-3) / 1e12
        c_ms = copy_ms(nbytes)
        row["copy_same_bytes_ms"] = c_ms
        row["copy_TBs"] = nbytes / (c_ms * 1e-3) / 1e12
        row["share_of_measured_copy"] = c_ms / row["remove"]["median_ms"]
        row["share_of_quoted_ceiling"] = row["TBs"] / COPY_CEILING_TBS
        row["roundtrip_over_remove"] = row["roundtrip"]["median_ms"] / row["remove"]["median_ms"]
        out[label] = row
        print(json.dumps({name: {label: row}}), flush=True)
    out["deferred"] = deferred(mi, N, restore, remove, torch.from_numpy((rng.choice(n - 2, n // 100, replace=False) + 2).astype(np.int32)).to(dev), C_, m, reps)
    print(json.dumps({name: {"deferred": out["deferred"]}}), flush=True)
    return out


def deferred(mi, N, restore, remove, d_req, C_, m, reps):
    """What (a) leaves to the next calls: the removal invalidates the per-code norms of the matrix-core pass B and the iid -> position
    table.  With (random) quantizers loaded and the search path warm: the first 64-query search after a removal of 1 % (it rebuilds
    the norms over all codes) beside the second one (it does not), and the first mmidx_get_codes after it beside the second."""
    L = mi.lib()
    rng = np.random.default_rng(3)
    coarse, pq = rng.standard_normal((C_, D_)), rng.standard_normal((m, KS, D_ // m))
    Q = rng.standard_normal((64, D_))
    one = np.array([1], np.int32)
    s1, s2, g1, g2 = [], [], [], []
    for r in range(reps + 1):
        ix = restore(lambda x: (x.loadCoarseQuantizer(coarse), x.loadProductQuantizer(pq), x.setW(8)))
        ix.search_batch(10, Q)
        ix.search_batch(10, Q)
        remove(ix, d_req, True)
        ts = []
        for _ in range(2):
            t0 = time.perf_counter()
            ix.search_batch(10, Q)
            ts.append((time.perf_counter() - t0) * 1e3)
        for _ in range(2):
            t0 = time.perf_counter()
            N.check(L.mmidx_get_codes(ix._h, 1, one.ctypes.data, None, None))
            ts.append((time.perf_counter() - t0) * 1e3)
        d = ix.get_dispatch()
        ix.close()
        if r > 0:
            for lst, v in zip((s1, s2, g1, g2), ts):
                lst.append(v)
    return {"search_first": spread(s1), "search_second": spread(s2), "get_codes_first": spread(g1), "get_codes_second": spread(g2),
            "pass_b": d["pass_b"], "queries": 64, "w": 8, "k": 10}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs="+", default=["cfg3"], choices=sorted(SHAPES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="write the figures as JSON to this file as well")
    a = ap.parse_args()
    import torch

    mi = importlib.import_module("multimedia-indexing_amd")
    N = importlib.import_module("multimedia-indexing_amd._native")
    if mi.lib().mmidx_device_count() < 1:
        raise SystemExit("remove_scale needs an MI355X: there is no CPU path to time")
    out = {}
    for name in a.shape:
        out[name] = run_shape(mi, N, torch, name, a.reps)
        torch.cuda.empty_cache()
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
