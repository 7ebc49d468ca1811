"""The re-indexing walk at scale (mmidx_linear_reindex) against the chain it replaces, in one process.

    python tools/reindex_scale.py [--shape cfg3 long] [--n 1000000] [--reps 5]

Shapes: cfg3  n x 128 -> 64 into an IVFPQ index (BASELINE config 3: C = 1024, m = 16 x 256)
        long  n x 1024 -> 128 into an IVFPQ index and a Linear index of 128 (the reference's long-vector shape)
Per shape:
  walk      mmidx_linear_reindex over all rows into fresh targets (default chunk), host clock around the synchronous call
  chain     what examples/index_transformation.py did before the walk existed: mmidx_linear_copy_rows_device, torch slice / vector_norm /
            divide, mmidx_add_vectors_device (and mmidx_linear_add_device), in chunks of 8192 rows as that example had them, and once
            more in chunks of the walk's size; host clock around the loop and a device synchronise
  The three alternate inside every one of `reps` rounds after one warm-up round; median and spread (min, max) of each.
  parity    4096 sampled rows of the walk's Linear target against the numpy twin (tests/reindex_twin.py), bit for bit; the number of
            records whose (cell, code) differs between the walk's index and the chain's (torch's norm is not the reference's sum)
  kernel    mmidx_truncate_l2_device alone over all rows (HIP events, one warm-up, 7 repeats): its time, and its bytes -- n max(lens) 8
            read plus the targets written -- per second, beside the 8 TB/s peak and the 6.29 TB/s measured copy ceiling; its share of
            the walk
--shape band: the kernel alone where its kept rows leave one block per CU (L = 160, 256, 288 of 512 columns), against its streamed form.
One JSON object on stdout."""
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

PEAK_TBS, COPY_CEILING_TBS = 8.0, 6.29
SHAPES = {"cfg3": (128, 64, False), "long": (1024, 128, True)}  # D, T, with a Linear target


def spread(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "reps": len(ts)}


def by_iid(off, iids, codes):
    """list-major export -> (cell, code) per internal id"""
    cells = np.repeat(np.arange(len(off) - 1), np.diff(off))
    oc, ok = np.empty(len(iids), np.int64), np.empty_like(codes)
    oc[iids] = cells
    ok[iids] = codes
    return oc, ok


def run_shape(mi, N, torch, name, n, reps):
    import reindex_twin as rx
    import synth

    L = mi.lib()
    D, T, with_linear = SHAPES[name]
    C_, m, ks = 1024, 16, 256
    g = torch.Generator(device="cuda").manual_seed(1234)
    mu = torch.randn((C_, D), dtype=torch.float64, device="cuda", generator=g)
    X = mu[torch.randint(0, C_, (n,), device="cuda", generator=g)]
    X += 0.3 * torch.randn((n, D), dtype=torch.float64, device="cuda", generator=g)
    src = mi.Linear(D, n)
    src.add_device(X)
    torch.cuda.synchronize()
    # codebooks over truncated, normalised vectors of a sample
    S = X[:20000, :T].cpu().numpy()
    S /= np.linalg.norm(S, axis=1, keepdims=True)
    coarse = S[np.random.default_rng(1).choice(len(S), C_, replace=False)]
    cell = ((S * S).sum(1)[:, None] - 2 * S @ coarse.T + (coarse * coarse).sum(1)[None]).argmin(1)
    resid = coarse[cell] - S
    ds = T // m
    pq = np.stack([synth.kmeans(resid[:, s * ds:(s + 1) * ds], ks, iters=3, seed=s) for s in range(m)])

    def targets():
        ix = mi.IVFPQ(T, n, False, "", m, ks, 0, C_, 512)
        ix.loadCoarseQuantizer(coarse)
        ix.loadProductQuantizer(pq)
        return ([mi.Linear(T, n)] if with_linear else []) + [ix]

    def walk(tg):
        kinds = np.array([0 if isinstance(t, mi.Linear) else 1 for t in tg], np.int32)
        hs = (C.c_void_p * len(tg))(*[t._h for t in tg])
        modes = np.full(len(tg), 2, np.int32)
        t0 = time.perf_counter()
        N.check(L.mmidx_linear_reindex(src._h, 0, n, None, len(tg), kinds.ctypes.data, C.addressof(hs), modes.ctypes.data, 0))
        return (time.perf_counter() - t0) * 1e3

    def chain(tg, chunk):
        ix = tg[-1]
        buf = torch.empty((chunk, D), dtype=torch.float64, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i0 in range(0, n, chunk):
            nb = min(chunk, n - i0)
            src.copy_rows_device(i0, buf[:nb])
            y = buf[:nb, :T].contiguous()
            y = (y / torch.linalg.vector_norm(y, dim=1, keepdim=True)).contiguous()
            N.check(L.mmidx_add_vectors_device(ix._h, nb, y.data_ptr(), None, i0, st))
            if with_linear:
                tg[0].add_device(y)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    walk_chunk = min(1 << 20, max(4096, (1 << 25) // T)) // 64 * 64  # the walk's default: sized by the longest target
    variants = {"walk": walk, "chain_8192": lambda tg: chain(tg, 8192), "chain_walk_chunk": lambda tg: chain(tg, walk_chunk)}
    times = {v: [] for v in variants}
    kept = {}
    for r in range(reps + 1):  # round 0 warms every shape up
        for v, f in variants.items():
            tg = targets()
            ms = f(tg)
            if r > 0:
                times[v].append(ms)
            if r == reps and v in ("walk", "chain_8192"):
                kept[v] = tg
            else:
                for t in tg:
                    t.close()
    out = {"n": n, "D": D, "T": T, "linear_target": with_linear, "C": C_, "m": m, "ks": ks, "walk_chunk_rows": walk_chunk}
    out.update({v: spread(ts) for v, ts in times.items()})
    # parity: the walk's rows against the twin; its records against the chain's
    rng = np.random.default_rng(7)
    ids = np.sort(rng.choice(n, 4096, replace=False))
    if with_linear:
        lin = kept["walk"][0]
    else:  # (the shape has no Linear target: one more, untimed walk with one)
        lin = mi.Linear(T, n)
        walk([lin])
    rows = X[torch.from_numpy(ids).cuda()].cpu().numpy()
    got = np.stack([lin.getVector(int(i)) for i in ids])
    out["twin_rows_checked"] = len(ids)
    out["twin_rows_differing"] = int((got.view(np.uint64) != rx.truncate_l2(rows, [T], [2])[0].view(np.uint64)).any(axis=1).sum())
    if not with_linear:
        lin.close()
    wc, wk = by_iid(*kept["walk"][-1].export())
    cc, ck = by_iid(*kept["chain_8192"][-1].export())
    out["records"] = len(wc)
    out["records_differing_from_chain"] = int(((wc != cc) | (wk != ck).any(axis=1)).sum())
    for tg in kept.values():
        for t in tg:
            t.close()
    # the kernel alone
    lens = [T, T] if with_linear else [T]
    outs = [torch.empty((n, t), dtype=torch.float64, device="cuda") for t in lens]
    ptrs = (C.c_void_p * len(lens))(*[o.data_ptr() for o in outs])
    la, ma = np.array(lens, np.int32), np.full(len(lens), 2, np.int32)
    s = torch.cuda.Stream()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(7)]
    with torch.cuda.stream(s):
        N.check(L.mmidx_truncate_l2_device(0, n, D, D, X.data_ptr(), len(lens), la.ctypes.data, ma.ctypes.data, C.addressof(ptrs), s.cuda_stream))
        s.synchronize()
        for e in ev:
            e[0].record(s)
            N.check(L.mmidx_truncate_l2_device(0, n, D, D, X.data_ptr(), len(lens), la.ctypes.data, ma.ctypes.data, C.addressof(ptrs), s.cuda_stream))
            e[1].record(s)
        s.synchronize()
    k = spread([e[0].elapsed_time(e[1]) for e in ev])
    nbytes = n * max(lens) * 8 + sum(n * t * 8 for t in lens)
    k.update({"bytes": nbytes, "TBs": nbytes / (k["median_ms"] * 1e-3) / 1e12, "peak_TBs": PEAK_TBS, "copy_ceiling_TBs": COPY_CEILING_TBS})
    k["share_of_copy_ceiling"] = k["TBs"] / COPY_CEILING_TBS
    k["share_of_walk"] = k["median_ms"] / out["walk"]["median_ms"]
    out["kernel"] = k
    src.close()
    return out


def run_band(mi, N, torch, n, reps=7):
    """K12 alone at L = 160, 256 and 288 out of 512 columns, where the rows kept in LDS leave one block per CU: that form against the
    streamed one (MMIDX_TRL_CACHED_MAX = 288 / 0), the two alternating inside every repeat; and L = 128 for the neighbouring band"""
    L = mi.lib()
    D = 512
    X = torch.randn((n, D), dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    s = torch.cuda.Stream()
    out = {"n": n, "D": D}
    for T in (128, 160, 256, 288):
        Y = torch.empty((n, T), dtype=torch.float64, device="cuda")
        ptrs = (C.c_void_p * 1)(Y.data_ptr())
        la, ma = np.array([T], np.int32), np.array([1], np.int32)
        forms = {"kept_in_lds": "288", "streamed": "0"}
        ts, ref = {f: [] for f in forms}, {}

        def launch():
            N.check(L.mmidx_truncate_l2_device(0, n, D, D, X.data_ptr(), 1, la.ctypes.data, ma.ctypes.data, C.addressof(ptrs), s.cuda_stream))

        with torch.cuda.stream(s):
            for r in range(reps + 1):
                for f, env in forms.items():
                    os.environ["MMIDX_TRL_CACHED_MAX"] = env
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(s)
                    launch()
                    e1.record(s)
                    s.synchronize()
                    if r == 0:
                        ref[f] = Y[::997].clone()
                    else:
                        ts[f].append(e0.elapsed_time(e1))
        os.environ.pop("MMIDX_TRL_CACHED_MAX", None)
        nbytes = 2 * n * T * 8
        row = {f: dict(spread(t), TBs=nbytes / (statistics.median(t) * 1e-3) / 1e12) for f, t in ts.items()}
        row["same_bits"] = bool(torch.equal(ref["kept_in_lds"].view(torch.int64), ref["streamed"].view(torch.int64)))
        out[str(T)] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs="+", default=["cfg3", "long"], choices=sorted(SHAPES) + ["band"])
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch

    mi = importlib.import_module("multimedia-indexing_amd")
    N = importlib.import_module("multimedia-indexing_amd._native")
    if mi.lib().mmidx_device_count() < 1:
        raise SystemExit("reindex_scale needs an MI355X: there is no CPU path to time")
    out = {}
    for name in a.shape:
        out[name] = run_band(mi, N, torch, a.n) if name == "band" else run_shape(mi, N, torch, name, a.n, a.reps)
        print(json.dumps({name: out[name]}), flush=True)
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
