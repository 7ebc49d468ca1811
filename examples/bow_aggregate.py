#!/usr/bin/env python3
"""Bag-of-words vectors for a batch of images on one MI355X (the reference's BowAggregator(codebook) / BowAggregator(codebook, k),
J/aggregation/BowAggregator.java), hard and soft, with the figures DESIGN.md section 5.7 quotes:

  * images/s and descriptors/s of mmidx_bow_aggregate_device on device-resident inputs: HIP events around the call on a
    non-default stream, after warm-up, median of the repeats;
  * the share of the call spent in the assignment (mmidx_assign_device / mmidx_coarse_device timed alone on the same
    descriptors, on an index handle of its own) against the rest (histogram, memset, conversion);
  * the host-pointer figure (BowAggregator.aggregate_batch: staging copies included, host clock);
  * two yardsticks from the same run: raw VLAD with two_pass = 1 on the same descriptors, and the CPU restatement
    (tests/bow_twin.py over the C oracle) on 16 threads.
A sample of images is compared with the CPU restatement, bit for bit.

  python examples/bow_aggregate.py                      # the four shapes of section 5.7
  python examples/bow_aggregate.py --nc 4096 --dl 64 --images 512 --k 1 3
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _event_ms(torch, stream, fn, warmup, repeats):
    """median over `repeats` of the device time of fn() (enqueued on `stream`), after `warmup` untimed calls"""
    times = []
    with torch.cuda.stream(stream):
        for i in range(warmup + repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            if i >= warmup:
                times.append(a.elapsed_time(b))
    return statistics.median(times), times


def run_shape(mi, torch, oracle, nc, dl, n_images, n_desc, ks, warmup=2, repeats=5, verify=4, cpu_images=8, vlad=False, seed=0, verbose=True):
    from bow_twin import BowTwin

    N = mi._native
    L = mi.lib()
    rng = np.random.default_rng(seed)
    cb = rng.standard_normal((nc, dl))
    total = n_images * n_desc
    descs = rng.standard_normal((total, dl))
    descs /= np.linalg.norm(descs, axis=1, keepdims=True)
    off = (np.arange(n_images + 1, dtype=np.int64) * n_desc)
    sets = [descs[off[i]:off[i + 1]] for i in range(n_images)]
    dev = torch.device("cuda:0")
    d_off, d_descs = torch.from_numpy(off).to(dev), torch.from_numpy(descs).to(dev)
    d_out = torch.empty((n_images, nc), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device=dev)
    sp = C.c_void_p(st.cuda_stream)
    res = {"nc": nc, "dl": dl, "images": n_images, "descriptors_per_image": n_desc, "runs": []}
    for k in ks:
        agg = mi.BowAggregator(cb, k)

        def call():
            N.check(L.mmidx_bow_aggregate_device(agg._h, n_images, d_off.data_ptr(), d_descs.data_ptr(), n_desc, d_out.data_ptr(), sp))

        ms, all_ms = _event_ms(torch, st, call, warmup, repeats)
        out = d_out.cpu().numpy()
        # the assignment alone: the same entry point the aggregator drives, on an index handle of its own
        h = C.c_void_p()
        asg_ms = None
        if nc >= 2:
            N.check(L.mmidx_create(N.KIND_IVFPQ, dl, 1, 2, nc, N.TR_NONE, None, None, 0, C.byref(h)))
            N.check(L.mmidx_set_coarse(h, cb.ctypes.data))
            N.check(L.mmidx_set_pq(h, np.zeros((2, dl)).ctypes.data))
            N.check(L.mmidx_set_w(h, k))
            d_cells = torch.empty((total, k), dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            if k == 1:
                asg_ms, _ = _event_ms(torch, st, lambda: N.check(L.mmidx_assign_device(h, total, d_descs.data_ptr(), d_cells.data_ptr(), sp)), warmup, repeats)
            else:
                asg_ms, _ = _event_ms(torch, st, lambda: N.check(L.mmidx_coarse_device(h, total, d_descs.data_ptr(), d_cells.data_ptr(), None, sp)), warmup, repeats)
            L.mmidx_destroy(h)
            del d_cells
        # host pointers: staging copies and the dense read-back included
        t_host = []
        for i in range(1 + 3):
            t0 = time.perf_counter()
            host_out = agg.aggregate_batch(sets)
            if i:
                t_host.append(time.perf_counter() - t0)
        assert np.array_equal(host_out, out), "host and device forms differ"
        # a sample of images against the CPU restatement, bit for bit
        tw = BowTwin(oracle, cb, k)
        pick = sorted(set(int(i) for i in np.linspace(0, n_images - 1, verify)))
        for i in pick:
            assert np.array_equal(out[i], tw.aggregate(sets[i])), f"image {i} differs from the CPU restatement (k = {k})"
        # the CPU restatement on 16 threads (the C oracle releases the GIL; the per-descriptor call overhead is part of the figure)
        ncpu = min(cpu_images, n_images)
        t0 = time.perf_counter()
        with ThreadPoolExecutor(16) as ex:
            list(ex.map(lambda s: BowTwin(oracle, cb, k).aggregate(s), sets[:ncpu]))
        t_cpu = time.perf_counter() - t0
        r = {"k": k, "device_ms": ms, "device_ms_all": all_ms, "images_per_s": n_images / ms * 1e3, "descriptors_per_s": total / ms * 1e3,
             "assignment_ms": asg_ms, "assignment_share": (asg_ms / ms) if asg_ms is not None else None,
             "host_ms": statistics.median(t_host) * 1e3, "host_images_per_s": n_images / statistics.median(t_host),
             "cpu16_descriptors_per_s": ncpu * n_desc / t_cpu, "cpu16_images_per_s": ncpu / t_cpu, "verified_images": pick}
        res["runs"].append(r)
        if verbose:
            print(json.dumps({**{x: res[x] for x in ("nc", "dl", "images", "descriptors_per_image")}, **r}), flush=True)
        agg.close()
    if vlad:  # yardstick: raw VLAD, assignment kernel + accumulation kernel, on the same descriptors (dl times the output)
        v = mi.VladAggregator(cb)
        v.set_option("two_pass", 1)
        d_vout = torch.empty((n_images, nc * dl), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        ms, all_ms = _event_ms(torch, st, lambda: N.check(L.mmidx_vlad_aggregate_device(v._h, n_images, d_off.data_ptr(), d_descs.data_ptr(), n_desc,
                                                                                       d_vout.data_ptr(), sp)), warmup, repeats)
        res["vlad_two_pass"] = {"device_ms": ms, "device_ms_all": all_ms, "images_per_s": n_images / ms * 1e3, "descriptors_per_s": total / ms * 1e3}
        if verbose:
            print(json.dumps({"nc": nc, "dl": dl, "images": n_images, "vlad_two_pass": res["vlad_two_pass"]}), flush=True)
        v.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nc", type=int, default=0, help="vocabulary size (0: the two shapes of DESIGN.md section 5.7)")
    ap.add_argument("--dl", type=int, default=64)
    ap.add_argument("--images", type=int, default=0)
    ap.add_argument("--desc", type=int, default=1000, help="descriptors per image")
    ap.add_argument("--k", type=int, nargs="+", default=[1, 3])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="write the results as JSON to this file")
    a = ap.parse_args()
    import torch

    from oracle import oracle

    oracle.build()
    mi = importlib.import_module("multimedia-indexing_amd")
    if mi.lib().mmidx_device_count() < 1:
        raise SystemExit("bow_aggregate.py needs an MI355X: libmmidx_hip has no CPU fallback")
    torch.cuda.init()
    if a.nc:
        shapes = [(a.nc, a.dl, a.images or 1024, a.nc <= 128)]
    else:
        # 128 words: 2048 images x 1000 descriptors = 1 GiB of descriptors, 8000 blocks of the assignment kernel on 256 CUs;
        # 65536 words: the assignment is 512 times the work per descriptor, 48 images keep a call near a second
        shapes = [(128, a.dl, a.images or 2048, True), (65536, a.dl, a.images or 48, False)]
    results = [run_shape(mi, torch, oracle, nc, dl, ni, a.desc, a.k, repeats=a.repeats, vlad=vl, verify=2 if nc > 4096 else 4,
                         cpu_images=16 if nc > 4096 else 64) for nc, dl, ni, vl in shapes]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
    return results


if __name__ == "__main__":
    main()
