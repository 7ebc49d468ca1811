"""PCA learning at scale: samples generated on the device (a planted low-rank signal plus noise, in chunks), then either learner.

    python tools/pca_learn_scale.py [--n 10000] [--ss 4096] [--nc 1024] [--streaming] [--solve host|device] [--lib PATH]
                                    [--chunk 2048] [--rank R] [--tol 1e-10] [--max-iter 200] [--probe-eig B ...]

Prints one JSON line: seconds to add the samples (streaming: the folds, with their rate in TF/s executed against the
mmidx_probe_f64_mfma ceiling measured in the same run, and the Gram-matrix bytes a fold moves), seconds of computeBasis, its
iterations and residual, what the library's trace line says about the b x b solves, and the peak device memory.
--lib points it at another build of libmmidx_hip.so (an older one has neither the streaming learner nor the device solves: the
resident learner is all it can run).  --probe-eig times mmidx_probe_sym_eig alone at the given sizes."""
import argparse
import ctypes as C
import json
import os
import re
import sys
import tempfile
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GR_BM, GR_BN = 64, 128  # k_pca_gram's tile


def executed_tiles(ss):
    return sum(1 for i0 in range(0, ss, GR_BM) for j0 in range(0, ss, GR_BN) if i0 + GR_BM - 1 >= j0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--ss", type=int, default=4096)
    ap.add_argument("--nc", type=int, default=1024)
    ap.add_argument("--rank", type=int, default=0, help="rank of the planted signal (default nc + 64)")
    ap.add_argument("--chunk", type=int, default=2048)
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--max-iter", type=int, default=200)
    ap.add_argument("--streaming", action="store_true")
    ap.add_argument("--solve", choices=["host", "device"], default=None)
    ap.add_argument("--probe-eig", type=int, nargs="*", default=[])
    ap.add_argument("--lib", default=os.path.join(ROOT, "multimedia-indexing_amd", "csrc", "libmmidx_hip.so"))
    a = ap.parse_args()
    import numpy as np
    import torch  # binds the HIP runtime torch ships before the library loads, as the package does

    torch.cuda.init()
    L = C.CDLL(a.lib)
    vp, dp = C.c_void_p, C.c_void_p
    L.mmidx_last_error.restype = C.c_char_p

    def ck(st):
        if st:
            raise SystemExit(f"status {st}: {L.mmidx_last_error().decode()}")

    os.environ["MMIDX_PCA_LEARN_TRACE"] = "1"
    if a.solve:
        os.environ["MMIDX_PCA_LEARN_SOLVE"] = a.solve
    out = {"lib": os.path.relpath(a.lib, ROOT), "n": a.n, "ss": a.ss, "nc": a.nc, "b": min(a.ss, a.nc + 32), "streaming": a.streaming,
           "solve": a.solve or "default", "tol": a.tol}
    v = (C.c_double * 2)()
    L.mmidx_probe_f64_mfma.argtypes = [C.c_int, dp]
    ck(L.mmidx_probe_f64_mfma(0, C.addressof(v)))
    out["f64_mfma_tf"] = round(v[0], 2)

    if a.probe_eig:
        L.mmidx_probe_sym_eig.argtypes = [C.c_int, C.c_int, dp, dp, dp, C.POINTER(C.c_int32)]
        rng = np.random.default_rng(1)
        rows = []
        for b in a.probe_eig:
            B = rng.standard_normal((b, b)) / np.sqrt(b)
            T = np.ascontiguousarray(B @ B.T)
            lam, Wt, sw = np.zeros(b), np.zeros((b, b)), C.c_int32(0)
            ck(L.mmidx_probe_sym_eig(0, b, T.ctypes.data, lam.ctypes.data, Wt.ctypes.data, C.byref(sw)))  # (warm: allocations, code load)
            t0 = time.perf_counter()
            ck(L.mmidx_probe_sym_eig(0, b, T.ctypes.data, lam.ctypes.data, Wt.ctypes.data, C.byref(sw)))
            rows.append({"b": b, "seconds": round(time.perf_counter() - t0, 4), "sweeps": sw.value})
        out["probe_sym_eig"] = rows
        print(json.dumps(out))
        return

    # samples: x = z B + noise + offset, z ~ N(0, diag(s^2)), s geometric with a step after nc
    r = a.rank or a.nc + 64
    g = torch.Generator(device="cuda").manual_seed(7)
    Bm = torch.randn((r, a.ss), dtype=torch.float64, device="cuda", generator=g) / (a.ss ** 0.5)
    s = 0.995 ** torch.arange(r, dtype=torch.float64, device="cuda")
    s[a.nc:] /= 2.0
    offset = 0.05 * torch.randn(a.ss, dtype=torch.float64, device="cuda", generator=g)

    def chunk_rows(m):
        z = torch.randn((m, r), dtype=torch.float64, device="cuda", generator=g) * s
        return torch.addmm(offset.expand(m, -1), z, Bm) + 1e-3 * torch.randn((m, a.ss), dtype=torch.float64, device="cuda", generator=g)

    free0, total = torch.cuda.mem_get_info()
    low = [free0]
    stop = threading.Event()

    def watch():
        while not stop.wait(0.05):
            low[0] = min(low[0], torch.cuda.mem_get_info()[0])

    th = threading.Thread(target=watch, daemon=True)
    th.start()
    h = vp()
    if a.streaming:
        L.mmidx_pca_stream_create.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
        L.mmidx_pca_stream_add_device.argtypes = [vp, C.c_int64, dp, vp]
        L.mmidx_pca_stream_compute.argtypes = [vp, C.c_double, C.c_int, dp, dp, dp, C.POINTER(C.c_int32), C.POINTER(C.c_double)]
        L.mmidx_pca_stream_destroy.argtypes = [vp]
        ck(L.mmidx_pca_stream_create(a.nc, a.ss, 0, C.byref(h)))
        add, compute, destroy = L.mmidx_pca_stream_add_device, L.mmidx_pca_stream_compute, L.mmidx_pca_stream_destroy
    else:
        L.mmidx_pca_learn_create.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_int, C.POINTER(vp)]
        L.mmidx_pca_learn_add_device.argtypes = [vp, C.c_int64, dp, vp]
        L.mmidx_pca_learn_compute.argtypes = [vp, C.c_double, C.c_int, dp, dp, dp, C.POINTER(C.c_int32), C.POINTER(C.c_double)]
        L.mmidx_pca_learn_destroy.argtypes = [vp]
        ck(L.mmidx_pca_learn_create(a.nc, a.n, a.ss, 0, C.byref(h)))
        add, compute, destroy = L.mmidx_pca_learn_add_device, L.mmidx_pca_learn_compute, L.mmidx_pca_learn_destroy
    t_gen = t_add = 0.0
    done = 0
    while done < a.n:
        m = min(a.chunk, a.n - done)
        t0 = time.perf_counter()
        X = chunk_rows(m)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        ck(add(h, m, X.data_ptr(), None))
        torch.cuda.synchronize()
        t_add += time.perf_counter() - t1
        t_gen += t1 - t0
        done += m
    out["generate_seconds"], out["add_seconds"] = round(t_gen, 3), round(t_add, 3)
    if a.streaming:
        R = min(4096, max(64, ((1 << 25) // a.ss) & ~63))
        folds_done = a.n // R  # (the tail is folded by compute)
        tiles = executed_tiles(a.ss)
        flops = 2.0 * folds_done * R * tiles * GR_BM * GR_BN
        out["fold_rows"], out["folds_in_add"] = R, folds_done
        out["fold_tf_executed"] = round(flops / t_add * 1e-12, 2) if t_add > 0 and folds_done else None  # (staging copy and column sums included)
        out["fold_fraction_of_f64_peak"] = round(out["fold_tf_executed"] / v[0], 3) if out["fold_tf_executed"] else None
        out["gram_bytes_per_fold"] = tiles * GR_BM * GR_BN * 8 * 3  # an owned element is read once and written twice (itself, its mirror)
    means, sv, Vt = np.zeros(a.ss), np.zeros(a.nc), np.zeros((a.nc, a.ss))
    it, res = C.c_int32(0), C.c_double(0.0)
    sys.stderr.flush()
    with tempfile.TemporaryFile(mode="w+b") as tf:  # the library's trace goes to stderr: keep a copy to read the solve times from
        saved = os.dup(2)
        os.dup2(tf.fileno(), 2)
        try:
            t0 = time.perf_counter()
            st = compute(h, a.tol, a.max_iter, means.ctypes.data, sv.ctypes.data, Vt.ctypes.data, C.byref(it), C.byref(res))
            t_compute = time.perf_counter() - t0
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tf.seek(0)
        trace = tf.read().decode(errors="replace")
    sys.stderr.write(trace)
    stop.set()
    th.join()
    if st:
        out["message"] = L.mmidx_last_error().decode()
    out.update({"status": st, "compute_seconds": round(t_compute, 3), "iterations": it.value, "residual": res.value,
                "peak_device_bytes": int(total - min(low[0], torch.cuda.mem_get_info()[0])), "device_bytes_before": int(total - free0)})
    for key, pat in (("gram_ms", r"gram ([\d.]+) ms"), ("gram_tf_executed", r"\(([\d.]+) TF/s executed\)"), ("iteration_seconds", r"iterations ([\d.]+) s"),
                     ("host_solve_seconds", r"host solves ([\d.]+) s"), ("device_solves", r"device solves (\d+) in"),
                     ("device_solve_seconds", r"device solves \d+ in ([\d.]+) s"), ("sweeps_per_solve", r"([\d.]+) sweeps per solve")):
        m = re.search(pat, trace)
        if m:
            out[key] = float(m.group(1))
    m = re.search(r"solver (\w+)", trace)
    out["solver"] = m.group(1) if m else "host"
    if it.value:
        out["solve_seconds_per_iteration"] = round((out.get("host_solve_seconds", 0.0) + out.get("device_solve_seconds", 0.0)) / it.value, 4)
    ck(destroy(h))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
