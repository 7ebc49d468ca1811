"""CPU checks of the streaming PCA learner's boundary (mmidx_pca_stream_*, frontend.PCA.streaming, mmidx_probe_sym_eig) and of the
host-compilable half of the device eigen-solver (csrc/mmidx_jacobi.h: the pair schedule and the rotation), which a stand-alone
program built with the address and undefined-behaviour sanitizers runs in a host loop."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def mi():
    m = importlib.import_module("multimedia-indexing_amd")
    m.build()
    return m


def test_symbols_and_abi(mi):
    L = mi.lib()
    for name in ("mmidx_pca_stream_create", "mmidx_pca_stream_add", "mmidx_pca_stream_add_device", "mmidx_pca_stream_count",
                 "mmidx_pca_stream_compute", "mmidx_pca_stream_destroy", "mmidx_probe_sym_eig"):
        assert hasattr(L, name), name
    assert L.mmidx_abi_version() == 8  # (adding symbols breaks no caller)


def test_c_abi_argument_errors(mi):
    L = mi.lib()
    h = C.c_void_p()
    assert L.mmidx_pca_stream_create(4, 8, 0, None) == 6  # null out
    assert L.mmidx_pca_stream_create(0, 8, 0, C.byref(h)) == 6 and not h.value
    assert L.mmidx_pca_stream_create(9, 8, 0, C.byref(h)) == 6  # PCA.java:102-104
    assert L.mmidx_last_error() == b"More components requested than the data's length."
    assert not h.value
    # outside the envelope: never a silent fallback
    assert L.mmidx_pca_stream_create(4, 32769, 0, C.byref(h)) == 10 and not h.value
    assert L.mmidx_pca_stream_create(1025, 2048, 0, C.byref(h)) == 10 and not h.value
    buf = (C.c_double * 8)()
    n = C.c_int64(-1)
    assert L.mmidx_pca_stream_add(None, 1, C.addressof(buf)) == 6
    assert L.mmidx_pca_stream_add_device(None, 1, C.addressof(buf), None) == 6
    assert L.mmidx_pca_stream_count(None, C.byref(n)) == 6 and n.value == -1
    assert L.mmidx_pca_stream_compute(None, 1e-12, 10, None, None, None, None, None) == 6
    assert L.mmidx_pca_stream_destroy(None) == 0
    # the eigen-solver probe: its own envelope, before any device call
    assert L.mmidx_probe_sym_eig(0, 4, None, None, None, None) == 6
    assert L.mmidx_probe_sym_eig(0, 0, C.addressof(buf), None, None, None) == 6
    assert L.mmidx_probe_sym_eig(0, 1057, C.addressof(buf), None, None, None) == 6
    # a valid shape (the old learner refuses it: ss > 16384): a handle on a GPU box, NO_DEVICE without one -- never a host computation
    st = L.mmidx_pca_stream_create(4, 16448, 0, C.byref(h))
    if L.mmidx_device_count() < 1:
        assert st == 8 and not h.value
        one = (C.c_double * 1)(1.0)
        assert L.mmidx_probe_sym_eig(0, 1, C.addressof(one), C.addressof(buf), None, None) == 8
    else:
        assert st == 0 and h.value
        assert L.mmidx_pca_stream_count(h, C.byref(n)) == 0 and n.value == 0
        assert L.mmidx_pca_stream_destroy(h) == 0


def test_staging_rows_override_is_validated(mi, monkeypatch):
    L = mi.lib()
    h = C.c_void_p()
    for bad in ("7", "12", "0", "-8", "x", "64k"):
        monkeypatch.setenv("MMIDX_PCA_STREAM_ROWS", bad)
        assert L.mmidx_pca_stream_create(4, 8, 0, C.byref(h)) == 6 and b"MMIDX_PCA_STREAM_ROWS" in L.mmidx_last_error()
        assert not h.value


def test_streaming_messages_before_any_device_call(mi):
    def msg(fn, *a):
        with pytest.raises(mi.MmidxError) as ei:
            fn(*a)
        return str(ei.value), ei.value.status

    assert msg(mi.PCA.streaming, 9, 8, False) == ("More components requested than the data's length.", 6)
    p = mi.PCA.streaming(2, 4, False)
    assert msg(p.addSample, np.zeros(5)) == ("Unexpected sample size", 2)       # PCA.java:123-124
    assert msg(p.addSamples, np.zeros((3, 5))) == ("Unexpected sample size", 2)
    assert msg(p.addSamples, np.zeros(4)) == ("Unexpected sample size", 2)
    assert msg(p.computeBasis) == ("More data needed to compute the desired number of components", 6)  # :138-140
    assert msg(p.savePCAToFile, "unused") == ("Cannot save to file, PCA matrix is null!", 7)
    assert p.numTrainingSamples == 0 and p.sampleIndex == 0
    p.addSamples(np.zeros((0, 4)))  # nothing to add: no handle is made
    assert p._learner is None
    p.close()
    # the resident form is what it was
    q = mi.PCA(2, 0, 4, False)
    assert msg(q.addSample, np.zeros(4)) == ("Too many samples", 6)


_HARNESS = r"""
#include "mmidx_jacobi.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
namespace J = mmidx_jacobi;
// every pair {i, j}, i < j < b, exactly once per sweep; pairs of a step are disjoint
static int schedule_ok(int b) {
    const int n = J::slots(b);
    if (n < b || n > b + 1 || (n & 1)) return 0;
    std::vector<int> seen((size_t)n * n, 0);
    for (int s = 0; s < n - 1; s++) {
        std::vector<int> used((size_t)n, 0);
        for (int k = 0; k < n / 2; k++) {
            int p, q;
            J::pair_of(n, s, k, &p, &q);
            if (p < 0 || q >= n || p >= q) return 0;
            if (used[p]++ || used[q]++) return 0;
            seen[(size_t)p * n + q]++;
        }
    }
    for (int i = 0; i < n; i++)
        for (int j = i + 1; j < n; j++)
            if (seen[(size_t)i * n + j] != 1) return 0;
    return 1;
}
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const int b = atoi(argv[1]);
    const int sched = schedule_ok(b);
    // A = B B^T, B from the xorshift of the host-solver harness
    std::vector<double> B((size_t)b * b), A((size_t)b * b), T, W((size_t)b * b, 0.0);
    unsigned long long x = 88172645463325252ull;
    for (auto &v : B) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; v = (double)(x >> 11) * 0x1p-53 - 0.5; }
    for (int i = 0; i < b; i++)
        for (int j = 0; j < b; j++) {
            double s = 0;
            for (int k = 0; k < b; k++) s += B[(size_t)i * b + k] * B[(size_t)j * b + k];
            A[(size_t)i * b + j] = s;
        }
    T = A;
    for (int i = 0; i < b; i++) W[(size_t)i * b + i] = 1.0;
    double all = 0;
    for (double v : T) all = std::max(all, std::fabs(v));
    const int n = J::slots(b);
    int sweeps = 0;
    const double level = std::sqrt((double)b) * 0x1p-52 * all;  // the device solver's stopping level
    for (; sweeps <= 30; sweeps++) {
        double off = 0;
        for (int i = 0; i < b; i++)
            for (int j = 0; j < b; j++)
                if (i != j) off = std::max(off, std::fabs(T[(size_t)i * b + j]));
        if (off <= level) break;
        for (int s = 0; s < n - 1; s++)
            for (int k = 0; k < n / 2; k++) {  // (pairs of a step are disjoint: one after the other equals all at once)
                int p, q;
                J::pair_of(n, s, k, &p, &q);
                if (q >= b) continue;
                const double app = T[(size_t)p * b + p], aqq = T[(size_t)q * b + q], apq = T[(size_t)p * b + q];
                const J::Rot r = J::rotation(app, aqq, apq);
                for (int j = 0; j < b; j++) J::rotate(r, &T[(size_t)p * b + j], &T[(size_t)q * b + j]);  // J^T T
                for (int i = 0; i < b; i++) J::rotate(r, &T[(size_t)i * b + p], &T[(size_t)i * b + q]);  // ... J
                for (int j = 0; j < b; j++) J::rotate(r, &W[(size_t)p * b + j], &W[(size_t)q * b + j]);  // Wt <- J^T Wt
                // the pair's own block, as the device kernel writes it: the annihilated entry is 0, not its rounding residue
                T[(size_t)p * b + p] = app - r.t * apq;
                T[(size_t)q * b + q] = aqq + r.t * apq;
                T[(size_t)p * b + q] = T[(size_t)q * b + p] = 0.0;
            }
    }
    double res = 0, orth = 0, lmax = 0;
    for (int i = 0; i < b; i++) lmax = std::max(lmax, T[(size_t)i * b + i]);
    for (int i = 0; i < b; i++) {
        double r = 0;
        for (int k = 0; k < b; k++) {
            double s = 0;
            for (int j = 0; j < b; j++) s += A[(size_t)k * b + j] * W[(size_t)i * b + j];
            s -= T[(size_t)i * b + i] * W[(size_t)i * b + k];
            r += s * s;
        }
        res = std::max(res, std::sqrt(r));
        for (int j = 0; j <= i; j++) {
            double s = 0;
            for (int k = 0; k < b; k++) s += W[(size_t)i * b + k] * W[(size_t)j * b + k];
            orth = std::max(orth, std::fabs(s - (i == j)));
        }
    }
    printf("%d %d %.17g %.17g", sched, sweeps, lmax > 0 ? res / lmax : 0.0, orth);
    for (int i = 0; i < b; i++) printf(" %.17g", T[(size_t)i * b + i]);
    printf("\n");
    return 0;
}
"""


def harness_gram(b):
    """A = B B^T with B from the xorshift of the C harnesses (here and in test_pca_learn_cpu.py)"""
    x, M, vals = 88172645463325252, (1 << 64) - 1, []
    for _ in range(b * b):
        x ^= (x << 13) & M
        x ^= x >> 7
        x ^= (x << 17) & M
        vals.append((x >> 11) * 2.0 ** -53 - 0.5)
    B = np.array(vals).reshape(b, b)
    return B @ B.T


def test_jacobi_helpers_under_sanitizers(tmp_path):
    """csrc/mmidx_jacobi.h compiled by plain g++: the round-robin schedule visits each of the b (b - 1) / 2 pairs exactly once per
    sweep, in steps of disjoint pairs; a host loop over the same rotation diagonalises a 40 x 40 Gram matrix to the bounds the
    device solver is held to (residual, orthogonality, eigenvalues: 30 b eps of the largest eigenvalue)."""
    src, exe = str(tmp_path / "jacobi.cpp"), str(tmp_path / "jacobi")
    open(src, "w").write(_HARNESS)
    # the sanitizer runtimes are linked statically: the program needs no option to start beside whatever else a process preloads
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "multimedia-indexing_amd", "csrc"), src, "-o", exe])
    env = dict(os.environ)
    env.pop("ASAN_OPTIONS", None)
    for b in (2, 3, 4, 37, 64):
        out = subprocess.check_output([exe, str(b)], env=env, text=True).split()
        assert out[0] == "1", f"schedule for b = {b}"
    out = subprocess.check_output([exe, "40"], env=env, text=True).split()
    b = 40
    sched, sweeps, res, orth = int(out[0]), int(out[1]), float(out[2]), float(out[3])
    lam = np.sort(np.array(out[4:], dtype=np.float64))[::-1]
    ref = np.linalg.eigvalsh(harness_gram(b))[::-1]
    print(f"host Jacobi, b = {b}: {sweeps} sweeps, residual {res:.3e}, orthogonality {orth:.3e}, "
          f"eigenvalues {np.max(np.abs(lam - ref)) / ref[0]:.3e} (bound {30 * b * EPS:.3e})")
    assert sched == 1 and 1 <= sweeps <= 30
    assert res <= 30 * b * EPS and orth <= 30 * b * EPS
    assert np.max(np.abs(lam - ref)) <= 30 * b * EPS * ref[0]
