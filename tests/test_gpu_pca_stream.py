"""GPU checks of the streaming PCA learner (mmidx_pca_stream_*: staging block, k_pca_gram's accumulating form, k_pca_shiftsum,
k_pca_finalise, the shared eigenpair loop) and of the dense b x b solves on the device (csrc/mmidx_dense_solve.h, mmidx_probe_sym_eig)
against the numpy twin of tests/pca_learn_twin.py.  The checks are those of tests/test_gpu_pca_learn.py, numbered as there:
  1 means bit-equal to the reference's sequential loop      2 residual against numpy's centred matrix <= 2 TOL sv_1^2
  3 orthonormality <= 16 x LAPACK's own defect              4 singular values: 2 TOL (sv_1 / sv_i)^2 + 16 eps
  5 components (Davis-Kahan with the twin's gaps)           6 identical bytes however the rows arrived, sign rule
Every bound comes from TOL = 1e-11 (the caller's request), from eps, or from LAPACK's defect on the same fixture -- none from what
the library returns.  Above ss = 4096 the Gram matrix is never formed here: residuals are A_c^T (A_c v)."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import pca_learn_twin as T

pytestmark = pytest.mark.gpu
TOL = 1e-11
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def mi():
    try:
        import torch

        torch.cuda.init()
    except Exception:
        pass
    m = importlib.import_module("multimedia-indexing_amd")
    if m.lib().mmidx_device_count() < 1:
        pytest.fail("libmmidx_hip.so found no HIP device: GPU tests must run the native path")
    return m


class Case:
    """a sample matrix with its twin: computed once, shared, never modified"""

    def __init__(self, A, nc):
        self.A, self.nc = A, nc
        self.n, self.ss = A.shape
        self.mu, self.sig, self.Vt = T.twin(A)
        self.Ac = A - self.mu
        for a in (self.A, self.mu, self.sig, self.Vt, self.Ac):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def plain_case(idx, offset=0.0):
    n, ss, nc, decay = T.FIXTURES[idx]
    return Case(T.make_fixture(n, ss, nc, decay, idx) + offset, nc)


@functools.lru_cache(maxsize=None)
def made_case(n, ss, nc, decay, seed):
    return Case(T.make_fixture(n, ss, nc, decay, seed), nc)


def stream_learn(mi, A, nc, splits=None, tol=TOL, max_iter=200, device_stream=False):
    n, ss = A.shape
    p = mi.PCA.streaming(nc, ss, False)
    lo = 0
    if device_stream:
        import torch

        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            for hi in list(splits or []) + [n]:
                d = torch.from_numpy(np.ascontiguousarray(A[lo:hi])).cuda()
                p.add_device(d, hi - lo, st.cuda_stream)
                d.record_stream(st)
                lo = hi
    else:
        for hi in list(splits or []) + [n]:
            p.addSamples(A[lo:hi])
            lo = hi
    p.computeBasis(tol=tol, max_iter=max_iter)
    assert p.numTrainingSamples == n and p.numSamples == n
    return p


def resident_learn(mi, A, nc, tol=TOL, max_iter=200):
    n, ss = A.shape
    p = mi.PCA(nc, n, ss, False)
    p.addSamples(A)
    p.computeBasis(tol=tol, max_iter=max_iter)
    return p


def checks_2_to_5(c, p, tol=TOL, label=""):
    nc, ss = c.nc, c.ss
    sv, Vt = p.singularValues, p.V_t
    assert T.sign_rule_holds(Vt) and np.all(np.diff(sv) <= 0.0)
    # 2. residual against numpy's centred matrix (never the library's Gram matrix): the caller's tol, a factor 2 for the summation orders
    res = float(np.max(np.linalg.norm(c.Ac.T @ (c.Ac @ Vt.T) - Vt.T * sv ** 2, axis=0)))
    print(f"{label} iterations {p.iterations}, residual_out {p.residual:.3e}; residual {res / sv[0] ** 2:.3e} (bound {2 * tol:.1e}) of sv_1^2")
    assert res <= 2 * tol * sv[0] ** 2, (res / sv[0] ** 2, 2 * tol)
    assert p.residual <= tol
    # 3. orthonormality: at most 16 x LAPACK's own defect on this fixture
    d_lib, d_twin = T.ortho_defect(Vt), T.ortho_defect(c.Vt[:nc])
    print(f"  orthogonality defect {d_lib:.3e}, twin {d_twin:.3e}")
    assert d_lib <= 16 * d_twin, f"defect {d_lib:.3e} > 16 x the twin's {d_twin:.3e}"
    # 4. singular values: a Ritz value lies within the residual norm of an eigenvalue
    sig = c.sig
    err = np.abs(sv / sig[:nc] - 1.0)
    bound = 2 * tol * (sig[0] / sig[:nc]) ** 2 + 16 * EPS
    print(f"  singular values: max relative error {err.max():.3e}, worst error / bound {np.max(err / bound):.3e}")
    assert np.all(err <= bound), (float(np.max(err / bound)))
    # 5. components up to sign (Davis-Kahan): gap_i = distance of sigma_i^2 to the nearest other eigenvalue, the (nc+1)-th included
    lam = sig ** 2
    lam_all = np.concatenate([lam, np.zeros(1)]) if lam.shape[0] < ss else lam  # (n < ss: the remaining eigenvalues of G are 0)
    gap = np.array([np.min(np.abs(np.delete(lam_all, i) - lam_all[i])) for i in range(nc)])
    miss = 1.0 - np.abs(np.sum(Vt * c.Vt[:nc], axis=1))
    bound = 0.5 * (2 * tol * lam[0] / gap) ** 2 + 16 * EPS
    print(f"  components: max 1 - |<v, v_twin>| {miss.max():.3e}, worst / bound {np.max(miss / bound):.3e}")
    assert np.all(miss <= bound), (float(np.max(miss / bound)))


def same_bytes(p, q):
    return p.V_t.tobytes() == q.V_t.tobytes() and p.singularValues.tobytes() == q.singularValues.tobytes()


# ---- 1. offset fixtures: what separates a shifted accumulation from uncentred X^T X - n mu mu^T ----
@pytest.mark.parametrize("idx", [0, 2])
def test_offset_fixture(mi, idx):
    c = plain_case(idx, 1000.0)
    p = stream_learn(mi, c.A, c.nc)
    assert np.array_equal(p.means, c.mu)  # 1.
    checks_2_to_5(c, p, label=f"fixture {T.FIXTURES[idx]} + 1000:")
    p.close()


# ---- 2. the result bytes do not depend on how the rows were split over add calls ----
@pytest.mark.parametrize("idx", range(len(T.FIXTURES)))
def test_call_pattern_independence(mi, idx):
    c = plain_case(idx)
    n = c.n
    p = stream_learn(mi, c.A, c.nc)
    q = stream_learn(mi, c.A, c.nc, splits=[n // 7, n // 7 + 1 + n // 3])  # three uneven add calls
    assert np.array_equal(p.means, c.mu) and np.array_equal(q.means, c.mu)  # 1.
    assert same_bytes(p, q)  # 6.
    if idx == 2:  # 300 rows, one per call
        r = mi.PCA.streaming(c.nc, c.ss, False)
        for row in c.A:
            r.addSample(row)
        r.computeBasis(tol=TOL, max_iter=200)
        assert np.array_equal(r.means, c.mu) and same_bytes(p, r) and r.numTrainingSamples == n
        r.close()
    if idx == 0:  # rows already on the device, handed over on a stream that is not the default one
        d = stream_learn(mi, c.A, c.nc, splits=[5, 700], device_stream=True)
        assert np.array_equal(d.means, c.mu) and same_bytes(p, d)
        d.close()
    checks_2_to_5(c, p, label=f"fixture {T.FIXTURES[idx]}:")
    p.close()
    q.close()


# ---- 3. fold boundaries: a staging block smaller than the sample count ----
def test_fold_boundaries(mi, monkeypatch):
    c = plain_case(2)  # 300 rows
    monkeypatch.setenv("MMIDX_PCA_STREAM_ROWS", "64")  # four folds and a 44-row tail
    p = stream_learn(mi, c.A, c.nc, splits=[63, 64, 129, 257])
    assert np.array_equal(p.means, c.mu)
    checks_2_to_5(c, p, label="fixture 2, 64-row folds:")
    q = stream_learn(mi, c.A, c.nc)
    assert same_bytes(p, q)  # the folds are the block's, not the calls'
    cut = Case(np.ascontiguousarray(c.A[:100]), c.nc)
    monkeypatch.setenv("MMIDX_PCA_STREAM_ROWS", "8")  # twelve folds and a 4-row tail
    r = stream_learn(mi, cut.A, cut.nc, splits=[1, 9, 50], max_iter=2000)
    assert np.array_equal(r.means, cut.mu)
    checks_2_to_5(cut, r, label="100 rows of fixture 2, 8-row folds:")
    for o in (p, q, r):
        o.close()


# ---- 4. beyond the resident learner's envelope ----
@pytest.mark.parametrize("shape", [(160, 16448, 8), (192, 32768, 8)])
def test_beyond_the_old_envelope(mi, shape):
    n, ss, nc = shape
    c = made_case(n, ss, nc, 0.9, 7)
    h = C.c_void_p()
    assert mi.lib().mmidx_pca_learn_create(nc, n, ss, 0, C.byref(h)) == 10  # the resident learner still refuses the shape
    p = stream_learn(mi, c.A, nc, splits=[n // 3])
    assert np.array_equal(p.means, c.mu)
    checks_2_to_5(c, p, label=f"{shape}:")
    p.close()


# ---- 5. the device eigen-solver alone ----
def harness_gram(b):
    """B B^T with B from the xorshift of the C harness in test_pca_learn_cpu.py"""
    x, M, vals = 88172645463325252, (1 << 64) - 1, []
    for _ in range(b * b):
        x ^= (x << 13) & M
        x ^= x >> 7
        x ^= (x << 17) & M
        vals.append((x >> 11) * 2.0 ** -53 - 0.5)
    B = np.array(vals).reshape(b, b)
    return B @ B.T


def eig_matrices(b):
    rng = np.random.default_rng(500 + b)
    Q = np.linalg.qr(rng.standard_normal((b, b)))[0]
    graded = (Q * 10.0 ** np.linspace(0.0, -6.0, b)) @ Q.T
    B = rng.standard_normal((b, b // 2))
    h = b // 2
    block = np.zeros((b, b))
    block[:h, :h] = np.eye(h)
    block[h:, h:] = harness_gram(b - h) if b - h <= 160 else (lambda X: X @ X.T)(rng.standard_normal((b - h, b - h)) / np.sqrt(b))
    return {"gram": harness_gram(b), "graded": 0.5 * (graded + graded.T), "rank b/2": B @ B.T, "diagonal": np.diag(rng.standard_normal(b)),
            "identity": np.eye(b), "identity block": block}


def probe(mi, Tm):
    b = Tm.shape[0]
    Tm = np.ascontiguousarray(Tm)
    lam, Wt, sw = np.full(b, -7.0), np.full((b, b), -7.0), C.c_int32(-1)
    st = mi.lib().mmidx_probe_sym_eig(0, b, Tm.ctypes.data, lam.ctypes.data, Wt.ctypes.data, C.byref(sw))
    return st, lam, Wt, sw.value


def check_eig(mi, Tm, label):
    b = Tm.shape[0]
    st, lam, Wt, sweeps = probe(mi, Tm)
    assert st == 0, mi.lib().mmidx_last_error()
    ref = np.linalg.eigvalsh(Tm)[::-1]
    l1 = max(abs(ref[0]), abs(ref[-1]))  # lambda_1 (the diagonal kind alone has negative eigenvalues: its largest magnitude)
    bound = 30 * b * EPS * l1
    res = float(np.max(np.linalg.norm(Tm @ Wt.T - Wt.T * lam, axis=0)))
    orth = float(np.max(np.abs(Wt @ Wt.T - np.eye(b))))
    dist = float(np.max(np.abs(lam - ref)))
    print(f"b {b} {label}: {sweeps} sweeps; residual {res:.2e}, eigenvalues {dist:.2e} (bound {bound:.2e}); orthogonality {orth:.2e} (bound {30 * b * EPS:.2e})")
    assert np.all(np.diff(lam) <= 0.0)
    assert res <= bound and dist <= bound and orth <= 30 * b * EPS
    assert 0 <= sweeps <= 30


@pytest.mark.parametrize("b", [1, 2, 3, 37, 64, 97, 160, 288])
def test_device_eigen_solver(mi, b):
    for label, Tm in eig_matrices(b).items():
        check_eig(mi, Tm, label)


def test_device_eigen_solver_at_the_largest_block(mi):
    check_eig(mi, harness_gram(1056), "gram")


@pytest.mark.parametrize("poison", [np.nan, np.inf])
def test_device_eigen_solver_refuses_non_finite_input(mi, poison):
    Tm = harness_gram(37)
    Tm[3, 5] = Tm[5, 3] = poison
    st, lam, Wt, sweeps = probe(mi, Tm)
    assert st == 6 and b"non-finite" in mi.lib().mmidx_last_error()
    assert np.all(lam == -7.0) and np.all(Wt == -7.0) and sweeps == -1  # nothing written


# ---- 6. the device solves inside the learners ----
@pytest.mark.parametrize("idx", range(len(T.FIXTURES)))
def test_resident_learner_with_device_solves(mi, idx, monkeypatch):
    monkeypatch.setenv("MMIDX_PCA_LEARN_SOLVE", "device")
    c = plain_case(idx)
    p = resident_learn(mi, c.A, c.nc)
    assert np.array_equal(p.means, c.mu)
    checks_2_to_5(c, p, label=f"fixture {T.FIXTURES[idx]}, device solves:")
    p.close()


def test_rank_deficient_samples_with_device_solves(mi, monkeypatch):
    """nc = n: the centred matrix has rank n - 1; the block holds deficient directions, which are refilled"""
    monkeypatch.setenv("MMIDX_PCA_LEARN_SOLVE", "device")
    n, ss, nc = 12, 64, 12
    A = np.random.default_rng(9).standard_normal((n, ss))
    tol = 1e-10
    mu, sig, Vt_twin = T.twin(A)
    for p in (resident_learn(mi, A, nc, tol=tol), stream_learn(mi, A, nc, tol=tol)):
        assert np.array_equal(p.means, mu)
        assert np.all(np.abs(p.singularValues[:n - 1] / sig[:n - 1] - 1.0) <= 2 * tol * (sig[0] / sig[:n - 1]) ** 2 + 16 * EPS)  # check 4's bound
        assert p.singularValues[n - 1] <= 2 * np.sqrt(tol) * sig[0]  # a Ritz value within the residual (tol sv_1^2) of the eigenvalue 0
        assert T.ortho_defect(p.V_t[:n - 1]) <= 16 * T.ortho_defect(Vt_twin[:n - 1])  # check 3's bound
        p.close()


def test_not_converged_with_device_solves(mi, monkeypatch):
    monkeypatch.setenv("MMIDX_PCA_LEARN_SOLVE", "device")
    c = plain_case(1)
    p = mi.PCA(c.nc, c.n, c.ss, False)
    p.addSamples(c.A)
    with pytest.raises(mi.MmidxError) as ei:
        p.computeBasis(tol=TOL, max_iter=1)
    assert ei.value.status == 11 and "not converged" in str(ei.value) and f"{p.residual:.3e}" in str(ei.value)
    assert p.iterations == 1 and p.residual > TOL
    assert p.V_t is not None and np.all(np.isfinite(p.V_t))  # outputs still written
    p.close()


def test_default_selection_takes_the_device_path_above_256(mi, monkeypatch, capfd):
    """(1200, 640, 288): b = 320 > 256, so the streaming learner's default is the device solver (the trace line says which ran);
    the host solver on the same input agrees to the bounds"""
    c = made_case(1200, 640, 288, 0.99, 11)
    monkeypatch.delenv("MMIDX_PCA_LEARN_SOLVE", raising=False)
    monkeypatch.setenv("MMIDX_PCA_LEARN_TRACE", "1")
    capfd.readouterr()
    p = stream_learn(mi, c.A, c.nc, splits=[500])
    err = capfd.readouterr().err
    line = [ln for ln in err.splitlines() if "pca_stream: n 1200 ss 640 nc 288 b 320" in ln]
    assert len(line) == 1 and "solver device" in line[0], err[-2000:]
    print(line[0])
    assert np.array_equal(p.means, c.mu)
    checks_2_to_5(c, p, label="(1200, 640, 288), default = device solves:")
    monkeypatch.setenv("MMIDX_PCA_LEARN_SOLVE", "host")
    q = stream_learn(mi, c.A, c.nc, splits=[500])
    err = capfd.readouterr().err
    assert "solver host" in err and "solver device" not in err
    checks_2_to_5(c, q, label="(1200, 640, 288), host solves:")
    p.close()
    q.close()


# ---- 7. state errors on a live stream handle ----
def test_c_abi_state_errors(mi):
    import torch

    L = mi.lib()
    n, ss, nc = 96, 40, 5
    A = np.random.default_rng(3).standard_normal((n, ss))
    h = C.c_void_p()
    assert L.mmidx_pca_stream_create(nc, ss, 0, C.byref(h)) == 0
    means, sv, Vt = np.zeros(ss), np.zeros(nc), np.zeros((nc, ss))
    it, res, cnt = C.c_int32(0), C.c_double(0.0), C.c_int64(-1)
    args = (1e-12, 100, means.ctypes.data, sv.ctypes.data, Vt.ctypes.data, C.byref(it), C.byref(res))
    assert L.mmidx_pca_stream_count(h, C.byref(cnt)) == 0 and cnt.value == 0
    assert L.mmidx_pca_stream_add(h, 4, A.ctypes.data) == 0
    assert L.mmidx_pca_stream_compute(h, *args) == 6
    assert L.mmidx_last_error() == b"More data needed to compute the desired number of components"
    assert L.mmidx_pca_stream_add(h, 46, A[4:].ctypes.data) == 0  # (a refused compute finalises nothing)
    dA = torch.from_numpy(A[50:]).cuda()
    assert L.mmidx_pca_stream_add_device(h, 46, dA.data_ptr(), None) == 0
    assert L.mmidx_pca_stream_count(h, C.byref(cnt)) == 0 and cnt.value == n
    assert L.mmidx_pca_stream_compute(h, 1e-12, 1, *args[2:]) == 11  # not converged after one iteration ...
    assert L.mmidx_pca_stream_compute(h, *args) == 0                 # ... a second compute succeeds
    mu, sig, _ = T.twin(A)
    assert np.array_equal(means, mu)
    # check 4's bound with the tol this call passed (1e-12)
    assert np.all(np.abs(sv / sig[:nc] - 1.0) <= 2 * 1e-12 * (sig[0] / sig[:nc]) ** 2 + 16 * EPS) and T.sign_rule_holds(Vt)
    sv2, Vt2 = sv.copy(), Vt.copy()
    assert L.mmidx_pca_stream_compute(h, *args) == 0 and sv.tobytes() == sv2.tobytes() and Vt.tobytes() == Vt2.tobytes()
    assert L.mmidx_pca_stream_add(h, 1, A.ctypes.data) == 6 and b"finalised" in L.mmidx_last_error()
    assert L.mmidx_pca_stream_add_device(h, 1, dA.data_ptr(), None) == 6
    assert L.mmidx_pca_stream_count(h, C.byref(cnt)) == 0 and cnt.value == n
    assert L.mmidx_pca_stream_destroy(h) == 0
    # destroy with work in flight: rows handed over on a side stream, no wait before the handle goes
    h2 = C.c_void_p()
    assert L.mmidx_pca_stream_create(8, 2048, 0, C.byref(h2)) == 0
    side = torch.cuda.Stream()
    big = torch.ones((4096, 2048), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert L.mmidx_pca_stream_add_device(h2, 4096, big.data_ptr(), side.cuda_stream) == 0
    assert L.mmidx_pca_stream_destroy(h2) == 0
    torch.cuda.synchronize()
