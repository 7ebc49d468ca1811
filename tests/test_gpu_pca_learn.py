"""GPU checks of the PCA learner (mmidx_pca_learn_*: k_pca_colsum, k_pca_gram, subspace iteration, k_pca_finish) against the
numpy twin (tests/pca_learn_twin.py): sequential means, then LAPACK's SVD of the centred matrix in fp64, which stands in for
EJML and is the reference quantity of every bound.  The Gram matrix and the twin are computed by numpy here, never taken from
the library.  tol = 1e-11 is the caller's request to computeBasis; every bound below is derived from it, from LAPACK's own
defect on the same fixture, or from eps -- none from what the library returns."""
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


@functools.lru_cache(maxsize=None)
def fixture_and_twin(idx):
    n, ss, nc, decay = T.FIXTURES[idx]
    A = T.make_fixture(n, ss, nc, decay, idx)
    mu, sig, Vt = T.twin(A)
    Ac = A - mu
    return A, mu, sig, Vt, Ac.T @ Ac


def learn(mi, A, nc, splits=None, tol=TOL, max_iter=200):
    n, ss = A.shape
    p = mi.PCA(nc, n, ss, False)
    lo = 0
    for hi in list(splits or []) + [n]:
        p.addSamples(A[lo:hi])
        lo = hi
    p.computeBasis(tol=tol, max_iter=max_iter)
    return p


def residual(G, Vt, sv):
    return float(np.max(np.linalg.norm(G @ Vt.T - Vt.T * sv ** 2, axis=0)))


@pytest.mark.parametrize("idx", range(len(T.FIXTURES)))
def test_learned_basis_against_the_twin(mi, idx):
    n, ss, nc, decay = T.FIXTURES[idx]
    A, mu, sig, Vt_twin, G = fixture_and_twin(idx)
    p = learn(mi, A, nc)
    q = learn(mi, A, nc, splits=[n // 7, n // 7 + 1 + n // 3])  # three uneven add calls
    print(f"fixture {T.FIXTURES[idx]}: iterations {p.iterations}, residual_out {p.residual:.3e}")
    # 1. means: the reference's sequential loop, bit for bit, however the samples arrived
    assert np.array_equal(p.means, mu) and np.array_equal(q.means, mu)
    # 6. determinism (a second learner, a second run: identical bytes) and the sign rule
    assert p.V_t.tobytes() == q.V_t.tobytes() and p.singularValues.tobytes() == q.singularValues.tobytes()
    assert T.sign_rule_holds(p.V_t)
    sv, Vt = p.singularValues, p.V_t
    assert np.all(np.diff(sv) <= 0.0)
    # 2. residual against numpy's Gram matrix: the caller's tol, a factor 2 for the device / numpy summation orders of G
    res = residual(G, Vt, sv)
    print(f"  residual {res / sv[0] ** 2:.3e} (bound {2 * TOL:.1e}) of sv_1^2")
    assert res <= 2 * TOL * sv[0] ** 2, (res / sv[0] ** 2, 2 * TOL)
    assert p.residual <= TOL
    # 3. orthonormality: at most 16 x LAPACK's own defect on this fixture
    d_lib, d_twin = T.ortho_defect(Vt), T.ortho_defect(Vt_twin[:nc])
    print(f"  orthogonality defect {d_lib:.3e}, twin {d_twin:.3e}")
    assert d_lib <= 16 * d_twin, f"defect {d_lib:.3e} > 16 x the twin's {d_twin:.3e}"
    # 4. singular values: a Ritz value lies within the residual norm of an eigenvalue
    err = np.abs(sv / sig[:nc] - 1.0)
    bound = 2 * TOL * (sig[0] / sig[:nc]) ** 2 + 16 * EPS
    print(f"  singular values: max relative error {err.max():.3e}, worst error / bound {np.max(err / bound):.3e}")
    assert np.all(err <= bound), (float(np.max(err / bound)))
    # 5. components up to sign (Davis-Kahan): gap_i = distance of sigma_i^2 to the nearest other eigenvalue, the (nc+1)-th included
    lam = sig ** 2
    lam_all = np.concatenate([lam, np.zeros(1)]) if lam.shape[0] < ss else lam  # (n < ss: the remaining eigenvalues of G are 0)
    gap = np.array([np.min(np.abs(np.delete(lam_all, i) - lam_all[i])) for i in range(nc)])
    miss = 1.0 - np.abs(np.sum(Vt * Vt_twin[:nc], axis=1))
    bound = 0.5 * (2 * TOL * lam[0] / gap) ** 2 + 16 * EPS
    print(f"  components: max 1 - |<v, v_twin>| {miss.max():.3e}, worst / bound {np.max(miss / bound):.3e}")
    assert np.all(miss <= bound), (float(np.max(miss / bound)))


def test_cfg5_shape(mi):
    """(16384, 8192, 128), 1 GiB of samples: checks 1-3 and 6; G from one numpy matmul, no LAPACK solve at this size.
    Rank-256 signal with a geometric spectrum (halved from the 129th on: sigma_nc / sigma_nc+1 ~ 2 >= 1.5) + 1e-3 noise."""
    n, ss, nc, r = 16384, 8192, 128, 256
    rng = np.random.default_rng(55)
    U = np.linalg.qr(rng.standard_normal((n, r)))[0]
    V = np.linalg.qr(rng.standard_normal((ss, r)))[0]
    s = 0.97 ** np.arange(r)
    s[nc:] /= 2.0
    A = np.sqrt(n) * (U * s) @ V.T
    A += 1e-3 * rng.standard_normal((n, ss))
    A += 0.05 * rng.standard_normal(ss)
    del U
    mu = T.sequential_means(A)
    p = learn(mi, A, nc)
    print(f"cfg5 shape: iterations {p.iterations}, residual_out {p.residual:.3e}")
    assert np.array_equal(p.means, mu)
    assert T.sign_rule_holds(p.V_t) and np.all(np.diff(p.singularValues) <= 0.0)
    q = learn(mi, A, nc, splits=[1000, 9001])
    assert np.array_equal(q.means, mu)
    assert p.V_t.tobytes() == q.V_t.tobytes() and p.singularValues.tobytes() == q.singularValues.tobytes()
    sv, Vt = p.singularValues.copy(), p.V_t.copy()
    p.close()
    q.close()
    A -= mu
    G = A.T @ A
    del A
    res = residual(G, Vt, sv)
    print(f"  residual {res / sv[0] ** 2:.3e} (bound {2 * TOL:.1e}) of sv_1^2")
    assert res <= 2 * TOL * sv[0] ** 2, (res / sv[0] ** 2, 2 * TOL)
    assert p.residual <= TOL
    d_twin = max(T.ortho_defect(fixture_and_twin(i)[3][:T.FIXTURES[i][2]]) for i in range(len(T.FIXTURES)))
    d_lib = T.ortho_defect(Vt)
    print(f"  orthogonality defect {d_lib:.3e}, largest twin defect of the small fixtures {d_twin:.3e}")
    assert d_lib <= 16 * d_twin, f"defect {d_lib:.3e} > 16 x {d_twin:.3e}"


def test_not_converged_is_reported(mi):
    """max_iter = 1 on fixture 2: the failure path is an error with the residual, not a silent result"""
    n, ss, nc, decay = T.FIXTURES[1]
    A = fixture_and_twin(1)[0]
    p = mi.PCA(nc, n, ss, False)
    p.addSamples(A)
    with pytest.raises(mi.MmidxError) as ei:
        p.computeBasis(tol=TOL, max_iter=1)
    assert ei.value.status == 11 and "not converged" in str(ei.value) and "residual" in str(ei.value)
    assert p.iterations == 1 and p.residual > TOL
    assert f"{p.residual:.3e}" in str(ei.value)
    assert p.V_t is not None and np.all(np.isfinite(p.V_t))  # outputs still written
    p.computeBasis(tol=TOL, max_iter=200)  # the samples are still resident: the same learner converges when allowed to
    assert p.residual <= TOL and p.iterations > 1


def test_c_abi_state_errors_and_device_rows(mi):
    """the reference's messages through the C ABI on a live learner, and mmidx_pca_learn_add_device"""
    import torch

    L = mi.lib()
    n, ss, nc = 96, 40, 5
    A = np.random.default_rng(3).standard_normal((n, ss))
    h = C.c_void_p()
    assert L.mmidx_pca_learn_create(nc, n, ss, 0, C.byref(h)) == 0
    means, sv, Vt = np.zeros(ss), np.zeros(nc), np.zeros((nc, ss))
    it, res = C.c_int32(0), C.c_double(0.0)
    args = (1e-12, 100, means.ctypes.data, sv.ctypes.data, Vt.ctypes.data, C.byref(it), C.byref(res))
    assert L.mmidx_pca_learn_add(h, 50, A.ctypes.data) == 0
    assert L.mmidx_pca_learn_compute(h, *args) == 6 and L.mmidx_last_error() == b"Not all the data has been added"
    assert L.mmidx_pca_learn_add(h, 47, A.ctypes.data) == 6 and L.mmidx_last_error() == b"Too many samples"
    dA = torch.from_numpy(A[50:]).cuda()
    assert L.mmidx_pca_learn_add_device(h, 46, dA.data_ptr(), None) == 0
    assert L.mmidx_pca_learn_add_device(h, 1, dA.data_ptr(), None) == 6 and L.mmidx_last_error() == b"Too many samples"
    assert L.mmidx_pca_learn_compute(h, *args) == 0
    mu, sig, Vt_twin = T.twin(A)
    assert np.array_equal(means, mu)
    # check 4's bound with the tol this call passed (1e-12)
    assert np.all(np.abs(sv / sig[:nc] - 1.0) <= 2 * 1e-12 * (sig[0] / sig[:nc]) ** 2 + 16 * EPS) and T.sign_rule_holds(Vt)
    assert L.mmidx_pca_learn_destroy(h) == 0
    h2 = C.c_void_p()
    assert L.mmidx_pca_learn_create(8, 4, 16, 0, C.byref(h2)) == 0
    assert L.mmidx_pca_learn_add(h2, 4, A.ctypes.data) == 0
    assert L.mmidx_pca_learn_compute(h2, *args) == 6
    assert L.mmidx_last_error() == b"More data needed to compute the desired number of components"
    assert L.mmidx_pca_learn_destroy(h2) == 0


def test_rank_deficient_samples(mi):
    """nc = n: the centred matrix has rank n - 1, the last singular value is 0 and its block directions are deficient"""
    n, ss, nc = 12, 64, 12
    A = np.random.default_rng(9).standard_normal((n, ss))
    tol = 1e-10
    p = learn(mi, A, nc, tol=tol)
    mu, sig, Vt_twin = T.twin(A)
    assert np.array_equal(p.means, mu)
    assert np.all(np.abs(p.singularValues[:n - 1] / sig[:n - 1] - 1.0) <= 2 * tol * (sig[0] / sig[:n - 1]) ** 2 + 16 * EPS)  # check 4's bound
    assert p.singularValues[n - 1] <= 2 * np.sqrt(tol) * sig[0]  # a Ritz value within the residual (tol sv_1^2) of the eigenvalue 0
    assert T.ortho_defect(p.V_t[:n - 1]) <= 16 * T.ortho_defect(Vt_twin[:n - 1])  # check 3's bound


def test_learn_save_load_project_end_to_end(mi, oracle, tmp_path):
    """VLAD vectors of synthetic images -> learn -> savePCAToFile -> a fresh PCA loads the file -> the existing projection"""
    rng = np.random.default_rng(21)
    dl, ncent, nimg, nc = 16, 16, 600, 32
    cb = rng.standard_normal((ncent, dl))
    M = rng.standard_normal((12, dl))
    sets = []
    for _ in range(nimg):
        k = int(rng.integers(30, 70))
        sets.append(cb[rng.integers(0, ncent, k)] + 0.4 * (rng.standard_normal(12) @ M) + 0.15 * rng.standard_normal((k, dl)))
    agg = mi.VladAggregatorMultipleVocabularies([cb])
    X = agg.aggregate_batch(sets)
    agg.close()
    ss = X.shape[1]
    p = mi.PCA(nc, nimg, ss, False)
    for x in X[:3]:
        p.addSample(x)
    p.addSamples(X[3:])
    p.computeBasis(tol=TOL, max_iter=2000)
    print(f"end to end: ss {ss}, iterations {p.iterations}, residual_out {p.residual:.3e}")
    path = str(tmp_path / "pca_learned.txt")
    p.savePCAToFile(path)
    sv, Vt, mu = p.singularValues, p.V_t, p.means
    assert np.array_equal(mu, T.sequential_means(X))
    plain = mi.PCA(nc, 1, ss, False)
    plain.loadPCAFromFile(path)
    with pytest.raises(mi.MmidxError):
        plain.savePCAToFile(path)
    Y = plain.project(X)
    # the Gram matrix of the projections is diag(sv^2) within check 2's bound
    dev = float(np.max(np.abs(Y.T @ Y - np.diag(sv ** 2))))
    print(f"  |Y^T Y - diag(sv^2)| {dev / sv[0] ** 2:.3e} (bound {2 * TOL:.1e}) of sv_1^2")
    assert dev <= 2 * TOL * sv[0] ** 2, (dev / sv[0] ** 2, 2 * TOL)
    # with whitening: test_pca_projection_mfma's tolerance against the oracle, for the learned basis
    white = mi.PCA(nc, 1, ss, True)
    white.loadPCAFromFile(path)
    Yw = white.project(X[:60])
    Vw = oracle.pca_whiten(Vt, sv)
    for i in range(60):
        ref = oracle.pca_project(Vw, mu, X[i], True)
        scale = max(1.0, float(np.linalg.norm(ref)))
        assert np.max(np.abs(Yw[i] - ref)) <= 1e-12 * scale, (i, np.max(np.abs(Yw[i] - ref)))
    for o in (p, plain, white):
        o.close()
