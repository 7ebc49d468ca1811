"""numpy restatement of PCA.addSample / computeBasis (J/dimreduction/PCA.java:120-177) for the PCA-learning tests.

means: the reference's loop (:142-153) -- every column summed in arrival order into a zero-initialised double, one
division by n.  Components and singular values: np.linalg.svd of the centred matrix in fp64; LAPACK stands in for EJML's SVD
(absent from the reference tree, assumption A2) and is the reference quantity of every tolerance in the tests.
Not a test module (no test_ prefix); the fixtures are generated, never committed."""
import numpy as np

# (n, ss, nc, decay): sigma_i = decay^i, every sigma_i with i >= nc divided by 1.5 (a clear gap at the cut); the third has n < ss
FIXTURES = [(2048, 512, 64, 0.97), (1500, 1024, 128, 0.985), (300, 512, 32, 0.95), (4096, 256, 240, 0.99)]


def sequential_means(A):
    s = np.zeros(A.shape[1])
    for row in A:  # one elementwise addition per sample: per column the additions run in arrival order
        s = s + row
    return s / A.shape[0]


def make_fixture(n, ss, nc, decay, seed=0):
    """A = sqrt(n) U diag(s) V^T + c with U, V from QR of seeded Gaussians and c a constant row 0.05 N(0, I)"""
    rng = np.random.default_rng(1000 + seed)
    r = min(n, ss)
    U = np.linalg.qr(rng.standard_normal((n, r)))[0]
    V = np.linalg.qr(rng.standard_normal((ss, r)))[0]
    s = decay ** np.arange(r)
    s[nc:] /= 1.5
    c = 0.05 * rng.standard_normal(ss)
    return np.ascontiguousarray(np.sqrt(n) * (U * s) @ V.T + c)


def twin(A):
    """-> means [ss], sigma [min(n, ss)] descending, Vt [min(n, ss)][ss] (LAPACK's signs)"""
    mu = sequential_means(A)
    _, sig, Vt = np.linalg.svd(A - mu, full_matrices=False)
    return mu, sig, Vt


def ortho_defect(Vt):
    return float(np.max(np.abs(Vt @ Vt.T - np.eye(Vt.shape[0]))))


def sign_rule_holds(Vt):
    """in every row the entry of largest magnitude (lowest index on a tie: np.argmax returns the first) is positive"""
    j = np.argmax(np.abs(Vt), axis=1)
    return bool(np.all(Vt[np.arange(Vt.shape[0]), j] > 0.0))
