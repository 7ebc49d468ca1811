"""Shapes and data shared by the id-query tests (tests/test_id_queries_cpu.py, tests/test_gpu_id_queries.py): clustered base
vectors around loose centroids and codebooks from two k-means rounds on residuals, as tests/test_gpu_passa_q.py builds them."""
import numpy as np

import synth

KIND_PQ, KIND_IVFPQ = 1, 2
TR_NONE, TR_ROTATION, TR_PERMUTATION = 0, 1, 2

# (name, kind, D, C, m, ks, n, k, transform, seed): a seed under which the ids the CPU test draws meet no tie in their top k + 1
# (at 500 records and 16-entry codebooks two records can share (list, code): seed 11 gives none)
TABLE = [
    ("d16", KIND_IVFPQ, 16, 4, 4, 16, 500, 3, TR_NONE, 11),
    ("d32_perm", KIND_IVFPQ, 32, 8, 8, 256, 3000, 10, TR_PERMUTATION, 12),
    ("d128", KIND_IVFPQ, 128, 6, 16, 256, 6000, 100, TR_NONE, 13),
    ("d128_rot", KIND_IVFPQ, 128, 6, 16, 256, 6000, 100, TR_ROTATION, 14),
    ("d64_short", KIND_IVFPQ, 64, 5, 8, 512, 4000, 20, TR_NONE, 15),
]
# the GPU suite adds: D not a power of two; D above any block size (the K3mk shape); flat PQ without and with a rotation
EXTRA = [
    ("d24_perm", KIND_IVFPQ, 24, 3, 6, 64, 2000, 10, TR_PERMUTATION, 16),
    ("d1024_rot", KIND_IVFPQ, 1024, 4, 64, 256, 1500, 10, TR_ROTATION, 17),
    ("pq32", KIND_PQ, 32, 0, 8, 256, 3000, 10, TR_NONE, 18),
    ("pq32_rot", KIND_PQ, 32, 0, 8, 256, 3000, 10, TR_ROTATION, 19),
]


def problem(seed, kind, D, C, m, ks, n, transform, dup=1):
    """dict(coarse [C][D] or None, base [n][D], pq [m][ks][dsub], rot [D][D] or None).  The permutation is the library's own
    (java.util.Random seed 1): the caller asks the oracle for it."""
    rng = np.random.default_rng(seed)
    ds = D // m
    ntrain = min(n // dup, 3000)
    if kind == KIND_IVFPQ:
        mu = 0.5 * rng.standard_normal((C, D))
        base = mu[rng.integers(0, C, n // dup)] + rng.standard_normal((n // dup, D))
        train = mu[rng.integers(0, C, ntrain)] - base[:ntrain]
    else:
        mu = None
        base = rng.standard_normal((n // dup, D))
        train = base[:ntrain]
    base = np.concatenate([base] * dup)[rng.permutation((n // dup) * dup)]
    pq = np.stack([synth.kmeans(train[:, s * ds:(s + 1) * ds], ks, iters=2, seed=s) for s in range(m)])
    rot = np.linalg.qr(rng.standard_normal((D, D)))[0] if transform == TR_ROTATION else None
    return dict(coarse=mu, base=base, pq=pq, rot=rot)


def oracle_index(o, p, kind, D, C, m, ks, transform, w=None):
    """the CPU oracle over the problem's quantizers, empty"""
    perm = o.random_permutation(1, D) if transform == TR_PERMUTATION else None
    ref = o.OracleIndex(kind, D, m, ks, C, transform=transform, perm=perm, rot=p["rot"])
    if kind == KIND_IVFPQ:
        ref.set_coarse(p["coarse"])
        ref.set_w(C if w is None else w)
    ref.set_pq(p["pq"])
    return ref, perm
