"""The vectorised k-means twin (oracle/kmeans_oracle.py: *_np) against the loop restatement it speeds up -- CPU only.

The GPU learning tests compare libmmidx_hip's k-means with the vectorised twin at codebook shapes, where the loop version
(pure Python over every point, centre and dimension) would take hours.  These fixtures pin the two twins to each other bit
for bit on small inputs built to reach the awkward paths: exact ties, duplicate rows, seeds that repeat a row, clusters that
empty in the middle of a run or on its last iteration, a constant attribute under normalisation."""
import numpy as np
import pytest

from oracle import kmeans_oracle as ko


def _lattice(n, d, levels, seed):
    """small-integer rows: squared distances are integers, so exact ties between centres are everywhere"""
    return np.random.default_rng(seed).integers(0, levels, (n, d)).astype(np.float64)


def _same(a, b):
    return np.array_equal(a, b) and a.shape == b.shape


@pytest.mark.parametrize("case", ["gauss", "lattice", "dups", "far"])
def test_lloyd_np_is_lloyd(case):
    rng = np.random.default_rng({"gauss": 1, "lattice": 2, "dups": 3, "far": 4}[case])
    if case == "gauss":
        X = rng.standard_normal((240, 5)) * [1.0, 3.0, 0.5, 10.0, 1e-3]
        C0 = X[rng.choice(len(X), 9, replace=False)]
    elif case == "lattice":  # ties in every iteration's first assignment; first index must win
        X = _lattice(200, 4, 3, 1)
        C0 = X[[0, 5, 9, 14, 33, 70, 71]]
    elif case == "dups":  # duplicated initial centres: the later copy loses every tie, empties and is dropped mid-run
        X = rng.standard_normal((180, 3))
        C0 = np.concatenate([X[:6], X[[1, 4]]])
    else:  # centres nobody is near: dropped on iteration 1
        X = rng.standard_normal((150, 2))
        C0 = np.array([[0.0, 0.0], [1.0, 1.0], [1e3, 1e3], [-1.0, 0.5], [-500.0, 7.0]])
    for it in (1, 2, 30):
        lC, lA, lI = ko.lloyd(X, C0, it)
        vC, vA, vI = ko.lloyd_np(X, C0, it)
        assert lI == vI and _same(lC, vC) and np.array_equal(lA, vA), (case, it)
    if case in ("dups", "far"):
        assert len(ko.lloyd_np(X, C0, 1)[0]) < len(C0)  # (the fixture really drops clusters)


def test_cluster_sums_are_index_ordered():
    """the sums are the sequential ones: a fixture where the pairwise / reversed order rounds differently"""
    X = np.array([[1.0], [1e16], [1.0], [-1e16], [1.0], [3.0]])
    a = np.array([0, 0, 0, 0, 1, 1])
    s, c = ko.cluster_sums_np(X, a, 2)
    seq = 0.0
    for v in X[:4, 0]:
        seq += v
    assert s[0, 0] == seq == 0.0 + 1.0 + 1e16 + 1.0 + -1e16  # ((1 + 1e16) + 1) - 1e16 = 0 in fp64; reversed gives 1
    assert s[1, 0] == 4.0 and list(c) == [4, 2]


def test_sqdist_np_is_seq_sqdist():
    rng = np.random.default_rng(2)
    X, C = rng.standard_normal((70, 13)) * 1e3, rng.standard_normal((11, 13))
    D = np.concatenate([blk for _, blk in ko.sqdist_np(X, C)])
    assert all(D[i, c] == ko.seq_sqdist(X[i], C[c]) for i in range(len(X)) for c in range(len(C)))
    assert np.array_equal(ko.nearest_np(X, C), [int(np.argmin([ko.seq_sqdist(x, c) for c in C])) for x in X])
    a = ko.nearest_np(X, C)
    assert np.array_equal(ko.point_sqerr_np(X, C, a), [ko.seq_sqdist(x, C[j]) for x, j in zip(X, a)])


@pytest.mark.parametrize("seed", [1, 2, 7])
def test_random_seeding_np_is_random_seeding(seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((120, 3))
    X[60:] = X[rng.integers(0, 10, 60)]  # half the rows repeat one of ten
    for k in (1, 5, 20, 70):
        assert ko.random_seeding(X, k, seed) == ko.random_seeding_np(X, k, seed)


def test_random_seeding_skips_rows_equal_to_a_centre():
    """SimpleKMeans' rule: a drawn instance equal to a centre already chosen is not taken (the swap still happens)"""
    X = np.repeat(np.arange(6, dtype=np.float64)[:, None], 5, 0)  # 30 rows, 6 distinct values
    picks = ko.random_seeding_np(X, 4, 3)
    assert len(picks) == 4 and len({X[p, 0] for p in picks}) == 4
    picks = ko.random_seeding_np(X, 10, 3)  # fewer distinct rows than k: seeding ends short
    assert len(picks) == 6 and len({X[p, 0] for p in picks}) == 6
    assert picks == ko.random_seeding(X, 10, 3)
    # the walk is the plain one when all rows differ: the first draws are nextInt(n), nextInt(n - 1), ... with swaps
    Y = np.arange(40, dtype=np.float64)[:, None]
    r, perm, want = ko.JavaRandom(5), list(range(40)), []
    for j in range(39, 31, -1):
        i = r.nextInt(j + 1)
        want.append(perm[i])
        perm[j], perm[i] = perm[i], perm[j]
    assert ko.random_seeding_np(Y, 8, 5) == want


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_plus_plus_np_is_plus_plus(seed):
    rng = np.random.default_rng(10 + seed)
    X = rng.standard_normal((150, 4)) * [1.0, 2.0, 1e-2, 5.0]
    try:
        want = ko.plus_plus_seeding(X, 9, seed)
    except ValueError:
        with pytest.raises(ValueError):
            ko.plus_plus_seeding_np(X, 9, seed)
        return
    assert ko.plus_plus_seeding_np(X, 9, seed) == want


def test_minmax_constant_column_is_zero():
    """a constant attribute normalises to 0 (NormalizableDistance.norm, k_normalize), not NaN"""
    X = np.array([[1.0, 5.0, -2.0], [3.0, 5.0, 0.0], [2.0, 5.0, 2.0]])
    Y = ko.minmax_normalise(X)
    assert np.all(np.isfinite(Y)) and np.all(Y[:, 1] == 0.0)
    assert np.array_equal(Y[:, 0], [0.0, 1.0, 0.5]) and np.array_equal(Y[:, 2], [0.0, 0.5, 1.0])
    # given centres are normalised with the data's min / max, constant attribute -> 0 as well
    assert np.array_equal(ko.minmax_normalise(np.array([[5.0, 9.0, 4.0]]), ref=X), [[2.0, 0.0, 1.5]])


def _kmeans_loop(X, k, max_iter, seed=1, plus_plus=False, normalize=True, init=None):
    """kmeans_np assembled from the loop versions only"""
    X = np.asarray(X, np.float64)
    W = ko.minmax_normalise(X) if normalize else X
    if init is not None:
        C0 = ko.minmax_normalise(init, ref=X) if normalize else init
    elif plus_plus:
        C0 = W[ko.plus_plus_seeding(W, k, seed)]
    else:
        C0 = W[ko.random_seeding(X, k, seed)]
    C, a, iters = ko.lloyd(W, C0, max_iter)
    sse = 0.0
    for x, j in zip(W, a):
        sse += ko.seq_sqdist(x, C[j])
    if normalize:
        C = np.array([_mean_in_order(X[a == c]) for c in range(len(C))])
    return C, a, sse, iters


def _mean_in_order(rows):
    acc = np.zeros(rows.shape[1])
    for r in rows:
        acc = acc + r
    return acc / float(len(rows))


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("mode", ["default", "plus_plus", "init_far"])
def test_kmeans_np_is_the_loop_assembly(mode, normalize):
    rng = np.random.default_rng(21)
    X = rng.standard_normal((160, 4)) * [1.0, 100.0, 0.01, 1.0]
    X[:, 3] = 2.5  # a constant attribute
    X[100:130] = X[:30]  # repeated rows (duplicate seeds for the default seeding)
    kw = dict(seed=2, normalize=normalize)
    if mode == "plus_plus":
        kw["plus_plus"] = True
    if mode == "init_far":  # a far centre, maxIterations = 1: dropped on the final iteration (remap, then the final means)
        kw["init"] = np.concatenate([X[:5], [[1e3, 1e3, 1e3, 2.5]]])
    for it in (1, 4):
        want = _kmeans_loop(X, 6, it, **kw)  # (seed 2's k-means++ draws sit clear of every bucket edge here)
        got = ko.kmeans_np(X, 6, it, **kw)
        assert got[3] == want[3] and got[2] == want[2]
        assert _same(got[0], want[0]) and np.array_equal(got[1], want[1])
        if mode == "init_far":
            assert len(got[0]) == 5
