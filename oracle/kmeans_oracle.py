"""CPU restatement of the clustering behind the reference's codebook learners -- TEST INFRASTRUCTURE (only tests/ import it).

PARITY UNPINNED.  The reference learns its coarse and product quantizers with Weka's SimpleKMeans:
    J/quantization/AbstractQuantizerLearning.java:39-81   learnAndWriteQuantizer: new SimpleKMeans(), optional
        setInitializationMethod(KMEANS_PLUS_PLUS) (:53-56), setSeed(seed) (:58), setNumClusters (:59),
        setMaxIterations (:60), setFastDistanceCalc(true) (:62), buildClusterer(data) (:64), centroids written one per
        line, comma separated (:73-80)
    J/quantization/CoarseQuantizerLearning.java:39-72, ProductQuantizationLearning.java:247-305   the callers
Weka (weka-dev 3.7.x, pom.xml) is a third-party dependency that is absent from /root/reference and from this image, and the
reference ships no test or fixture for the learners, so nothing pins this file to Weka's output.

What IS Weka's, restated from its published algorithm (SimpleKMeans.buildClusterer):
    * default seeding: walk j = n-1 .. 0, pick instIndex = Random(seed).nextInt(j + 1), take the instance as a centre if
      no equal centre exists yet, swap it to position j, stop at k centres                          -> random_seeding()
    * k-means++ seeding: first centre = instance Random(seed).nextInt(n), every next centre drawn with probability
      proportional to the squared distance to the nearest centre so far (cumulative sum, nextDouble)   -> plus_plus_seeding()
    * distance = EuclideanDistance with attribute normalisation to [0, 1] (min-max over the data) by default
    * Lloyd iterations until no instance changes cluster or maxIterations; empty clusters are dropped -> lloyd()
    * java.util.Random: the JDK's documented 48-bit LCG                                              -> JavaRandom
What is NOT Weka's and is this build's own choice (libmmidx_hip's kernels make the same one, which is what the GPU tests
compare bit for bit): the nearest centre is the exact sequential fp64 squared distance with the FIRST index winning ties, a
centroid is the sum of its members in ascending index order divided by their number, and after an iteration that dropped a
cluster every instance counts as "changed".  Weka's own summation order and tie rule are not known here.
"""
import numpy as np


class JavaRandom:
    """java.util.Random (JDK javadoc): seed scrambling, next(bits), nextInt(bound), nextDouble()"""

    def __init__(self, seed):
        self.s = (seed ^ 0x5DEECE66D) & ((1 << 48) - 1)

    def next(self, bits):
        self.s = (self.s * 0x5DEECE66D + 0xB) & ((1 << 48) - 1)
        v = self.s >> (48 - bits)
        return v - (1 << bits) if v >= (1 << (bits - 1)) and bits == 32 else v

    def nextInt(self, bound):
        r = self.next(31)
        m = bound - 1
        if bound & m == 0:
            return (bound * r) >> 31
        u = r
        while True:
            r = u % bound
            if u - r + m < (1 << 31):
                return r
            u = self.next(31)

    def nextDouble(self):
        return ((self.next(26) << 27) + self.next(27)) * 2.0 ** -53


def seq_sqdist(x, c):
    """sequential fp64 squared distance, dimension ascending"""
    acc = 0.0
    for a, b in zip(x, c):
        df = a - b
        acc += df * df
    return acc


def random_seeding(X, k, seed):
    """SimpleKMeans' default initialisation (indices of the picked instances): an instance equal to a centre already
    picked is skipped, the swap and the walk go on; fewer than k picks when X has fewer than k distinct rows"""
    r = JavaRandom(seed)
    perm, picks = list(range(len(X))), []
    for j in range(len(X) - 1, -1, -1):
        i = r.nextInt(j + 1)
        if not any(np.array_equal(X[perm[i]], X[p]) for p in picks):
            picks.append(perm[i])
        perm[j], perm[i] = perm[i], perm[j]
        if len(picks) == k:
            break
    return picks


def plus_plus_seeding(X, k, seed, margin=1e-9):
    """k-means++ initialisation; raises when a draw lands within `margin` (relative) of a bucket edge, where the order of a
    parallel prefix sum could pick the neighbouring instance"""
    r = JavaRandom(seed)
    picks = [r.nextInt(len(X))]
    d2 = None
    for _ in range(1, k):
        nd = np.array([seq_sqdist(x, X[picks[-1]]) for x in X])
        d2 = nd if d2 is None else np.minimum(d2, nd)
        cum = np.cumsum(d2)
        target = r.nextDouble() * cum[-1]
        idx = int(np.searchsorted(cum, target, side="right"))
        if abs(cum[min(idx, len(X) - 1)] - target) <= margin * cum[-1]:
            raise ValueError("fixture too close to a bucket edge")
        picks.append(min(idx, len(X) - 1))
    return picks


def lloyd(X, C0, max_iter):
    """Lloyd iterations: sequential fp64 distances, first index wins, index-ordered sums, empty clusters dropped.
    Returns (centroids, assignment into them, iterations)"""
    C = np.array(C0, dtype=np.float64).copy()
    a_old = np.full(len(X), -1)
    iters = 0
    while True:
        iters += 1
        a = np.array([int(np.argmin([seq_sqdist(x, c) for c in C])) for x in X])
        changed = int((a != a_old).sum())
        newC, keep = [], []
        for c in range(len(C)):
            mem = np.nonzero(a == c)[0]
            if len(mem):
                acc = np.zeros(X.shape[1])
                for i in mem:
                    acc = acc + X[i]
                newC.append(acc / float(len(mem)))
                keep.append(c)
        done = changed == 0 or iters >= max_iter
        dropped = len(keep) != len(C)
        remap = {c: t for t, c in enumerate(keep)}
        C = np.array(newC)
        if done:
            return C, np.array([remap[c] for c in a]), iters
        a_old = np.full(len(X), -1) if dropped else a


def minmax_normalise(X, ref=None):
    """EuclideanDistance's default attribute normalisation (the clustering then runs in this space): (x - min) / (max - min),
    0 for a constant attribute (NormalizableDistance.norm).  ref: the data whose min / max are used (default X itself)"""
    X = np.asarray(X, np.float64)
    R = X if ref is None else np.asarray(ref, np.float64)
    mn, mx = R.min(0), R.max(0)
    r = mx - mn
    return np.divide(X - mn, r, out=np.zeros_like(X), where=r > 0.0)


# ---- vectorised twins ---------------------------------------------------------------------------------------------------
# The same fp64 operations in the same order as the loop versions above (which stay the specification), with numpy doing
# the loops: bit-identical results at the shapes the GPU learner runs at.  numpy never contracts a * b + c to an FMA, and
# every sum below is an explicit sequential accumulation (no np.sum / reduceat, whose order is pairwise).

_CHUNK_ELEMS = 1 << 22  # (n_chunk, k) distance block: 32 MB of fp64


def sqdist_np(X, C):
    """yields (i0, D) with D[i, c] = seq_sqdist(X[i0 + i], C[c]) for row chunks of X: dimension ascending, one fp64 add each"""
    X, C = np.asarray(X, np.float64), np.asarray(C, np.float64)
    n, d = X.shape
    step = max(1, _CHUNK_ELEMS // max(1, len(C)))
    for i0 in range(0, n, step):
        xb = X[i0:i0 + step]
        acc = np.zeros((len(xb), len(C)))
        for j in range(d):
            df = xb[:, j:j + 1] - C[None, :, j]
            acc += df * df
        yield i0, acc


def nearest_np(X, C):
    """index of the nearest centre, first index wins ties (np.argmin)"""
    out = np.empty(len(X), np.int64)
    for i0, D in sqdist_np(X, C):
        out[i0:i0 + len(D)] = np.argmin(D, 1)
    return out


def point_sqerr_np(X, C, a):
    """|x_i - C[a_i]|^2 per point, dimension ascending"""
    X, C = np.asarray(X, np.float64), np.asarray(C, np.float64)
    acc = np.zeros(len(X))
    for j in range(X.shape[1]):
        df = X[:, j] - C[a, j]
        acc += df * df
    return acc


def seq_total(v):
    """v[0] + v[1] + ... in index order (np.add.accumulate is sequential)"""
    v = np.asarray(v, np.float64)
    return float(np.add.accumulate(v)[-1]) if len(v) else 0.0


def cluster_sums_np(X, a, k):
    """(sums [k][d], counts [k]): the members of every cluster added up in ascending index order, starting from 0.0 --
    one step per member rank r (the r-th member of every cluster that has one), not one per cluster"""
    X = np.asarray(X, np.float64)
    a = np.asarray(a, np.int64)
    counts = np.bincount(a, minlength=k)
    order = np.argsort(a, kind="stable")  # grouped by cluster, ascending index inside a cluster
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    by_size = np.argsort(-counts, kind="stable")  # clusters with more than r members form a prefix of by_size
    sizes = counts[by_size]
    acc = np.zeros((k, X.shape[1]))
    for r in range(int(counts.max()) if k else 0):
        cl = by_size[:int(np.searchsorted(-sizes, -r, side="left"))]
        acc[cl] = acc[cl] + X[order[starts[cl] + r]]
    return acc, counts


def lloyd_np(X, C0, max_iter):
    """lloyd() vectorised (same results bit for bit)"""
    X = np.asarray(X, np.float64)
    C = np.array(C0, dtype=np.float64).copy()
    a_old = np.full(len(X), -1)
    iters = 0
    while True:
        iters += 1
        a = nearest_np(X, C)
        changed = int((a != a_old).sum())
        sums, counts = cluster_sums_np(X, a, len(C))
        keep = np.nonzero(counts)[0]
        newC = sums[keep] / counts[keep].astype(np.float64)[:, None]
        done = changed == 0 or iters >= max_iter
        dropped = len(keep) != len(C)
        remap = np.full(len(C), -1)
        remap[keep] = np.arange(len(keep))
        C = newC
        if done:
            return C, remap[a], iters
        a_old = np.full(len(X), -1) if dropped else a


def random_seeding_np(X, k, seed):
    """random_seeding() with a hash set of the picked rows in place of the pairwise comparison (same picks)"""
    X = np.asarray(X, np.float64)
    r = JavaRandom(seed)
    n = len(X)
    perm, picks, seen = np.arange(n), [], set()
    for j in range(n - 1, -1, -1):
        i = r.nextInt(j + 1)
        key = tuple(X[perm[i]].tolist())  # (float ==: -0.0 and 0.0 are one key, as with np.array_equal)
        if key not in seen:
            seen.add(key)
            picks.append(int(perm[i]))
        perm[j], perm[i] = perm[i], perm[j]
        if len(picks) == k:
            break
    return picks


def plus_plus_seeding_np(X, k, seed, margin=1e-9):
    """plus_plus_seeding() vectorised (same picks, same bucket-edge check)"""
    X = np.asarray(X, np.float64)
    n = len(X)
    r = JavaRandom(seed)
    picks = [r.nextInt(n)]
    d2 = None
    for _ in range(1, k):
        nd = point_sqerr_np(X, X[picks[-1]][None, :], np.zeros(n, np.int64))
        d2 = nd if d2 is None else np.minimum(d2, nd)
        cum = np.cumsum(d2)
        target = r.nextDouble() * cum[-1]
        idx = int(np.searchsorted(cum, target, side="right"))
        if abs(cum[min(idx, n - 1)] - target) <= margin * cum[-1]:
            raise ValueError("fixture too close to a bucket edge")
        picks.append(min(idx, n - 1))
    return picks


def kmeans_np(X, k, max_iter, seed=1, plus_plus=False, normalize=True, init=None):
    """the whole of mmidx_kmeans restated: (centroids [k_eff][d], assignment, squared error, iterations).
    normalize: the clustering runs on minmax_normalise(X) (given centres normalised with the data's min / max), the squared
    error is measured there, and the centroids reported are the means of the ORIGINAL members of the final clusters.
    Default seeding compares original rows; k-means++ draws in the space the clustering runs in."""
    X = np.asarray(X, np.float64)
    W = minmax_normalise(X) if normalize else X
    if init is not None:
        C0 = minmax_normalise(init, ref=X) if normalize else np.asarray(init, np.float64)
    elif plus_plus:
        C0 = W[plus_plus_seeding_np(W, k, seed)]
    else:
        C0 = W[random_seeding_np(X, k, seed)]
    C, a, iters = lloyd_np(W, C0, max_iter)
    sse = seq_total(point_sqerr_np(W, C, a))
    if normalize:
        sums, counts = cluster_sums_np(X, a, len(C))
        C = sums / counts.astype(np.float64)[:, None]
    return C, a, sse, iters
