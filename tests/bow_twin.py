"""Restatement of BowAggregator.aggregateInternal (J/aggregation/BowAggregator.java:39-74) from what the oracle exports.

  k == 1   bow[computeNearestCentroid(d)]++                       -> oracle.nearest_centroid (AFA:136-155, strict `<`)
  k  > 1   nn = computeKNearestCentroids(d, k) (AFA:193-220), and for each of the k indices bow[nn[j]]++ runs
           descriptorLength times (the inner loop :47-51, sic)    -> an OracleIndex whose coarse quantizer is the vocabulary and
           nearest_coarse(d, k): IVFPQ.computeNearestCoarseIndices (IVFPQ.java:575-601) is that loop line for line, bounded queue
           (oracle.set_queue_rule) included.
The output is raw: no normalisation, getVectorLength() == numCentroids."""
import numpy as np


class BowTwin:
    def __init__(self, oracle, codebook, k=1):
        self.o = oracle
        self.cb = np.ascontiguousarray(codebook, np.float64)
        self.nc, self.dl = self.cb.shape
        self.k = int(k)
        if self.k < 1 or self.k > self.nc:
            raise ValueError("k outside 1..numCentroids")  # LingPipe queue constructor / poll() == null
        self.ix = None
        if self.k > 1:
            # (m = 1, ks = 2: the smallest product quantizer the constructor takes; it is never set and never used)
            self.ix = oracle.OracleIndex(oracle.KIND_IVFPQ, self.dl, 1, 2, self.nc)
            self.ix.set_coarse(self.cb)

    def aggregate(self, descriptors):
        bow = np.zeros(self.nc, np.float64)
        if descriptors is None or len(descriptors) == 0:
            return bow
        descs = np.ascontiguousarray(descriptors, np.float64)
        if descs.ndim != 2 or descs.shape[1] != self.dl:
            raise ValueError("Descriptor length is incompatible with codebook centroid length!")  # AFA:72-79
        for d in descs:
            if self.k == 1:
                bow[self.o.nearest_centroid(self.cb, d)] += 1.0
            else:
                for c in self.ix.nearest_coarse(d, self.k):
                    # BowAggregator.java:47-51: bow[c]++ descriptorLength times.  On an integer-valued double far below 2^53 that
                    # is one exact addition of descriptorLength.
                    bow[c] += float(self.dl)
        return bow

    def aggregate_batch(self, sets):
        return np.stack([self.aggregate(s) for s in sets]) if len(sets) else np.zeros((0, self.nc))


def bow_numpy(codebook, descriptors, k=1):
    """independent numpy form for tie-free data: full distance matrix, stable argsort, np.add.at"""
    cb = np.asarray(codebook, np.float64)
    bow = np.zeros(cb.shape[0])
    if descriptors is None or len(descriptors) == 0:
        return bow
    X = np.asarray(descriptors, np.float64)
    d2 = ((X[:, None, :] - cb[None, :, :]) ** 2).sum(axis=2)
    nn = np.argsort(d2, axis=1, kind="stable")[:, :k]
    np.add.at(bow, nn.reshape(-1), 1.0 if k == 1 else float(cb.shape[1]))
    return bow
