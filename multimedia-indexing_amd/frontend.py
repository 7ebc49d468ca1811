"""Host-side mirror of the two steps that feed the index (BASELINE config 5), over the C ABI:

  gr.iti.mklab.visual.dimreduction.PCA                        (J/dimreduction/PCA.java)
  gr.iti.mklab.visual.aggregation.VladAggregator              (J/aggregation/VladAggregator.java)
  gr.iti.mklab.visual.aggregation.VladAggregatorMultipleVocabularies
  gr.iti.mklab.visual.aggregation.BowAggregator               (J/aggregation/BowAggregator.java)

Projection = one batched f64-MFMA GEMM, aggregation = one block per image.  The PCA basis is learned on the
GPU as well (addSample / addSamples, computeBasis, savePCAToFile: `mmidx_pca_learn_*`, a Gram matrix on the f64
matrix cores and a blocked subspace iteration in place of EJML's SVD; PCA.streaming: `mmidx_pca_stream_*`, the same from a
stream of samples that are not kept, up to 32768 -> 1024); codebooks: quantization.py.
"""
import ctypes as C

import numpy as np

from . import _native as N
from ._native import MmidxError


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class PCA:
    """PCA(numComponents, numTrainingSamples, sampleSize, doWhitening), PCA.java:75-93."""

    def __init__(self, numComponents, numTrainingSamples, sampleSize, doWhitening, device=0):
        self.numComponents, self.sampleSize, self.doWhitening = numComponents, sampleSize, bool(doWhitening)
        self.numTrainingSamples = numTrainingSamples
        self.device = device
        self._h = None
        self.isPcaInitialized = False
        if numComponents > sampleSize:  # IllegalArgumentException, PCA.java:102-104
            raise MmidxError(N.ERR_INVALID_ARG, "More components requested than the data's length.")
        # learning side (PCA.java:109-110, :135-177): the samples live in the learner's HBM, the results here
        self._learner = None
        self.sampleIndex = 0
        self.means = self.singularValues = self.V_t = None
        self.iterations = self.residual = None

    @classmethod
    def streaming(cls, numComponents, sampleSize, doWhitening, device=0):
        """A PCA that learns from a stream of samples (`mmidx_pca_stream_*`): no numTrainingSamples, the rows are folded into
        the Gram matrix as they arrive and are not kept, sampleSize up to 32768 (the flagship 32768 -> 1024 basis).
        addSample / addSamples / add_device feed it; computeBasis works on the rows so far and sets numTrainingSamples to their
        count; after it no more samples are taken.  Everything else is as on PCA."""
        p = cls(numComponents, 0, sampleSize, doWhitening, device)
        p._streaming = True
        return p

    _streaming = False

    # ---- learning: addSample / computeBasis / savePCAToFile (PCA.java:120-177, :219-247) ----
    def addSamples(self, X):
        """Batch form of addSample: rows of X [n][sampleSize] in arrival order."""
        X = _f64(X)
        if X.ndim != 2:
            raise MmidxError(N.ERR_WRONG_DIM, "Unexpected sample size")
        if self._streaming:
            if X.shape[1] != self.sampleSize:
                raise MmidxError(N.ERR_WRONG_DIM, "Unexpected sample size")  # PCA.java:123-124
            if X.shape[0] == 0:
                return
            self._ensure_learner()
            N.check(N.lib().mmidx_pca_stream_add(self._learner, X.shape[0], X.ctypes.data))
            self.sampleIndex += X.shape[0]
            return
        if self.sampleIndex + X.shape[0] > self.numTrainingSamples:
            raise MmidxError(N.ERR_INVALID_ARG, "Too many samples")  # PCA.java:121-122
        if X.shape[1] != self.sampleSize:
            raise MmidxError(N.ERR_WRONG_DIM, "Unexpected sample size")  # PCA.java:123-124
        if X.shape[0] == 0:
            return
        self._ensure_learner()
        N.check(N.lib().mmidx_pca_learn_add(self._learner, X.shape[0], X.ctypes.data))
        self.sampleIndex += X.shape[0]

    def addSample(self, sampleData):
        """PCA.java:120-130"""
        if not self._streaming and self.sampleIndex >= self.numTrainingSamples:
            raise MmidxError(N.ERR_INVALID_ARG, "Too many samples")
        x = _f64(sampleData)
        if x.ndim != 1 or x.shape[0] != self.sampleSize:
            raise MmidxError(N.ERR_WRONG_DIM, "Unexpected sample size")
        self.addSamples(x.reshape(1, -1))

    def add_device(self, dX, n, stream=None):
        """n rows of sampleSize doubles that already lie in the HBM of this PCA's device (dX: a device address, or an object
        with data_ptr()), in arrival order; asynchronous on `stream` (a stream address; None = the device's default stream)."""
        ptr = dX.data_ptr() if hasattr(dX, "data_ptr") else int(dX)
        n = int(n)
        if not self._streaming and self.sampleIndex + n > self.numTrainingSamples:
            raise MmidxError(N.ERR_INVALID_ARG, "Too many samples")
        if n <= 0:
            return
        self._ensure_learner()
        add = N.lib().mmidx_pca_stream_add_device if self._streaming else N.lib().mmidx_pca_learn_add_device
        N.check(add(self._learner, n, ptr, stream))
        self.sampleIndex += n

    def _ensure_learner(self):
        if self._learner is None and self._streaming:
            h = C.c_void_p()
            N.check(N.lib().mmidx_pca_stream_create(self.numComponents, self.sampleSize, self.device, C.byref(h)))
            self._learner = h
        if self._learner is None:
            h = C.c_void_p()
            N.check(N.lib().mmidx_pca_learn_create(self.numComponents, self.numTrainingSamples, self.sampleSize, self.device, C.byref(h)))
            self._learner = h

    def computeBasis(self, tol=1e-12, max_iter=200):
        """PCA.java:135-177 on the GPU.  Fills .means [sampleSize], .singularValues [numComponents] (singular values of the centred
        sample matrix, descending -- NOT divided by n: the reference's line 2, W.get(i, i)) and .V_t [numComponents][sampleSize]
        (in every row the entry of largest magnitude is positive; EJML's row signs are arbitrary), .iterations, .residual.
        Raises MmidxError(status NOT_CONVERGED) when max_iter is reached above tol; the fields are filled all the same."""
        if self._streaming:
            self.numSamples = self.numTrainingSamples = self.sampleIndex  # the count at computeBasis
        if self.sampleIndex != self.numTrainingSamples:
            raise MmidxError(N.ERR_INVALID_ARG, "Not all the data has been added")  # PCA.java:136-137
        if self.numComponents > self.numTrainingSamples:
            raise MmidxError(N.ERR_INVALID_ARG, "More data needed to compute the desired number of components")  # :138-140
        self._ensure_learner()
        means, sv = np.zeros(self.sampleSize), np.zeros(self.numComponents)
        Vt = np.zeros((self.numComponents, self.sampleSize))
        it, res = C.c_int32(0), C.c_double(0.0)
        compute = N.lib().mmidx_pca_stream_compute if self._streaming else N.lib().mmidx_pca_learn_compute
        st = compute(self._learner, float(tol), int(max_iter), means.ctypes.data, sv.ctypes.data, Vt.ctypes.data, C.byref(it), C.byref(res))
        if st in (N.OK, N.ERR_NOT_CONVERGED):
            self.means, self.singularValues, self.V_t = means, sv, Vt
            self.iterations, self.residual = int(it.value), float(res.value)
        N.check(st)

    def setCompact(self, compact):
        """PCA.java:320-322 chooses between EJML's two SVD forms; there is one method here: a no-op kept for drop-in callers."""

    def savePCAToFile(self, PCAFileName):
        """PCA.java:219-247: line 1 means, line 2 singular values, then one component per line, space separated; repr(float)
        is the shortest text that parses back to the same double (as Java's Double.toString round-trips)."""
        if self.isPcaInitialized:
            raise MmidxError(N.ERR_INVALID_ARG, "Cannot save, PCA is initialized!")  # :220-222
        if self.V_t is None:
            raise MmidxError(N.ERR_NOT_READY, "Cannot save to file, PCA matrix is null!")  # :223-225
        with open(PCAFileName, "w") as f:
            f.write(" ".join(repr(float(v)) for v in self.means) + "\n")
            f.write(" ".join(repr(float(v)) for v in self.singularValues) + "\n")
            for row in self.V_t:
                f.write(" ".join(repr(float(v)) for v in row) + "\n")

    def loadPCAFromFile(self, filename):
        """PCA.java:257-318: line 1 means, line 2 eigenvalues, then one component per line (space separated)."""
        with open(filename) as f:
            means = np.array(f.readline().strip().split(" "), dtype=np.float64)
            if means.shape[0] != self.sampleSize:
                raise MmidxError(N.ERR_INVALID_ARG, "Means line is wrong!")
            eig_line = f.readline()
            eig = None
            if self.doWhitening:
                eig = np.array(eig_line.strip().split(" "), dtype=np.float64)
                if eig.shape[0] < self.numComponents:
                    raise MmidxError(N.ERR_INVALID_ARG, "Eigenvalues line is wrong!")
            Vt = np.zeros((self.numComponents, self.sampleSize))
            for i in range(self.numComponents):
                Vt[i] = np.array(f.readline().strip().split(" ")[: self.sampleSize], dtype=np.float64)
        self.load(means, eig, Vt)

    def load(self, means, eig, Vt):
        """Same as loadPCAFromFile with the parsed arrays (Vt = raw components, whitening folded natively)."""
        means, Vt = _f64(means), _f64(Vt).reshape(self.numComponents, self.sampleSize)
        eig = _f64(eig)[: self.numComponents].copy() if eig is not None else None
        h = C.c_void_p()
        N.check(N.lib().mmidx_pca_create(self.numComponents, self.sampleSize, int(self.doWhitening), means.ctypes.data,
                                         eig.ctypes.data if eig is not None else None, Vt.ctypes.data, self.device, C.byref(h)))
        if self._h:  # (a learner in progress is left alone)
            N.lib().mmidx_pca_destroy(self._h)
        self._h = h
        self.isPcaInitialized = True

    def project(self, X):
        """Batch form of sampleToEigenSpace: X [n][sampleSize] -> [n][numComponents]."""
        if not self.isPcaInitialized:
            raise MmidxError(N.ERR_NOT_READY, "PCA is not correctly initiallized!")  # sic, PCA.java:191
        X = _f64(X)
        if X.ndim != 2 or X.shape[1] != self.sampleSize:
            raise MmidxError(N.ERR_WRONG_DIM, "Unexpected vector length!")  # IllegalArgumentException, PCA.java:194
        Y = np.zeros((X.shape[0], self.numComponents))
        N.check(N.lib().mmidx_pca_project(self._h, X.shape[0], X.ctypes.data, Y.ctypes.data))
        return Y

    def sampleToEigenSpace(self, sampleData):
        """PCA.java:188-208 (does not modify its argument)."""
        x = _f64(sampleData)
        if x.ndim != 1 or x.shape[0] != self.sampleSize:
            raise MmidxError(N.ERR_WRONG_DIM, "Unexpected vector length!")
        return self.project(x.reshape(1, -1))[0]

    def close(self):
        if self._h:
            N.lib().mmidx_pca_destroy(self._h)
            self._h = None
        if getattr(self, "_learner", None):
            (N.lib().mmidx_pca_stream_destroy if self._streaming else N.lib().mmidx_pca_learn_destroy)(self._learner)
            self._learner = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class VladAggregatorMultipleVocabularies:
    """VladAggregatorMultipleVocabularies(double[][][] codebooks), normalizationsOn default true."""

    def __init__(self, codebooks, normalizationsOn=True, device=0):
        cbs = [_f64(cb) for cb in codebooks]
        self.descriptorLength = cbs[0].shape[1]
        self.numCentroids = [cb.shape[0] for cb in cbs]
        self.normalizationsOn = bool(normalizationsOn)
        ncent = np.array(self.numCentroids, np.int32)
        cat = np.ascontiguousarray(np.concatenate([cb.reshape(-1) for cb in cbs]))
        h = C.c_void_p()
        N.check(N.lib().mmidx_vlad_create(len(cbs), ncent.ctypes.data, self.descriptorLength, cat.ctypes.data,
                                          int(self.normalizationsOn), device, C.byref(h)))
        self._h = h
        self.vectorLength = int(sum(self.numCentroids)) * self.descriptorLength

    def getVectorLength(self):
        return self.vectorLength

    def aggregate_batch(self, descriptor_sets):
        """descriptor_sets: list of [n_i][descriptorLength] arrays (n_i may be 0) -> [nimg][vectorLength]."""
        nimg = len(descriptor_sets)
        off = np.zeros(nimg + 1, np.int64)
        for i, d in enumerate(descriptor_sets):
            off[i + 1] = off[i] + (0 if d is None else len(d))
        total = int(off[-1])
        descs = np.zeros((max(total, 1), self.descriptorLength))
        for i, d in enumerate(descriptor_sets):
            if off[i + 1] > off[i]:
                descs[off[i]:off[i + 1]] = _f64(d).reshape(-1, self.descriptorLength)
        out = np.zeros((nimg, self.vectorLength))
        N.check(N.lib().mmidx_vlad_aggregate(self._h, nimg, off.ctypes.data, descs.ctypes.data, out.ctypes.data))
        return out

    def set_option(self, name, value):
        """measurement / test switch: "exact" = 1 -> the one-kernel form with the fp64 brute-force assignment"""
        N.check(N.lib().mmidx_vlad_set_option(self._h, name.encode(), int(value)))

    def aggregate(self, descriptors):
        """VladAggregatorMultipleVocabularies.aggregate(double[][]), :84-101"""
        return self.aggregate_batch([descriptors])[0]

    def close(self):
        if getattr(self, "_h", None):
            N.lib().mmidx_vlad_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class VladAggregator(VladAggregatorMultipleVocabularies):
    """VladAggregator(double[][] codebook): raw VLAD, no normalisation (VladAggregator.java:56-70)."""

    def __init__(self, codebook, device=0):
        super().__init__([codebook], normalizationsOn=False, device=device)


class BowAggregator:
    """BowAggregator(double[][] codebook) / BowAggregator(double[][] codebook, int k), BowAggregator.java:24-37: raw bag-of-words
    counts, hard (k = 1) or soft over the k nearest centroids -- where every (descriptor, neighbour) hit adds descriptorLength, as
    the reference's inner loop does (:47-51).  Bit-exact; no normalisation."""

    def __init__(self, codebook, k=1, device=0):
        cb = _f64(codebook)
        if cb.ndim != 2:
            raise MmidxError(N.ERR_INVALID_ARG, "the codebook is a [numCentroids][descriptorLength] array")
        self.numCentroids, self.descriptorLength, self.k = int(cb.shape[0]), int(cb.shape[1]), int(k)
        h = C.c_void_p()
        N.check(N.lib().mmidx_bow_create(self.numCentroids, self.descriptorLength, self.k, cb.ctypes.data, device, C.byref(h)))
        self._h = h

    def getVectorLength(self):
        return self.numCentroids

    def getNumCentroids(self):
        return self.numCentroids

    def getDescriptorLength(self):
        return self.descriptorLength

    def _rows(self, d):
        """one image's descriptors as [n][descriptorLength]; AbstractFeatureAggregator.aggregate's check, AFA:72-79"""
        if d is None or len(d) == 0:
            return None
        a = _f64(d)
        if a.ndim != 2 or a.shape[1] != self.descriptorLength:
            raise MmidxError(N.ERR_WRONG_DIM, "Descriptor length is incompatible with codebook centroid length!")
        return a

    def aggregate_batch(self, descriptor_sets):
        """descriptor_sets: list of [n_i][descriptorLength] arrays (n_i may be 0) -> [nimg][numCentroids]."""
        rows = [self._rows(d) for d in descriptor_sets]
        nimg = len(rows)
        off = np.zeros(nimg + 1, np.int64)
        for i, a in enumerate(rows):
            off[i + 1] = off[i] + (0 if a is None else a.shape[0])
        descs = np.zeros((max(int(off[-1]), 1), self.descriptorLength))
        for i, a in enumerate(rows):
            if a is not None:
                descs[off[i]:off[i + 1]] = a
        out = np.zeros((nimg, self.numCentroids))
        N.check(N.lib().mmidx_bow_aggregate(self._h, nimg, off.ctypes.data, descs.ctypes.data, out.ctypes.data))
        return out

    def aggregate(self, descriptors):
        """BowAggregator.aggregateInternal(double[][]), :39-74"""
        return self.aggregate_batch([descriptors])[0]

    def set_option(self, name, value):
        """measurement / test switches, none changes a result: "exact" = 1 (fp64 assignment), "hist_global" = 1 (the global-memory
        histogram also where the LDS form applies), "chunk_images" = n (images per round of the host form, 0 = automatic)"""
        N.check(N.lib().mmidx_bow_set_option(self._h, name.encode(), int(value)))

    def close(self):
        if getattr(self, "_h", None):
            N.lib().mmidx_bow_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ImageVectorizer:
    """Batch form of ImageVectorization.transformToVector (J/vectorization/ImageVectorization.java:169-208):
    descriptors -> VLAD -> PCA projection in one native call (`mmidx_vectorize`), replacing the reference's
    per-image thread pool (ImageVectorizer.java:123-126); the 8192-d VLAD vectors never leave the GPU."""

    def __init__(self, aggregator, pca):
        if not isinstance(aggregator, VladAggregatorMultipleVocabularies):  # (mmidx_vectorize takes a mmidx_vlad handle and nothing else)
            raise MmidxError(N.ERR_INVALID_ARG, "ImageVectorizer needs a VLAD aggregator (ImageVectorization is VLAD-only), got "
                             + type(aggregator).__name__)
        if aggregator.getVectorLength() != pca.sampleSize:
            raise MmidxError(N.ERR_WRONG_DIM, "aggregator vector length does not match the PCA sample size")
        self.aggregator, self.pca = aggregator, pca

    def transform_batch(self, descriptor_sets):
        """descriptor_sets: list of [n_i][descriptorLength] arrays -> [nimg][numComponents]"""
        ag = self.aggregator
        nimg = len(descriptor_sets)
        off = np.zeros(nimg + 1, np.int64)
        for i, d in enumerate(descriptor_sets):
            off[i + 1] = off[i] + (0 if d is None else len(d))
        total = int(off[-1])
        descs = np.zeros((max(total, 1), ag.descriptorLength))
        for i, d in enumerate(descriptor_sets):
            if off[i + 1] > off[i]:
                descs[off[i]:off[i + 1]] = _f64(d).reshape(-1, ag.descriptorLength)
        out = np.zeros((nimg, self.pca.numComponents))
        N.check(N.lib().mmidx_vectorize(ag._h, self.pca._h, nimg, off.ctypes.data, descs.ctypes.data, out.ctypes.data))
        return out

    def transformToVector(self, descriptors):
        return self.transform_batch([descriptors])[0]
