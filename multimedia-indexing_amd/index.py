"""Host-side mirror of the reference's index classes over the C ABI.

Same names, argument meaning and error behaviour as
  gr.iti.mklab.visual.datastructures.{AbstractSearchStructure, PQ, IVFPQ}
(J/ = src/main/java/gr/iti/mklab/visual/ in the reference tree), so that parity tests read like
tests of the reference.  The reference keeps id <-> iid maps and the persistent records in
BDB-JE; that half stays on the Java side of the JNI boundary and is represented
here by plain dicts.  All vector arithmetic happens in libmmidx_hip.so on the GPU.
"""
import ctypes as C
import time

import os

import numpy as np

from . import _native as N
from ._native import MmidxError


class TransformationType:
    """PQ.TransformationType, J/datastructures/PQ.java:78-80"""
    None_ = 0
    RandomRotation = 1
    RandomPermutation = 2


class Answer:
    """J/utilities/Answer.java:8-60 (timers are nanoseconds, ASS:285-287, :352-358)."""

    def __init__(self, ids, distances, nameLookupTime, indexSearchTime):
        self._ids, self._distances = ids, distances
        self._nameLookupTime, self._indexSearchTime = nameLookupTime, indexSearchTime

    def getIds(self):
        return self._ids

    def getDistances(self):
        return self._distances

    def getIndexSearchTime(self):
        return self._indexSearchTime

    def getNameLookupTime(self):
        return self._nameLookupTime


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a


def read_quantizer(filename, num_centroids, centroid_length):
    """AbstractFeatureAggregator.readQuantizer, J/aggregation/AbstractFeatureAggregator.java:234-254:
    one centroid per line, comma separated; lines without a comma are skipped as headers."""
    q = np.zeros((num_centroids, centroid_length), np.float64)
    counter = 0
    with open(filename) as f:
        for line in f:
            line = line.rstrip("\n")
            if "," not in line:
                continue
            vals = line.split(",")
            for i, v in enumerate(vals):
                q[counter, i] = float(v)
            counter += 1
    return q


class AbstractSearchStructure:
    """Template-method base, J/datastructures/AbstractSearchStructure.java."""

    def __init__(self, vectorLength, maxNumVectors, readOnly=False, countSizeOnLoad=True, loadCounter=0,
                 loadIndexInMemory=True, cacheSize=512):
        self.vectorLength = vectorLength
        self.maxNumVectors = maxNumVectors
        self.readOnly = readOnly
        self.loadCounter = loadCounter
        self.loadIndexInMemory = loadIndexInMemory
        self._id_to_iid = {}
        self._iid_to_id = {}
        self._h = None

    # -- id maps (BDB in the reference: ASS:383-419, :537-562) --
    def getInternalId(self, id_):
        return self._id_to_iid.get(id_, -1)

    def getId(self, iid):
        return self._iid_to_id.get(int(iid))

    def isIndexed(self, id_):
        return id_ in self._id_to_iid

    def getLoadCounter(self):
        return self.loadCounter

    def _create_mapping(self, id_):
        self._iid_to_id[self.loadCounter] = id_
        self._id_to_iid[id_] = self.loadCounter

    # -- ASS:229-257 --
    def indexVector(self, id_, vector):
        if self.loadCounter >= self.maxNumVectors:
            print("Maximum index capacity reached, no more vectors can be indexed!")
            return False
        if self.isIndexed(id_):
            print(f"Vector '{id_}' already indexed!")
            return False
        vector = np.asarray(vector, dtype=np.float64)
        # dimension check first so that a failed call leaves no mapping behind
        if vector.ndim != 1 or vector.shape[0] != self.vectorLength:
            raise MmidxError(N.ERR_WRONG_DIM, "The dimensionality of the vector is wrong!")
        self._create_mapping(id_)
        try:
            self.indexVectorInternal(vector)
        except Exception:
            # a failed native call must not leave the id marked as indexed (the reference's createMapping precedes
            # indexVectorInternal too, ASS:244-248, but its only failure there is the dimension check done above)
            self._iid_to_id.pop(self.loadCounter, None)
            self._id_to_iid.pop(id_, None)
            raise
        self.loadCounter += 1
        return True

    def indexVectors(self, ids, vectors):
        """Batch overload (one launch for the whole batch); same checks per id."""
        vectors = _f64(vectors)
        if vectors.ndim != 2 or vectors.shape[1] != self.vectorLength:
            raise MmidxError(N.ERR_WRONG_DIM, "The dimensionality of the vector is wrong!")
        keep, seen = [], set()
        for i, id_ in enumerate(ids):
            if self.loadCounter + len(keep) >= self.maxNumVectors:
                print("Maximum index capacity reached, no more vectors can be indexed!")
                break
            if self.isIndexed(id_) or id_ in seen:
                print(f"Vector '{id_}' already indexed!")
                continue
            keep.append(i)
            seen.add(id_)
        if not keep:
            return 0
        iids = np.arange(self.loadCounter, self.loadCounter + len(keep), dtype=np.int32)
        self._add_vectors(vectors[keep], iids)
        for i in keep:
            self._create_mapping(ids[i])
            self.loadCounter += 1
        return len(keep)

    # -- removal (an extension of the reference, which can only index: DESIGN.md section 5.13) --
    def removeVectors(self, ids):
        """Take the vectors with these external ids out of the index: their records leave the GPU (remove_batch) and both id maps
        lose their entries, so isIndexed is false and getInternalId answers -1 afterwards.  An id that is not indexed is reported
        with a printed line, in the style of indexVector's duplicate check, and skipped.  Returns the number of ids removed.
        loadCounter is NOT decremented: it hands out internal ids, which must stay unique, and it bounds maxNumVectors as the
        reference's capacity check does -- a removed record does not give its capacity back."""
        iids, seen = [], set()
        for id_ in ids:
            if not self.isIndexed(id_):
                print(f"Vector '{id_}' is not indexed!")
                continue
            if id_ in seen:
                continue
            seen.add(id_)
            iids.append(self._id_to_iid[id_])
        if not iids:
            return 0
        self.remove_batch(np.array(iids, np.int32))
        for id_ in seen:
            self._iid_to_id.pop(self._id_to_iid.pop(id_), None)
        return len(iids)

    def removeVector(self, id_):
        """removeVectors for one id: False (and a printed line) where it is not indexed"""
        return self.removeVectors([id_]) == 1

    def replaceVector(self, id_, vector):
        """Update: remove, then indexVector.  The record gets a fresh internal id (and, like any add, needs capacity left).
        What can be refused is refused before the removal -- a wrong length, an id that is not indexed, a full index -- but the two
        steps are NOT one atomic step: if the native add fails after the removal (a device error, say), the old record is gone and
        the id is not indexed; the exception of indexVector reaches the caller, who indexes the vector again."""
        vector = np.asarray(vector, dtype=np.float64)
        if vector.ndim != 1 or vector.shape[0] != self.vectorLength:
            raise MmidxError(N.ERR_WRONG_DIM, "The dimensionality of the vector is wrong!")
        if not self.isIndexed(id_):
            print(f"Vector '{id_}' is not indexed!")
            return False
        if self.loadCounter >= self.maxNumVectors:
            print("Maximum index capacity reached, no more vectors can be indexed!")
            return False
        if not self.removeVector(id_):
            return False
        return self.indexVector(id_, vector)

    def remove_batch(self, iids):
        # (Linear: its internal id is the row number, and the exact re-ranking rests on that -- only PQ and IVFPQ override this)
        raise MmidxError(N.ERR_UNSUPPORTED, "this index cannot remove records: its internal ids are row numbers")

    # -- ASS:281-291, :320-328, :345-373 --
    def computeNearestNeighbors(self, k, query):
        if isinstance(query, str):
            iid = self.getInternalId(query)
            start = time.perf_counter_ns()
            res = self.computeNearestNeighborsInternalById(k, iid)
            return self._look_up(res, time.perf_counter_ns() - start)
        if not self.loadIndexInMemory:
            raise MmidxError(N.ERR_NOT_IN_MEMORY, "Cannot execute query because the index is not loaded in memory!")
        start = time.perf_counter_ns()
        res = self.computeNearestNeighborsInternal(k, query)
        return self._look_up(res, time.perf_counter_ns() - start)

    def _look_up(self, res, search_ns):
        iids, dists = res
        start = time.perf_counter_ns()
        ids = [self.getId(i) for i in iids]
        return Answer(ids, np.array(dists, dtype=np.float64), time.perf_counter_ns() - start, search_ns)

    def close(self):
        if self._h:
            N.lib().mmidx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _PQBase(AbstractSearchStructure):
    _kind = None

    def _create(self, numSubVectors, numProductCentroids, transformation, numCoarseCentroids, device, perm, rot):
        self.numSubVectors = numSubVectors
        self.numProductCentroids = numProductCentroids
        self.transformation = transformation
        self.numCoarseCentroids = numCoarseCentroids
        L = N.lib()
        h = C.c_void_p()
        pp = rp = None
        if perm is not None:
            self._perm = np.ascontiguousarray(perm, np.int32)
            pp = self._perm.ctypes.data
        if rot is not None:
            self._rot = _f64(rot)
            rp = self._rot.ctypes.data
        devices = getattr(self, "_devices", None)
        if devices is not None:
            # one index over several GPUs from this one process (mmidx_create_sharded; the Java form is -Dmmidx.devices=0,1,...)
            N.preload_rccl()
            self._devs = (C.c_int * len(devices))(*[int(d) for d in devices])
            N.check(L.mmidx_create_sharded(self._kind, self.vectorLength, numSubVectors, numProductCentroids, numCoarseCentroids,
                                           transformation, pp, rp, len(devices), self._devs, C.byref(h)))
        else:
            N.check(L.mmidx_create(self._kind, self.vectorLength, numSubVectors, numProductCentroids, numCoarseCentroids,
                                   transformation, pp, rp, device, C.byref(h)))
        self._h = h
        self.subVectorLength = self.vectorLength // numSubVectors
        self._code_dtype = np.int8 if numProductCentroids <= 256 else np.int16

    # ---- quantizers ----
    def loadProductQuantizer(self, filename_or_array):
        """IVFPQ.java:275-288 / PQ.java:210-223: m*ks lines of dsub comma-separated doubles."""
        m, ks, ds = self.numSubVectors, self.numProductCentroids, self.subVectorLength
        if isinstance(filename_or_array, str):
            pq = np.zeros((m, ks, ds), np.float64)
            with open(filename_or_array) as f:
                for i in range(m):
                    for j in range(ks):
                        parts = f.readline().split(",")
                        for t in range(ds):
                            pq[i, j, t] = float(parts[t])
        else:
            pq = _f64(filename_or_array, (m, ks, ds))
        N.check(N.lib().mmidx_set_pq(self._h, pq.ctypes.data))

    # ---- native calls ----
    def _add_vectors(self, X, iids):
        X = _f64(X)
        iids = np.ascontiguousarray(iids, np.int32)
        N.check(N.lib().mmidx_add_vectors(self._h, X.shape[0], X.ctypes.data, iids.ctypes.data, None, None))

    def indexVectorInternal(self, vector):
        if len(vector) != self.vectorLength:
            raise MmidxError(N.ERR_WRONG_DIM, "The dimensionality of the vector is wrong!")
        self._add_vectors(_f64(vector).reshape(1, -1), np.array([self.loadCounter], np.int32))

    def encode(self, X):
        """cells [n] (-1 for PQ), codes [n][m] in the stored form (int8 = idx-128 / int16)."""
        X = _f64(X)
        if X.ndim != 2 or X.shape[1] != self.vectorLength:
            raise MmidxError(N.ERR_WRONG_DIM, "The dimensionality of the vector is wrong!")
        cells = np.zeros(X.shape[0], np.int32)
        codes = np.zeros((X.shape[0], self.numSubVectors), self._code_dtype)
        N.check(N.lib().mmidx_encode(self._h, X.shape[0], X.ctypes.data, cells.ctypes.data, codes.ctypes.data))
        return cells, codes

    def search_batch(self, k, Q):
        """Batch overload of computeNearestNeighborsInternal: (iids [nq][k], dists [nq][k], counts [nq])."""
        Q = _f64(Q)
        if Q.ndim != 2 or Q.shape[1] != self.vectorLength:
            raise MmidxError(N.ERR_WRONG_DIM, "The dimensionality of the vector is wrong!")
        nq = Q.shape[0]
        iids = np.full((nq, max(k, 1)), -1, np.int32)
        dists = np.full((nq, max(k, 1)), np.inf, np.float64)
        counts = np.zeros(nq, np.int32)
        N.check(N.lib().mmidx_search(self._h, k, nq, Q.ctypes.data, iids.ctypes.data, dists.ctypes.data, counts.ctypes.data))
        return iids, dists, counts

    def computeNearestNeighborsInternal(self, k, query):
        iids, dists, counts = self.search_batch(k, _f64(query).reshape(1, -1))
        n = int(counts[0])
        return iids[0, :n].copy(), dists[0, :n].copy()

    def search_sdc_batch(self, k, iids):
        """Batch form of computeNearestNeighborsInternal(k, int iid): PQ.computeKnnSDC, PQ.java:334-374."""
        iids = np.ascontiguousarray(iids, np.int32)
        nq = iids.shape[0]
        out_i = np.full((nq, max(k, 1)), -1, np.int32)
        out_d = np.full((nq, max(k, 1)), np.inf, np.float64)
        cnt = np.zeros(nq, np.int32)
        N.check(N.lib().mmidx_search_sdc(self._h, k, nq, iids.ctypes.data, out_i.ctypes.data, out_d.ctypes.data, cnt.ctypes.data))
        return out_i, out_d, cnt

    def computeNearestNeighborsInternalById(self, k, iid):
        # PQ: computeKnnSDC (PQ.java:334-374), the reference's behaviour.  (IVFPQ overrides this: the SDC call reports
        # UNSUPPORTED on its handles, the reference's computeKnnIVFSDC being a stub.)
        if iid < 0:
            raise MmidxError(N.ERR_INVALID_ARG, "Id does not exist!")
        i, d, c = self.search_sdc_batch(k, np.array([iid], np.int32))
        n = int(c[0])
        return i[0, :n].copy(), d[0, :n].copy()

    # -- queries by indexed id and the vectors behind the records (an extension of the reference: DESIGN.md section 5.9) --
    def reconstruct(self, iids):
        """[n][vectorLength]: the vector the index holds for each internal id -- the codebook rows its code selects, the
        transformation undone, for IVFPQ subtracted from the centroid of its list.  An unknown id raises "Id does not exist!"."""
        q = np.ascontiguousarray(np.asarray(iids).reshape(-1), np.int32)
        out = np.zeros((q.shape[0], self.vectorLength), np.float64)
        N.check(N.lib().mmidx_reconstruct(self._h, q.shape[0], q.ctypes.data, out.ctypes.data))
        return out

    def reconstructVector(self, id_):
        """reconstruct by external id: the counterpart of Linear.getVector for a quantized index"""
        iid = self.getInternalId(id_)
        if iid == -1:
            raise MmidxError(N.ERR_INVALID_ARG, "Id does not exist!")
        return self.reconstruct([iid])[0]

    def search_ids_batch(self, k, iids):
        """search_batch with the reconstructed vectors of the given internal ids as the queries (they never leave the device):
        computeKnnIVFADC / computeKnnADC on the handle's usual search path.  Every query's own record is among its answers."""
        q = np.ascontiguousarray(np.asarray(iids).reshape(-1), np.int32)
        nq = q.shape[0]
        out = np.full((nq, max(k, 1)), -1, np.int32)
        dists = np.full((nq, max(k, 1)), np.inf, np.float64)
        counts = np.zeros(nq, np.int32)
        N.check(N.lib().mmidx_search_ids(self._h, k, nq, q.ctypes.data, out.ctypes.data, dists.ctypes.data, counts.ctypes.data))
        return out, dists, counts

    # -- exact re-ranking against a Linear index over the same vectors (an extension of the reference: DESIGN.md section 5.11) --
    def search_refine_batch(self, k, R, Q, linear):
        """The R best records of search_batch(R, Q), re-ranked by their exact distances from the rows of `linear` (record iid = row
        iid, as IndexTransformation.java:113-122 builds the pair), the k best kept under the bounded queue's rule:
        (iids [nq][k], exact squared distances [nq][k], counts [nq], missing).  `missing` counts candidates without a row."""
        Q = _f64(Q)
        if Q.ndim != 2 or Q.shape[1] != self.vectorLength:
            raise MmidxError(N.ERR_WRONG_DIM, "The dimensionality of the vector is wrong!")
        nq = Q.shape[0]
        iids = np.full((nq, max(k, 1)), -1, np.int32)
        dists = np.full((nq, max(k, 1)), np.inf, np.float64)
        counts = np.zeros(nq, np.int32)
        missing = C.c_int64(0)
        N.check(N.lib().mmidx_search_refine(self._h, linear._h, k, R, nq, Q.ctypes.data, iids.ctypes.data, dists.ctypes.data, counts.ctypes.data,
                                            C.byref(missing)))
        return iids, dists, counts, missing.value

    def search_refine_ids_batch(self, k, R, iids, linear):
        """search_refine_batch with the rows iids[q] of `linear` as the queries (gathered on the device, Linear.java:181-184).  An id
        outside the Linear index gives count 0 and a padded row."""
        q = np.ascontiguousarray(np.asarray(iids).reshape(-1), np.int32)
        nq = q.shape[0]
        out = np.full((nq, max(k, 1)), -1, np.int32)
        dists = np.full((nq, max(k, 1)), np.inf, np.float64)
        counts = np.zeros(nq, np.int32)
        missing = C.c_int64(0)
        N.check(N.lib().mmidx_search_refine_ids(self._h, linear._h, k, R, nq, q.ctypes.data, out.ctypes.data, dists.ctypes.data, counts.ctypes.data,
                                                C.byref(missing)))
        return out, dists, counts, missing.value

    def search_refine_batch_device(self, k, R, Q, linear):
        """search_refine_batch on a torch tensor [nq][vectorLength] (float64, contiguous) in HBM: (ids int32 [nq][k], distances
        float64 [nq][k], counts int32 [nq], missing int64 [1]) as tensors on the same device, on torch's current stream; nothing
        is read back."""
        import torch

        if Q.dim() != 2 or Q.shape[1] != self.vectorLength or Q.dtype != torch.float64 or not Q.is_contiguous():
            raise MmidxError(N.ERR_WRONG_DIM, "The dimensionality of the vector is wrong!")
        nq = Q.shape[0]
        iids = torch.empty((nq, max(k, 1)), dtype=torch.int32, device=Q.device)
        dists = torch.empty((nq, max(k, 1)), dtype=torch.float64, device=Q.device)
        counts = torch.empty(nq, dtype=torch.int32, device=Q.device)
        missing = torch.zeros(1, dtype=torch.int64, device=Q.device)
        st = torch.cuda.current_stream(Q.device).cuda_stream
        N.check(N.lib().mmidx_search_refine_device(self._h, linear._h, k, R, nq, Q.data_ptr(), iids.data_ptr(), dists.data_ptr(), counts.data_ptr(),
                                                   missing.data_ptr(), st))
        return iids, dists, counts, missing

    def computeNearestNeighborsRefined(self, k, R, query, linear):
        """computeNearestNeighbors with the exact re-ranking: `query` is a vector or an indexed id (its row of `linear` is then the
        query).  The Answer carries this index's external ids and exact squared distances.  R is always explicit."""
        start = time.perf_counter_ns()
        if isinstance(query, str):
            iid = self.getInternalId(query)
            if iid < 0:
                raise MmidxError(N.ERR_INVALID_ARG, "Id does not exist!")
            i, d, c, _ = self.search_refine_ids_batch(k, R, [iid], linear)
        else:
            i, d, c, _ = self.search_refine_batch(k, R, _f64(query).reshape(1, -1), linear)
        n = int(c[0])
        return self._look_up((i[0, :n].copy(), d[0, :n].copy()), time.perf_counter_ns() - start)

    def remove_batch(self, iids):
        """mmidx_remove: every stored record whose internal id occurs in `iids` leaves the index; the survivors keep their list and
        their order inside it.  (found [n] int32: 1 where the id was stored before the call; removed: records, not request entries).
        Unknown, negative and repeated ids are no error.  The id maps are not touched: removeVectors does that."""
        q = np.ascontiguousarray(np.asarray(iids).reshape(-1), np.int32)
        found = np.zeros(q.shape[0], np.int32)
        removed = C.c_int64(0)
        N.check(N.lib().mmidx_remove(self._h, q.shape[0], q.ctypes.data, found.ctypes.data, C.byref(removed)))
        return found, removed.value

    def export(self):
        """List-major snapshot (list_off [nlists+1], iids [n], codes [n][m] stored form)."""
        nl = self.numCoarseCentroids if self._kind == N.KIND_IVFPQ else 1
        off = np.zeros(nl + 1, np.int64)
        N.check(N.lib().mmidx_export(self._h, off.ctypes.data, None, None))
        n = int(off[-1])
        iids = np.zeros(n, np.int32)
        codes = np.zeros((n, self.numSubVectors), self._code_dtype)
        N.check(N.lib().mmidx_export(self._h, off.ctypes.data, iids.ctypes.data, codes.ctypes.data))
        return off, iids, codes

    def saveSnapshot(self, filename):
        """Flat snapshot of the in-memory index for fast restart: the library's own file (mmidx_save: the
        list-major arrays loadIndexInMemory builds, IVFPQ.java:680-728) plus, next to it, the id map this mirror keeps where the
        Java side keeps its BDB environment (`filename`.ids.npz)."""
        N.check(N.lib().mmidx_save(self._h, os.fsencode(filename)))
        iids = np.array(sorted(self._iid_to_id), np.int32)
        # ids as a fixed-width unicode array: loadable without pickle (an untrusted snapshot must not be able to run code)
        ids = np.array([str(self._iid_to_id[int(i)]) for i in iids], dtype=str)
        np.savez(str(filename) + ".ids.npz", iids=iids, ids=ids, load_counter=np.int64(self.loadCounter))

    def loadSnapshot(self, filename):
        """Inverse of saveSnapshot on an empty index of the same shape (quantizers loaded separately, as after the reference's
        constructor): mmidx_load for the records, the sidecar for the id map."""
        N.check(N.lib().mmidx_load(self._h, os.fsencode(filename)))
        z = np.load(str(filename) + ".ids.npz", allow_pickle=False)
        for i, name in zip(z["iids"], z["ids"]):
            self._iid_to_id[int(i)] = str(name)
            self._id_to_iid[str(name)] = int(i)
        self.loadCounter = int(z["load_counter"])

    # -- per-id utilities (IVFPQ.java:464-497, :801-880; the reference reads the BDB record of the id) --
    def _record(self, id_):
        iid = self.getInternalId(id_)
        if iid == -1:
            raise MmidxError(N.ERR_INVALID_ARG, "Id does not exist!")
        iids = np.array([iid], np.int32)
        cell = np.zeros(1, np.int32)
        code = np.zeros((1, self.numSubVectors), self._code_dtype)
        N.check(N.lib().mmidx_get_codes(self._h, 1, iids.ctypes.data, cell.ctypes.data, code.ctypes.data))
        return int(cell[0]), code[0]

    def getPQCodeByte(self, id_):
        """IVFPQ.java:801-824: the stored byte code (index - 128) of the vector with the given id"""
        if self.getInternalId(id_) == -1:
            raise MmidxError(N.ERR_INVALID_ARG, "Id does not exist!")
        if self.numProductCentroids > 256:
            raise MmidxError(N.ERR_INVALID_ARG, "Call the short variant of the method!")
        return self._record(id_)[1]

    def getPQCodeShort(self, id_):
        """IVFPQ.java:833-856"""
        if self.getInternalId(id_) == -1:
            raise MmidxError(N.ERR_INVALID_ARG, "Id does not exist!")
        if self.numProductCentroids <= 256:
            raise MmidxError(N.ERR_INVALID_ARG, "Call the short variant of the method!")  # (sic: the reference's message)
        return self._record(id_)[1]

    def computeDistance(self, qVector, existingVecId):
        """distance between a query vector and the code of an indexed vector: IVFPQ.computeDistanceIVFADC, IVFPQ.java:464-497
        (for PQ: the same sum with the query in place of the residual)"""
        iid = self.getInternalId(existingVecId)
        if iid == -1:
            raise MmidxError(N.ERR_INVALID_ARG, "Id does not exist!")
        q = _f64(qVector, (1, self.vectorLength))
        iids = np.array([iid], np.int32)
        out = np.zeros(1, np.float64)
        N.check(N.lib().mmidx_distance(self._h, 1, q.ctypes.data, iids.ctypes.data, out.ctypes.data))
        return float(out[0])

    def size(self):
        n = C.c_int64()
        N.check(N.lib().mmidx_size(self._h, C.byref(n)))
        return n.value

    def set_profiling(self, on=True):
        N.check(N.lib().mmidx_set_profiling(self._h, int(on)))

    def set_option(self, name, value):
        """measurement / A-B switches of the native library (mmidx_set_option)"""
        N.check(N.lib().mmidx_set_option(self._h, name.encode(), int(value)))

    def get_stats(self):
        s = N.Stats()
        N.check(N.lib().mmidx_get_stats(self._h, C.byref(s)))
        return {f: getattr(s, f) for f, _ in N.Stats._fields_}

    def get_dispatch(self):
        """which kernel family served each stage of the most recent search sub-batch: {"coarse": .., "pass_a": .., "pre": .., "pass_b": ..,
        "coarse_mm": ..}, and of the most recent build call: "assign" (K6a'(rows) | K6a'(copies) | K6a | exact | -), "encode" (K6b' | K6b | -)
        and "flagged", the number of vectors that call sent to the exact redo as text ("-" where no certified kernel ran).
        "screened": the queries of that sub-batch the head-only screen's certificate served ("-" where the screen did not run; option
        "coarse_screen"), and last "near_only": the queries the coarse stage answered with the nearest cell alone.
        "pass_a" names the kernel that was launched: "K3(table in two halves)" only where k_scan_split ran (ADC, m = 128 byte codes, a
        chunk of at most 32768 codes), "K3(table in global scratch)" for every other table beyond the LDS, "K3" / "K3(single pass)"
        otherwise.  After search_sdc_batch "pass_a" is one of these three K3 forms, "pre" is "-" and "pass_b" is
        "K3(exact scan: symmetric distances)" on an index of several chunks, "-" on one chunk.  Diagnostic text of the native library
        (mmidx_get_dispatch): not a stable format."""
        buf = C.create_string_buffer(512)
        N.check(N.lib().mmidx_get_dispatch(self._h, buf, 512))
        return dict(kv.split("=", 1) for kv in buf.value.decode().split(";"))

    @staticmethod
    def transformToByte(code):
        """PQ.transformToByte, PQ.java:552-558"""
        return (np.asarray(code, np.int32) - 128).astype(np.int8)

    @staticmethod
    def transformToShort(code):
        """PQ.transformToShort, PQ.java:544-550"""
        return np.asarray(code, np.int32).astype(np.int16)


class PQ(_PQBase):
    """J/datastructures/PQ.java (exhaustive ADC search)."""
    _kind = N.KIND_PQ

    def __init__(self, vectorLength, maxNumVectors, readOnly, BDBEnvHome, numSubVectors, numProductCentroids,
                 transformation, *rest, device=0, perm=None, rot=None):
        # PQ.java:142-144 (11 args) and :197-198 (8 args: ..., cacheSize)
        if len(rest) == 1:
            countSizeOnLoad, loadCounter, loadIndexInMemory, cacheSize = True, 0, True, rest[0]
        elif len(rest) == 4:
            countSizeOnLoad, loadCounter, loadIndexInMemory, cacheSize = rest
        else:
            raise TypeError("PQ(vectorLength, maxNumVectors, readOnly, BDBEnvHome, numSubVectors, "
                            "numProductCentroids, transformation, [countSizeOnLoad, loadCounter, "
                            "loadIndexInMemory,] cacheSize)")
        super().__init__(vectorLength, maxNumVectors, readOnly, countSizeOnLoad, loadCounter, loadIndexInMemory, cacheSize)
        self.BDBEnvHome = BDBEnvHome
        self._create(numSubVectors, numProductCentroids, transformation, 0, device, perm, rot)

    def loadIndex(self, codes):
        """loadIndexInMemory PQ.java:436-483: codes [n][m] in the stored form, iid = position."""
        codes = np.ascontiguousarray(codes, self._code_dtype)
        n = codes.shape[0]
        iids = np.arange(self.loadCounter, self.loadCounter + n, dtype=np.int32)
        N.check(N.lib().mmidx_add_codes(self._h, n, iids.ctypes.data, None, codes.ctypes.data))
        for i in iids:
            self._create_mapping(str(int(i)))
            self.loadCounter += 1


class IVFPQ(_PQBase):
    """J/datastructures/IVFPQ.java (IVFADC)."""
    _kind = N.KIND_IVFPQ

    def __init__(self, vectorLength, maxNumVectors, readOnly, BDBEnvHome, numSubVectors, numProductCentroids,
                 transformation, numCoarseCentroids, *rest, device=0, perm=None, rot=None, devices=None):
        # IVFPQ.java:174-177 (12 args) and :261-263 (9 args: ..., cacheSize); devices = [0, 1, ...]: the inverted lists are
        # partitioned over these GPUs (a device listed twice = virtual shards: tests on a one-GPU box)
        self._devices = list(devices) if devices is not None else None
        if len(rest) == 1:
            countSizeOnLoad, loadCounter, loadIndexInMemory, cacheSize = True, 0, True, rest[0]
        elif len(rest) == 4:
            countSizeOnLoad, loadCounter, loadIndexInMemory, cacheSize = rest
        else:
            raise TypeError("IVFPQ(vectorLength, maxNumVectors, readOnly, BDBEnvHome, numSubVectors, "
                            "numProductCentroids, transformation, numCoarseCentroids, [countSizeOnLoad, "
                            "loadCounter, loadIndexInMemory,] cacheSize)")
        super().__init__(vectorLength, maxNumVectors, readOnly, countSizeOnLoad, loadCounter, loadIndexInMemory, cacheSize)
        self.BDBEnvHome = BDBEnvHome
        self._create(numSubVectors, numProductCentroids, transformation, numCoarseCentroids, device, perm, rot)

    def setW(self, w):
        """IVFPQ.java:95-97"""
        N.check(N.lib().mmidx_set_w(self._h, int(w)))

    def getW(self):
        w = C.c_int()
        N.check(N.lib().mmidx_get_w(self._h, C.byref(w)))
        return w.value

    def loadCoarseQuantizer(self, filename_or_array):
        """IVFPQ.java:297-300"""
        if isinstance(filename_or_array, str):
            cq = read_quantizer(filename_or_array, self.numCoarseCentroids, self.vectorLength)
        else:
            cq = _f64(filename_or_array, (self.numCoarseCentroids, self.vectorLength))
        N.check(N.lib().mmidx_set_coarse(self._h, cq.ctypes.data))

    def indexPQCode(self, id_, listId, code):
        """IVFPQ.java:357-386: append a pre-computed (id, listId, byte[] code)."""
        if self.numProductCentroids > 256:
            raise MmidxError(N.ERR_BYTE_OVERFLOW,
                             "Byte is not sufficient to enumerate the centroids of the product quantizer!")
        if self.loadCounter >= self.maxNumVectors:
            print("Maximum index capacity reached, no more vectors can be indexed!")
            return False
        if self.isIndexed(id_):
            print(f"Vector '{id_}' already indexed!")
            return False
        code = np.ascontiguousarray(code, np.int8).reshape(1, -1)
        iid = np.array([self.loadCounter], np.int32)
        cell = np.array([listId], np.int32)
        N.check(N.lib().mmidx_add_codes(self._h, 1, iid.ctypes.data, cell.ctypes.data, code.ctypes.data))
        self._create_mapping(id_)
        self.loadCounter += 1
        return True

    def loadIndex(self, iids, listIds, codes):
        """loadIndexInMemory IVFPQ.java:680-728: stream (iid, listId, code) records."""
        iids = np.ascontiguousarray(iids, np.int32)
        listIds = np.ascontiguousarray(listIds, np.int32)
        codes = np.ascontiguousarray(codes, self._code_dtype)
        N.check(N.lib().mmidx_add_codes(self._h, len(iids), iids.ctypes.data, listIds.ctypes.data, codes.ctypes.data))
        for i in iids:
            self._iid_to_id[int(i)] = str(int(i))
            self._id_to_iid[str(int(i))] = int(i)
        self.loadCounter += len(iids)

    def computeNearestNeighborsInternalById(self, k, iid):
        # The reference's computeKnnIVFSDC returns null (IVFPQ.java:509-511).  Here the id's record is decoded on the device and
        # searched as any vector (computeKnnIVFADC); the id's own record is among the answers, as in PQ.computeKnnSDC.
        if iid < 0:
            raise MmidxError(N.ERR_INVALID_ARG, "Id does not exist!")
        i, d, c = self.search_ids_batch(k, [int(iid)])
        n = int(c[0])
        return i[0, :n].copy(), d[0, :n].copy()

    def getInvertedListId(self, id_):
        """IVFPQ.java:865-880: the inverted list (coarse cell) of the vector with the given id"""
        return self._record(id_)[0]

    def computeDistanceIVFADC(self, qVector, existingVecId):
        """IVFPQ.java:464-497"""
        return self.computeDistance(qVector, existingVecId)

    def listSizes(self):
        out = np.zeros(self.numCoarseCentroids, np.int32)
        N.check(N.lib().mmidx_list_sizes(self._h, out.ctypes.data))
        return out

    def outputItemsPerList(self):
        """IVFPQ.java:654-673"""
        s = self.listSizes()
        print(f"Maximum number of vectors: {int(s.max())}")
        print(f"Minimum number of vectors: {int(s.min())}")
        print(f"Average number of vectors: {float(s.sum()) / self.numCoarseCentroids}")


class Linear(AbstractSearchStructure):
    """Linear(vectorLength, maxNumVectors, readOnly, BDBEnvHome, ...), J/datastructures/Linear.java:67-100: exhaustive
    exact search (BASELINE config 1).  indexVector / computeNearestNeighbors as everywhere; the arithmetic is the
    reference's (sequential fp64 squared distance per vector, bounded queue in index order, Linear.java:138-163)."""

    def __init__(self, vectorLength, maxNumVectors, readOnly=False, BDBEnvHome="", loadIndexInMemory=True, countSizeOnLoad=True,
                 loadCounter=0, device=0):
        super().__init__(vectorLength, maxNumVectors, readOnly, countSizeOnLoad, loadCounter, loadIndexInMemory)
        h = C.c_void_p()
        N.check(N.lib().mmidx_linear_create(vectorLength, maxNumVectors, device, C.byref(h)))
        self._h = h

    def _add_vectors(self, X, iids):
        X = _f64(X)
        N.check(N.lib().mmidx_linear_add(self._h, X.shape[0], X.ctypes.data))

    def indexVectorInternal(self, vector):
        if len(vector) != self.vectorLength:
            raise MmidxError(N.ERR_WRONG_DIM, "The dimensionality of the vector is wrong!")
        self._add_vectors(_f64(vector).reshape(1, -1), None)

    def search_batch(self, k, Q):
        Q = _f64(Q)
        if Q.ndim != 2 or Q.shape[1] != self.vectorLength:
            raise MmidxError(N.ERR_WRONG_DIM, "The dimensionality of the vector is wrong!")
        nq = Q.shape[0]
        iids = np.full((nq, max(k, 1)), -1, np.int32)
        dists = np.full((nq, max(k, 1)), np.inf, np.float64)
        counts = np.zeros(nq, np.int32)
        N.check(N.lib().mmidx_linear_search(self._h, k, nq, Q.ctypes.data, iids.ctypes.data, dists.ctypes.data, counts.ctypes.data))
        return iids, dists, counts

    def computeNearestNeighborsInternal(self, k, query):
        iids, dists, counts = self.search_batch(k, _f64(query).reshape(1, -1))
        n = int(counts[0])
        return iids[0, :n].copy(), dists[0, :n].copy()

    def add_device(self, X):
        """indexVectorInternal for the rows of a torch tensor [n][vectorLength] (float64, contiguous) already on the handle's
        device; runs on torch's current stream.  The rows get the next internal ids (no external ids are mapped)."""
        import torch

        if X.dim() != 2 or X.shape[1] != self.vectorLength or X.dtype != torch.float64 or not X.is_contiguous():
            raise MmidxError(N.ERR_WRONG_DIM, "The dimensionality of the vector is wrong!")
        st = torch.cuda.current_stream(X.device).cuda_stream
        N.check(N.lib().mmidx_linear_add_device(self._h, X.shape[0], X.data_ptr(), st))

    def search_batch_device(self, k, Q):
        """search_batch on a torch tensor [nq][vectorLength] (float64, contiguous) in HBM: (ids int32 [nq][k], distances
        float64 [nq][k], counts int32 [nq]) as tensors on the same device, on torch's current stream."""
        import torch

        if Q.dim() != 2 or Q.shape[1] != self.vectorLength or Q.dtype != torch.float64 or not Q.is_contiguous():
            raise MmidxError(N.ERR_WRONG_DIM, "The dimensionality of the vector is wrong!")
        nq = Q.shape[0]
        iids = torch.empty((nq, max(k, 1)), dtype=torch.int32, device=Q.device)
        dists = torch.empty((nq, max(k, 1)), dtype=torch.float64, device=Q.device)
        counts = torch.empty(nq, dtype=torch.int32, device=Q.device)
        st = torch.cuda.current_stream(Q.device).cuda_stream
        N.check(N.lib().mmidx_linear_search_device(self._h, k, nq, Q.data_ptr(), iids.data_ptr(), dists.data_ptr(), counts.data_ptr(), st))
        return iids, dists, counts

    def copy_rows_device(self, iid0, out):
        """rows iid0 .. iid0 + len(out) - 1 into the torch tensor out [n][vectorLength] (float64, contiguous, in HBM)"""
        import torch

        if out.dim() != 2 or out.shape[1] != self.vectorLength or out.dtype != torch.float64 or not out.is_contiguous():
            raise MmidxError(N.ERR_WRONG_DIM, "The dimensionality of the vector is wrong!")
        st = torch.cuda.current_stream(out.device).cuda_stream
        N.check(N.lib().mmidx_linear_copy_rows_device(self._h, int(iid0), out.shape[0], out.data_ptr(), st))
        return out

    def search_ids_batch(self, k, iids):
        """computeNearestNeighborsInternal(k, int iid) for many ids at once (Linear.java:181-184): the stored vectors are
        the queries, gathered on the device"""
        q = np.ascontiguousarray(np.asarray(iids).reshape(-1), np.int32)
        nq = q.shape[0]
        out = np.full((nq, max(k, 1)), -1, np.int32)
        dists = np.full((nq, max(k, 1)), np.inf, np.float64)
        counts = np.zeros(nq, np.int32)
        N.check(N.lib().mmidx_linear_search_ids(self._h, k, nq, q.ctypes.data, out.ctypes.data, dists.ctypes.data, counts.ctypes.data))
        return out, dists, counts

    def computeNearestNeighborsInternalById(self, k, iid):
        # Linear.java:181-186: the stored vector of iid is the query (it never leaves the device)
        iids, dists, counts = self.search_ids_batch(k, [int(iid)])
        n = int(counts[0])
        return iids[0, :n].copy(), dists[0, :n].copy()

    def set_option(self, name, value):
        """"exact", "mfma_qcap", "debug_sync" (include/mmidx.h, Linear section)"""
        N.check(N.lib().mmidx_linear_set_option(self._h, name.encode(), int(value)))

    def get_stats(self):
        s = N.LinearStats()
        N.check(N.lib().mmidx_linear_get_stats(self._h, C.byref(s)))
        return {f: getattr(s, f) for f, _ in s._fields_}

    def getVector(self, iid):
        """Linear.getVector, Linear.java:253-263"""
        out = np.zeros(self.vectorLength, np.float64)
        N.check(N.lib().mmidx_linear_get_vector(self._h, int(iid), out.ctypes.data))
        return out

    def size(self):
        n = C.c_int64(0)
        N.check(N.lib().mmidx_linear_size(self._h, C.byref(n)))
        return n.value

    def reindex(self, targets, iid0=None, n=None, pca=None, normalize=2, chunk_rows=0):
        """The walk of IndexTransformation.java:111-123 / PCAProjectionExample.java:74-88 as one native call
        (mmidx_linear_reindex): rows iid0 .. iid0 + n - 1 of this index, projected through `pca` (a frontend.PCA) where given,
        truncated to every target's vectorLength, L2-normalised by `normalize` (0 never, 1 always, 2 where the target is
        shorter; one value or one per target) and appended to the targets (Linear / PQ / IVFPQ mirrors) -- nothing leaves HBM.
        iid0 defaults to the targets' common loadCounter, n to the rest of this index.  The ids go with the rows
        (fromIndex.getId(i) -> the target's maps, :114, :121): a row of this index without an id gets none.  Refused before the
        native call, with the reference's messages: an id already indexed in a target, a target whose maxNumVectors would be
        passed.  The targets' loadCounter and maps change only after the native call has succeeded.  Returns n."""
        targets = list(targets)
        if iid0 is None:
            counters = {t.loadCounter for t in targets}
            if len(counters) != 1:
                raise MmidxError(N.ERR_INVALID_ARG, f"the targets hold different numbers of vectors ({sorted(counters)}): give iid0")
            iid0 = counters.pop()
        iid0 = int(iid0)
        n = self.loadCounter - iid0 if n is None else int(n)
        modes = [int(normalize)] * len(targets) if np.isscalar(normalize) else [int(v) for v in normalize]
        if len(modes) != len(targets):
            raise MmidxError(N.ERR_INVALID_ARG, "one normalize value, or one per target")
        ids = [self.getId(i) for i in range(iid0, iid0 + max(n, 0))]
        for t in targets:
            if t.loadCounter + max(n, 0) > t.maxNumVectors:
                raise MmidxError(N.ERR_CAPACITY, "Maximum index capacity reached, no more vectors can be indexed!")
            for id_ in ids:
                if id_ is not None and t.isIndexed(id_):
                    raise MmidxError(N.ERR_INVALID_ARG, f"Vector '{id_}' already indexed!")
        kinds = np.array([0 if isinstance(t, Linear) else 1 for t in targets], np.int32)
        handles = (C.c_void_p * len(targets))(*[t._h for t in targets])
        mode_arr = np.array(modes, np.int32)
        N.check(N.lib().mmidx_linear_reindex(self._h, iid0, n, pca._h if pca is not None else None, len(targets), kinds.ctypes.data,
                                             C.addressof(handles), mode_arr.ctypes.data, int(chunk_rows)))
        for t in targets:
            for i, id_ in enumerate(ids):
                if id_ is not None:
                    t._iid_to_id[iid0 + i] = id_
                    t._id_to_iid[id_] = iid0 + i
            t.loadCounter = iid0 + n
        return n

    def close(self):
        if self._h:
            N.lib().mmidx_linear_destroy(self._h)
            self._h = None


class IndexTransformation:
    """IndexTransformation.java:61-125: a full-length Linear index into a shorter Linear, a PQ or an IVFPQ one."""

    @staticmethod
    def transform(fromIndex, toIndex, chunk_rows=0):
        """The loop of :111-123: every vector of fromIndex, its first toIndex.vectorLength entries (:117), L2-normalised when
        that was a truncation (:118-120), indexed in toIndex under the same id (:121).  A toIndex that already holds the first
        rows is brought up to date.  Returns the number of vectors moved."""
        return fromIndex.reindex([toIndex], normalize=2, chunk_rows=chunk_rows)


class PCAProjection:
    """PCAProjectionExample.java:74-88: project every vector once, index its truncations."""

    @staticmethod
    def project(fullVectors, pca, projectedVectors, L2Normalization=True, chunk_rows=0):
        """Every vector of the Linear index fullVectors through pca.sampleToEigenSpace (:79), truncated to the length of each
        Linear index of projectedVectors (:82), L2-normalised on request (:83-85) and indexed there under its id (:86)."""
        return fullVectors.reindex(list(projectedVectors), pca=pca, normalize=1 if L2Normalization else 0, chunk_rows=chunk_rows)
